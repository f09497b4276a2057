"""The configurations of tests/deep_row_configs.py as far as they can be seen without a device: mdt_create's validation accepts
every one, and the row counts tests/test_route_table.py ties to the routes are those of the configuration the library is handed."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib
from tests.deep_row_configs import DEEP_BATCHES, DEEP_ENVELOPE, DEEP_REUSE, rows_of


def hip_config(name):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = DEEP_ENVELOPE[name]
    return GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(DEEP_ENVELOPE))
def test_create_accepts_every_deep_row_configuration(name):
    """Without a GPU every configuration gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or
    MDT_ERR_UNSUPPORTED (2)."""
    lib = _lib.load()
    cfg = hip_config(name)
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


@pytest.mark.parametrize("name", sorted(DEEP_ENVELOPE))
def test_rows_of_counts_the_tokens_the_library_is_configured_for(name):
    cfg, e = hip_config(name), DEEP_ENVELOPE[name]
    tokens = cfg.goal_seq_len + (cfg.n_obs_token if cfg.arch == 0 else 2) + (1 if e["proprio"] else 0)
    for B in DEEP_BATCHES[name]:
        assert rows_of(name, B) == (B * tokens, B * cfg.action_seq_len)
    assert cfg.embed_dim % cfg.n_heads == 0 and cfg.embed_dim // cfg.n_heads in (32, 48, 64)


def test_the_batches_are_the_row_counts_they_are_named_for():
    assert [rows_of("ta64_a64", B)[1] for B in DEEP_BATCHES["ta64_a64"]] == [4096, 5120, 8128, 8192]
    assert rows_of("ta64_a64_d192", 128)[1] == 8192 and rows_of("ta64_a64_d256", 64)[1] == 4096 and rows_of("ctx64", 128)[0] == 8192
    assert rows_of("a64_rows2600", 260)[1] == 2600 and rows_of("a17_mlp_proprio_rows2600", 260) == (1300, 2600)
    assert rows_of("mdt_ta40", 205)[1] == 8200
    assert DEEP_REUSE[2] < DEEP_REUSE[1] and DEEP_REUSE[1] in DEEP_BATCHES[DEEP_REUSE[0]]
