"""Action vectors of 17 .. 64 elements as far as they can be seen without a device: mdt_create's validation accepts every
configuration of tests/wide_action_configs.py and refuses, with a message that names the rule, what lies outside 1 .. 64; the
facade's state_dict is the reference's at the five widths a list was recorded for (17, 20, 24, 48, 64)."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib
from tests.helpers import cfg_of, load_fixture
from tests.wide_action_configs import WIDE_ENVELOPE, WIDE_GOLDEN, WIDE_REFUSED_AT_CREATE


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(WIDE_ENVELOPE))
def test_create_accepts_every_wide_action_configuration(name):
    """Without a GPU every configuration gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or
    MDT_ERR_UNSUPPORTED (2)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = WIDE_ENVELOPE[name]
    lib = _lib.load()
    cfg = GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])
    assert 17 <= cfg.action_dim <= 64
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_create_refuses_widths_outside_1_to_64_and_names_the_rule():
    """65 and 0 come back before any allocation (with or without a GPU) as MDT_ERR_UNSUPPORTED with the width and the range."""
    lib = _lib.load()
    for bad, status in WIDE_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.MDTConfig(**bad)
        assert lib.mdt_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        assert lib.mdt_last_error() == b"action_dim %d: supported 1..64" % bad["action_dim"], (bad, lib.mdt_last_error())


def test_the_top_of_the_range_passes_the_validation():
    """action_dim = 64 on the plain configuration fields (status 4 without a GPU, 0 with one)."""
    lib = _lib.load()
    cfg = _lib.MDTConfig(**dict(WIDE_REFUSED_AT_CREATE[0][0], action_dim=64))
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st in (0, 4), (st, lib.mdt_last_error())
    if st == 0:
        lib.mdt_destroy(h)


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_facade_state_dict_matches_the_reference_at_wide_actions(name):
    """Names, shapes and order of the facade's state_dict against the list the reference recorded: action_emb.weight is
    (embed_dim, action_dim), the last layer of action_pred (action_dim, .)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    meta, _ = load_fixture(f"g20_wide_{name}.npz")
    cfg = cfg_of(meta)
    assert cfg == WIDE_ENVELOPE[name]["cfg"] and meta["proprio"] == WIDE_ENVELOPE[name]["proprio"]
    m = GCDenoiser(cfg, sigma_data=0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    shapes = dict((k, s) for k, s in meta["state_dict"])
    assert shapes["inner_model.action_emb.weight"] == [cfg["embed_dim"], cfg["action_dim"]]
    last = "inner_model.action_pred.weight" if cfg["linear_output"] else "inner_model.action_pred.2.weight"
    assert shapes[last][0] == cfg["action_dim"] > 16
