"""Action chunks of 17 .. 64 steps as far as they can be seen without a device: mdt_create's validation accepts every
configuration of tests/long_chunk_configs.py and refuses, with a message that names the rule, what lies outside the envelope;
the facade's state_dict is the reference's at the four lengths a list was recorded for (17, 33, 40, 48)."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib, configs
from tests.helpers import cfg_of, load_fixture
from tests.long_chunk_configs import LONG_ENVELOPE, LONG_GOLDEN, LONG_REFUSED_AT_CREATE


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(LONG_ENVELOPE))
def test_create_accepts_every_long_chunk_configuration(name):
    """Without a GPU every configuration gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or
    MDT_ERR_UNSUPPORTED (2)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = LONG_ENVELOPE[name]
    lib = _lib.load()
    cfg = GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])
    assert 17 <= cfg.action_seq_len <= 64
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_create_refuses_what_lies_outside_the_envelope_and_names_the_rule():
    """Head dim 16 keeps 1 .. 16, nothing goes past 64, RoPE still needs head dim 32: each refusal comes back before any
    allocation (with or without a GPU) with its status and a message that names the limit."""
    lib = _lib.load()
    for bad, status in LONG_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.MDTConfig(**bad)
        assert lib.mdt_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        msg = lib.mdt_last_error()
        assert b"64" in msg or b"head dim" in msg, (bad, msg)
    # the two new refusals spell the rule out
    h = C.c_void_p()
    cfg = _lib.MDTConfig(**LONG_REFUSED_AT_CREATE[0][0])
    assert lib.mdt_create(C.byref(cfg), C.byref(h)) == 2
    assert b"action_seq_len 17..64 needs head dim 32 / 48 / 64; head dim 16 takes 1..16" in lib.mdt_last_error()
    cfg = _lib.MDTConfig(**LONG_REFUSED_AT_CREATE[1][0])
    assert lib.mdt_create(C.byref(cfg), C.byref(h)) == 2
    assert b"<= 64" in lib.mdt_last_error()


def test_head_dim_16_keeps_its_16_rows():
    """action_seq_len = 16 at head dim 16 passes the validation as before (status 4 without a GPU, 0 with one)."""
    lib = _lib.load()
    cfg = _lib.MDTConfig(**dict(LONG_REFUSED_AT_CREATE[0][0], action_seq_len=16))
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st in (0, 4), (st, lib.mdt_last_error())
    if st == 0:
        lib.mdt_destroy(h)


@pytest.mark.parametrize("name", LONG_GOLDEN)
def test_facade_state_dict_matches_the_reference_at_long_chunks(name):
    """Names, shapes and order of the facade's state_dict against the list the reference recorded (pos_emb grows with the
    chunk)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    meta, _ = load_fixture(f"g19_long_{name}.npz")
    cfg = cfg_of(meta)
    assert cfg == LONG_ENVELOPE[name]["cfg"]
    m = GCDenoiser(cfg, sigma_data=0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    pos = dict((k, s) for k, s in meta["state_dict"])["inner_model.pos_emb"]
    assert pos[1] >= cfg["action_seq_len"] + cfg["goal_seq_len"]


def test_facade_state_dict_at_64_steps():
    """The facade against ITSELF at the top of the range (no reference list was recorded at 64 steps; the reference's lists are the
    four of the test above, at 17 / 33 / 40 / 48): pos_emb has goal_seq_len + obs tokens + 64 rows (MDT-V) / goal_seq_len + 64 rows
    (MDT) -- the rule those four lists follow -- and every other shape is that of the 10-step model.  A consistency check of the
    constructor, not new ground: it holds without the long-chunk kernels."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    for factory, rows in ((configs.mdtv_default, 1 + 3 + 64), (configs.mdt_default, 1 + 64)):
        short = {k: tuple(v.shape) for k, v in GCDenoiser(factory(), 0.5).state_dict().items()}
        long_ = {k: tuple(v.shape) for k, v in GCDenoiser(factory(action_seq_len=64), 0.5).state_dict().items()}
        assert list(short) == list(long_)
        assert long_["inner_model.pos_emb"][1] == rows
        assert {k for k in short if short[k] != long_[k]} == {"inner_model.pos_emb"}
