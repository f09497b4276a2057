"""Contexts of 17 .. 64 tokens as far as they can be seen without a device: mdt_create's validation accepts every configuration
of tests/long_context_configs.py and refuses, with a message that names the rule, what lies outside the envelope; the facade's
state_dict is the reference's at the five contexts a list was recorded for; the LDS rule of the attention kernels, restated from
the header's text, is the library's at every case's shapes."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib
from tests.helpers import cfg_of, load_fixture
from tests.long_context_configs import CTX_ENVELOPE, CTX_GOLDEN, CTX_REFUSED_AT_CREATE, CTX_SHAPES, attn_chunk_lds, context_len


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(CTX_ENVELOPE))
def test_create_accepts_every_long_context_configuration(name):
    """Without a GPU every configuration gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or
    MDT_ERR_UNSUPPORTED (2)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = CTX_ENVELOPE[name]
    lib = _lib.load()
    cfg = GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])
    sig_tok = int(not cfg.use_ada_conditioning)
    assert sig_tok + 1 + cfg.n_obs_token + cfg.use_proprio == context_len(name) and 17 <= context_len(name) <= 64
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_the_table_covers_the_shapes_it_names():
    """(Ta, Te, head dim) of the twelve cases."""
    assert CTX_SHAPES == {"ctx17_hd48": (10, 17, 48), "ctx64_hd48": (10, 64, 48), "ctx31_h3_d144": (10, 31, 48), "ctx33_rope_hd64": (10, 33, 64),
                          "ctx64_rope_hd32": (10, 64, 32), "ctx32_plain": (10, 32, 48), "ctx24_noise": (10, 24, 48), "ctx40_ta48": (48, 40, 48),
                          "ctx64_ta64_hd64": (64, 64, 64), "ctx34_proprio_mlp_head": (10, 34, 48), "ctx40_no_goal": (10, 40, 32),
                          "ctx18_a64": (10, 18, 48)}


def test_create_refuses_what_lies_outside_the_envelope_and_names_the_rule():
    """Head dim 16 keeps 1 .. 16 tokens, nothing goes past 64, RoPE still needs head dim 32: each refusal comes back before any
    allocation (with or without a GPU) with its status and a message that names the limit."""
    lib = _lib.load()
    for bad, status in CTX_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.MDTConfig(**bad)
        assert lib.mdt_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        msg = lib.mdt_last_error()
        assert b"64" in msg or b"head dim" in msg, (bad, msg)
    h = C.c_void_p()
    cfg = _lib.MDTConfig(**CTX_REFUSED_AT_CREATE[0][0])
    assert lib.mdt_create(C.byref(cfg), C.byref(h)) == 2
    assert b"context length 17 tokens at head dim 16" in lib.mdt_last_error()
    assert b"a context of 17..64 tokens needs head dim 32 / 48 / 64; head dim 16 takes 1..16" in lib.mdt_last_error()
    cfg = _lib.MDTConfig(**CTX_REFUSED_AT_CREATE[1][0])
    assert lib.mdt_create(C.byref(cfg), C.byref(h)) == 2
    assert b"context length 65 tokens" in lib.mdt_last_error() and b"<= 64" in lib.mdt_last_error()


def test_head_dim_16_keeps_its_16_tokens():
    """goal + 15 state tokens at head dim 16 pass the validation as before (status 4 without a GPU, 0 with one)."""
    lib = _lib.load()
    cfg = _lib.MDTConfig(**dict(CTX_REFUSED_AT_CREATE[0][0], n_obs_token=15))
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st in (0, 4), (st, lib.mdt_last_error())
    if st == 0:
        lib.mdt_destroy(h)


@pytest.mark.parametrize("name", CTX_GOLDEN)
def test_facade_state_dict_matches_the_reference_at_long_contexts(name):
    """Names, shapes and order of the facade's state_dict against the list the reference recorded (pos_emb grows with
    n_obs_token)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    meta, _ = load_fixture(f"g21_ctx_{name}.npz")
    cfg = cfg_of(meta)
    assert cfg == CTX_ENVELOPE[name]["cfg"]
    m = GCDenoiser(cfg, sigma_data=0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    pos = dict((k, s) for k, s in meta["state_dict"])["inner_model.pos_emb"]
    assert pos[1] >= cfg["goal_seq_len"] + cfg["n_obs_token"] + cfg["action_seq_len"]


def test_the_lds_rule_restated_from_the_header_is_the_librarys():
    """include/mdt_hip_debug.h states the bytes of LDS of one workgroup; tests/long_context_configs.py restates them.  At every
    case's (Ta, Te, head dim): the decoder's cross-attention with its visible prefix Tv = min(Ta, Te) and with every key, the
    encoder's self-attention (Te x Te) and the decoder's (Ta x Ta), forward and backward -- all within the 160 KiB of a CU, and the
    prefix form never above the full-key form."""
    lds = _lib.load().mdt_op_attn_chunk_lds
    worst = {0: 0, 1: 0}
    for name, (Ta, Te, hd) in CTX_SHAPES.items():
        for bwd in (0, 1):
            for Tq, Tv in ((Ta, min(Ta, Te)), (Ta, Te), (Te, Te), (Ta, Ta)):
                want = attn_chunk_lds(hd, Tq, Tv, bool(bwd))
                assert lds(hd, Tq, Tv, bwd) == want, (name, Tq, Tv, bwd)
                assert want <= 160 * 1024
                worst[bwd] = max(worst[bwd], want)
            assert attn_chunk_lds(hd, Ta, min(Ta, Te), bool(bwd)) <= attn_chunk_lds(hd, Ta, Te, bool(bwd))
    assert worst == {0: 52224, 1: 104448}   # 64 x 64 at head dim 64
    # Ta = 10, Te = 64, head dim 48: one key tile staged instead of four
    assert (attn_chunk_lds(48, 10, 10, False), attn_chunk_lds(48, 10, 64, False)) == (10496, 29696)
