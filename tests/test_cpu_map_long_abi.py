"""The MAP pooling block at 17 .. 64 tokens as far as it can be seen without a device: mdt_map_pool_create accepts every case of
tests/map_long_configs.py, the facade's state_dict is the reference's at the recorded cases, the three hooks of
include/mdt_hip_debug.h have the prototypes the header declares, the LDS rule of the (sample, head group) kernels, restated from the
header's text, is the library's over the whole constructor envelope, and 0 / 65 tokens are refused with a text that names 1..64.
What needs a handle (the refusals of mdt_map_pool_forward itself) is in tests/test_gpu_map_long.py."""
import ctypes as C
import os
import re

import pytest
import torch

from mdt_policy_amd import _lib
from tests import map_long_configs as L
from tests.helpers import load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # an aligned address no call may dereference: every refusal below comes back before anything is enqueued


def _map_config(kw):
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    return _lib.MapPoolConfig(**MAPBlock(**kw)._cfg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(L.MAP_LONG))
def test_map_pool_create_accepts_every_long_case(name):
    """Without a GPU every case gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or MDT_ERR_UNSUPPORTED (2)."""
    lib = _lib.load()
    cfg = _map_config(L.MAP_LONG[name]["kwargs"])
    h = C.c_void_p()
    st = lib.mdt_map_pool_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_the_table_is_the_one_the_kernels_were_built_for():
    """(tokens, head dim, heads per workgroup) of the six cases; every case above 16 tokens, none above 64; the batches reach 8192
    token rows where the block is narrow."""
    got = {}
    for name, c in L.MAP_LONG.items():
        kw = c["kwargs"]
        H = 2 * kw["n_heads"]
        got[name] = (c["N"], kw["output_dim"] // H, L.head_group(kw["output_dim"], H))
        assert 16 < c["N"] <= L.MAP_TOKEN_LIMIT and c["batches"][0] == 1 and 2 <= c["train_b"] <= 5
        assert int(kw["mlp_ratio"] * kw["output_dim"]) % 16 == 0
    assert got == {"clip_n34": (34, 24, 4), "q16_hd256_n64": (64, 256, 1), "q16_h64_n64": (64, 8, 8), "hd3_n17": (17, 3, 8),
                   "hd1_n63": (63, 1, 8), "clip_n18": (18, 24, 4)}
    for name in ("hd3_n17", "hd1_n63"):
        assert max(L.MAP_LONG[name]["batches"]) * L.MAP_LONG[name]["N"] >= 8192


@pytest.mark.parametrize("name", sorted(L.MAP_LONG_GOLDEN))
def test_facade_state_dict_matches_the_reference(name):
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    meta, _ = load_fixture(f"g22_map_long_{name}.npz")
    m = MAPBlock(**meta["kwargs"])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in meta["state_dict"]]


def test_the_hooks_have_the_prototypes_the_header_declares():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_debug.h")).read(), flags=re.S)
    protos = {n: (r, [a.strip() for a in args.split(",")])
              for r, n, args in re.findall(r"\b(mdt_status|int64_t)\s+(mdt_op_map_attn_[a-z]+)\s*\(([^)]*)\)\s*;", src)}
    kinds = lambda args: ["ptr" if "*" in a else a.split()[0] for a in args]  # noqa: E731
    assert protos["mdt_op_map_attn_fwd"][0] == "mdt_status"
    assert kinds(protos["mdt_op_map_attn_fwd"][1]) == ["int32_t"] + ["ptr"] * 4 + ["int64_t"] + ["int32_t"] * 4 + ["ptr"]
    assert protos["mdt_op_map_attn_bwd"][0] == "mdt_status"
    assert kinds(protos["mdt_op_map_attn_bwd"][1]) == ["int32_t"] + ["ptr"] * 6 + ["int64_t"] + ["int32_t"] * 4 + ["ptr"]
    assert protos["mdt_op_map_attn_lds"] == ("int64_t", ["int32_t Q", "int32_t N", "int32_t D", "int32_t H", "int32_t bwd"])
    table = {n: (r, a) for n, r, a in _lib.SYMBOLS}
    I32, I64, VP = C.c_int32, C.c_int64, C.c_void_p
    assert table["mdt_op_map_attn_fwd"] == (I32, [I32, VP, VP, VP, VP, I64, I32, I32, I32, I32, VP])
    assert table["mdt_op_map_attn_bwd"] == (I32, [I32, VP, VP, VP, VP, VP, VP, I64, I32, I32, I32, I32, VP])
    assert table["mdt_op_map_attn_lds"] == (I64, [I32] * 5)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in protos)


def test_the_lds_rule_restated_from_the_header_is_the_librarys():
    """Every (output_dim, heads) mdt_map_pool_create accepts, Q = 1 and 16, N = 1, 17, 34 and 64, forward and backward: the hook
    returns the header's formula, and the formula never leaves the 160 KiB of a CU -- there is no LDS refusal above 16 tokens."""
    lds = _lib.load().mdt_op_map_attn_lds
    worst = {0: (0,), 1: (0,)}
    for D in range(16, 513, 16):
        for H in range(2, D + 1, 2):
            if D % H:
                continue
            for Q in (1, 16):
                for N in (1, 17, 34, 64):
                    for bwd in (0, 1):
                        want = L.map_long_lds_bytes(Q, N, D, H, bool(bwd))
                        assert lds(Q, N, D, H, bwd) == want, (Q, N, D, H, bwd)
                        worst[bwd] = max(worst[bwd], (want, D, H))
    assert worst == {0: (86272, 512, 2), 1: (114944, 512, 32)} and worst[1][0] <= L.MAP_LONG_LDS_LIMIT
    # the numbers the header quotes
    assert (L.map_long_lds_bytes(16, 64, 512, 2, False), L.map_long_lds_bytes(16, 64, 512, 2, True)) == (86272, 106752)
    assert (L.map_long_lds_bytes(16, 64, 512, 32, False), L.map_long_lds_bytes(16, 64, 512, 32, True)) == (73984, 114944)
    assert (L.map_long_lds_bytes(1, 34, 384, 16, False), L.map_long_lds_bytes(1, 34, 384, 16, True)) == (14120, 15048)
    for name, c in L.MAP_LONG.items():
        kw = c["kwargs"]
        for bwd in (0, 1):
            assert lds(kw["n_latents"], c["N"], kw["output_dim"], 2 * kw["n_heads"], bwd) == \
                L.map_long_lds_bytes(kw["n_latents"], c["N"], kw["output_dim"], 2 * kw["n_heads"], bool(bwd))
    assert lds(1, 34, 384, 7, 0) == -1   # 7 heads do not divide 384 channels


def test_zero_and_65_tokens_are_refused_before_anything_is_enqueued():
    """Both hooks, the family the block runs above 16 tokens: MDT_ERR_UNSUPPORTED (2) with a text that names 1..64; the
    one-workgroup-per-sample family stops at 16 tokens and keeps its "LDS budget" text for 16 latents x 512 channels."""
    lib = _lib.load()
    for N in (0, 65, -3):
        assert lib.mdt_op_map_attn_fwd(1, FAKE, FAKE, FAKE, None, 2, 1, N, 384, 16, None) == 2
        assert b"1..64 tokens" in lib.mdt_last_error() and str(N).encode() in lib.mdt_last_error()
        assert lib.mdt_op_map_attn_bwd(1, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 1, N, 384, 16, None) == 2
        assert b"1..64 tokens" in lib.mdt_last_error()
    assert lib.mdt_op_map_attn_fwd(0, FAKE, FAKE, FAKE, None, 2, 1, 17, 384, 16, None) == 2
    assert b"1..16 tokens" in lib.mdt_last_error()
    assert lib.mdt_op_map_attn_fwd(0, FAKE, FAKE, FAKE, None, 1, 16, 16, 512, 16, None) == 2
    assert b"LDS budget" in lib.mdt_last_error()
    # bad arguments: a third family, a null or misaligned pointer, heads that do not divide the channels
    assert lib.mdt_op_map_attn_fwd(2, FAKE, FAKE, FAKE, None, 2, 1, 34, 384, 16, None) == 1
    assert lib.mdt_op_map_attn_fwd(1, None, FAKE, FAKE, None, 2, 1, 34, 384, 16, None) == 1
    assert lib.mdt_op_map_attn_fwd(1, FAKE, FAKE + 4, FAKE, None, 2, 1, 34, 384, 16, None) == 1
    assert lib.mdt_op_map_attn_bwd(1, FAKE, FAKE, FAKE, FAKE, None, FAKE, 2, 1, 34, 384, 16, None) == 1
    assert lib.mdt_op_map_attn_fwd(1, FAKE, FAKE, FAKE, None, 2, 17, 34, 384, 16, None) == 1
    assert lib.mdt_op_map_attn_fwd(1, FAKE, FAKE, FAKE, None, 2, 1, 34, 384, 14, None) == 1
    # the handle entry points refuse a null handle before they look at the token count
    assert lib.mdt_map_pool_forward(None, FAKE, 1, 65, FAKE, None) == 1
