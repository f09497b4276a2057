"""The decoder's cross-attention at contexts above 16 tokens (pytest -m gpu): the three attention ops with a visible prefix, through
the hooks of include/mdt_hip_debug.h (mdt_op_attention_prefix, mdt_op_attn_fwd_train_prefix, mdt_op_attn_bwd_prefix), against
float64 torch in the guarded, padded layouts of tests/test_gpu_long_attention_ops.py and at that file's tolerances.

A launch with kv_rows = min(Tq, Tk) stages and multiplies the first kv_rows keys of every sample; Tk stays the k / v sample stride
and the row length of the dropout index, so tests/dropout_masks.py replays the masks of a (B, H, Tq, Tk) site unmodified.  The twin
of every call fills the k / v rows >= kv_rows of every sample with NaN (the guard bands hold NaN already): the outputs and dq must
have the bits of the call on finite rows, and rows >= kv_rows of dk / dv must be exactly zero (accumulate_kv: keep their bits) --
the prefix form reads and writes what it says."""
import ctypes as C

import pytest
import torch

from tests import dropout_masks as DM
from tests.guarded import NAN, same_bits
from tests.helpers import assert_close
from tests.test_gpu_long_attention_ops import TOL_ATTN, operands, rope_tables
from tests.test_gpu_ops import ref_attn, stream
from tests.test_gpu_ops_bounds import Lay, seeded
from tests.test_gpu_train_ops import G_TOL, _rot
from tests.test_gpu_train_ops_bounds import SEED, SITE, TOL_ATTN_FWD, TOL_FWD, agree, both

pytestmark = pytest.mark.gpu

# (Tq, Tk, kv_rows): Ta = 10 against 17 and 64 tokens, a full query tile, two query tiles, Te < Ta, the top of the range (kv_rows =
# Tk: the full-key launch), one query
SHAPES = [(10, 17, 10), (10, 64, 10), (16, 33, 16), (24, 40, 24), (48, 40, 40), (64, 64, 64), (1, 64, 1)]
HDS = [32, 48, 64]
H = 3


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def poisoned(t, n, Tk, kvr):
    """(n * Tk, cols) rows with rows >= kvr of every sample NaN."""
    t = t.clone().view(n, Tk, -1)
    t[:, kvr:] = NAN
    return t.view(n * Tk, -1)


def run_inference(lib, q, k, v, B, hd, Tq, Tk, kvr, rope, div, what):
    Dm = H * hd

    def call(guarded, k_, v_, rows):
        L = Lay(guarded)
        qp, kp, vp, ldq, ldkv = operands(L, "kv", B, Tq, Tk, Dm, q, k_, v_)
        out = L.out("out", B * Tq, Dm, pad=4)
        a = lib.AttnArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, out=out.ptr, ldo=out.ld, B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=1, rope=rope)
        lib.check(lib.load().mdt_op_attention_prefix(C.byref(a), div, rows, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        return {"out": out.host()}

    dense, got = both(lambda g: call(g, k, v, kvr))
    agree(got, dense, what)
    twin = call(True, poisoned(k, B // div, Tk, kvr), poisoned(v, B // div, Tk, kvr), kvr)
    assert same_bits(twin["out"], got["out"]), f"{what}: k / v rows >= kv_rows reached the result"
    full = call(True, k, v, 0)
    return got["out"], full["out"]


@pytest.mark.parametrize("Tq,Tk,kvr", SHAPES)
@pytest.mark.parametrize("hd", HDS)
def test_inference_attention_reads_the_visible_prefix_only(lib, hd, Tq, Tk, kvr):
    """mdt_op_attention_prefix, causal: RoPE off and on, ctx_div 1 (B = 2) and 3 (six query samples over two contexts); the prefix
    launch and the full-key launch (kv_rows = 0) against float64, and the NaN twin's bits."""
    Dm = H * hd
    for rope in (0, 1):
        for div, B in ((1, 2), (3, 6)):
            g = seeded("context attention", hd, Tq, Tk, rope, div)
            q = torch.randn(B, Tq, Dm, generator=g)
            k, v = (torch.randn(B // div, Tk, Dm, generator=g) for _ in range(2))
            want = ref_attn(q, k.repeat_interleave(div, 0), v.repeat_interleave(div, 0), H, True, rope=bool(rope))
            what = f"prefix attention hd {hd}, {Tq} x {Tk} / {kvr}, rope {rope}, ctx_div {div}"
            got, full = run_inference(lib, q.reshape(-1, Dm), k.reshape(-1, Dm), v.reshape(-1, Dm), B, hd, Tq, Tk, kvr, rope, div, what)
            assert_close(got.reshape(B, Tq, Dm), want, what=what, **TOL_ATTN)
            assert_close(full.reshape(B, Tq, Dm), want, what=what + ", every key", **TOL_ATTN)


@pytest.mark.parametrize("Tq,Tk,kvr", SHAPES)
@pytest.mark.parametrize("hd", HDS)
def test_training_attention_forward_and_backward_on_the_visible_prefix(lib, hd, Tq, Tk, kvr):
    """mdt_op_attn_fwd_train_prefix and mdt_op_attn_bwd_prefix at B = 2, causal: RoPE off and on, p = 0 and p = 0.3 against float64
    with the restated mask of the (B, H, Tq, Tk) site, accumulate_kv 0 and 1; the NaN twin's bits and the rows of dk / dv no query
    sees."""
    B, Dm = 2, H * hd
    g = seeded("context train attention", hd, Tq, Tk)
    q, k, v = (torch.randn(B * T, Dm, generator=g) for T in (Tq, Tk, Tk))
    do, dkv0 = torch.randn(B * Tq, Dm, generator=g), torch.randn(B * Tk, 2 * Dm, generator=g)
    rc, rs = rope_tables()
    split = lambda t, T: t.view(B, T, H, hd).transpose(1, 2)
    dead = torch.zeros(B, Tk, dtype=torch.bool)
    dead[:, kvr:] = True
    dead = dead.view(-1)
    for rope in (0, 1):
        for p in (0.0, 0.3):
            mask = torch.from_numpy(DM.scale(SEED, SITE, (B, H, Tq, Tk), p)) if p else 1.0
            q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
            att = _rot(split(q64, Tq), rope) @ _rot(split(k64, Tk), rope).transpose(-1, -2) / hd ** 0.5
            att = att.masked_fill(~torch.ones(Tq, Tk, dtype=torch.bool).tril(), float("-inf"))
            y = ((att.softmax(-1) * mask) @ split(v64, Tk)).transpose(1, 2).reshape(B * Tq, Dm)
            y.backward(do.double())
            assert not k64.grad[dead].any() and not v64.grad[dead].any()   # float64 agrees: no query sees those keys
            for acc in (0, 1):
                what = f"prefix training attention hd {hd}, {Tq} x {Tk} / {kvr}, rope {rope}, p {p}, accumulate_kv {acc}"

                def run(guarded, k_=k, v_=v):
                    L = Lay(guarded)
                    qp, kp, vp, ldq, ldkv = operands(L, "kv", B, Tq, Tk, Dm, q, k_, v_)
                    dqo, grad = L.out("dq", B * Tq, Dm, pad=4), L.out("dkv", B * Tk, 2 * Dm, pad=4, fill=dkv0 if acc else None)
                    out, dod = L.out("out", B * Tq, Dm, pad=4), L.inp("d_out", do, pad=4)
                    rcd, rsd = L.inp("rope_cos", rc), L.inp("rope_sin", rs)
                    kw = dict(B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=1, p=p, site=SITE, seed=SEED, rope=rope, rope_cos=rcd.ptr, rope_sin=rsd.ptr)
                    a = lib.AttnTrainArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, out=out.ptr, ldo=out.ld, **kw)
                    lib.check(lib.load().mdt_op_attn_fwd_train_prefix(C.byref(a), kvr, stream()))
                    L.check(what + ": forward")
                    out.check(what + ": out", written=True)
                    gb = lib.AttnBwdArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, d_out=dod.ptr, ld_do=dod.ld, dq=dqo.ptr, ld_dq=dqo.ld,
                                         dk=grad.at(0, 0), dv=grad.at(0, Dm), ld_dkv=grad.ld, accumulate_kv=acc, **kw)
                    lib.check(lib.load().mdt_op_attn_bwd_prefix(C.byref(gb), kvr, stream()))
                    L.check(what + ": backward")
                    r = {"out": out.host(), "dq": dqo.host(), "dkv": grad.host()}
                    for name, t in r.items():
                        assert not t.isnan().any(), f"{what}: NaN left in {name}"
                    return r

                dense, got = both(run)
                agree(got, dense, what)
                assert_close(got["out"], y.detach(), what=what + ": out", **(TOL_FWD if p else TOL_ATTN_FWD))
                assert_close(got["dq"], q64.grad, what=what + ": dq", **G_TOL)
                base = dkv0.double() if acc else torch.zeros(B * Tk, 2 * Dm, dtype=torch.float64)
                assert_close(got["dkv"][:, :Dm].double() - base[:, :Dm], k64.grad, what=what + ": dk", **G_TOL)
                assert_close(got["dkv"][:, Dm:].double() - base[:, Dm:], v64.grad, what=what + ": dv", **G_TOL)
                if acc:
                    assert same_bits(got["dkv"][dead], dkv0[dead]), f"{what}: dk / dv rows >= kv_rows were touched"
                else:
                    assert same_bits(got["dkv"][dead], torch.zeros(int(dead.sum()), 2 * Dm)), f"{what}: dk / dv rows >= kv_rows are not +0"
                twin = run(True, poisoned(k, B, Tk, kvr), poisoned(v, B, Tk, kvr))
                for name in ("out", "dq", "dkv"):
                    assert same_bits(twin[name], got[name]), f"{what}: k / v rows >= kv_rows reached {name}"


@pytest.mark.parametrize("Tq,Tk,causal,kvr", [(10, 64, 1, 9), (10, 64, 0, 10), (10, 64, 1, 65), (10, 16, 1, 10), (40, 33, 1, 32)])
def test_prefixes_that_would_hide_a_visible_key_are_refused(lib, Tq, Tk, causal, kvr):
    """kv_rows below min(Tq, Tk), a prefix of a non-causal launch, more rows than keys, a prefix at Tk <= 16 (the 16-row kernels
    have no such form): MDT_ERR_INVALID_ARG from each of the three hooks."""
    B, hd = 1, 32
    Dm = H * hd
    t = {n: torch.zeros(B * T, Dm, device="cuda") for n, T in (("q", Tq), ("k", Tk), ("v", Tk), ("out", Tq), ("do", Tq), ("dq", Tq), ("dk", Tk), ("dv", Tk))}
    p = {n: x.data_ptr() for n, x in t.items()}
    Lh = lib.load()
    a = lib.AttnArgs(q=p["q"], ldq=Dm, k=p["k"], v=p["v"], ldkv=Dm, out=p["out"], ldo=Dm, B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=causal, rope=0)
    assert Lh.mdt_op_attention_prefix(C.byref(a), 1, kvr, stream()) == 1
    kw = dict(B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=causal, p=0.0, site=SITE, seed=SEED, rope=0, rope_cos=None, rope_sin=None)
    f = lib.AttnTrainArgs(q=p["q"], ldq=Dm, k=p["k"], v=p["v"], ldkv=Dm, out=p["out"], ldo=Dm, **kw)
    assert Lh.mdt_op_attn_fwd_train_prefix(C.byref(f), kvr, stream()) == 1
    gb = lib.AttnBwdArgs(q=p["q"], ldq=Dm, k=p["k"], v=p["v"], ldkv=Dm, d_out=p["do"], ld_do=Dm, dq=p["dq"], ld_dq=Dm, dk=p["dk"], dv=p["dv"],
                         ld_dkv=Dm, accumulate_kv=0, **kw)
    assert Lh.mdt_op_attn_bwd_prefix(C.byref(gb), kvr, stream()) == 1
    assert b"kv_rows" in Lh.mdt_last_error()
