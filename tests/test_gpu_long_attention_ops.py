"""The three attention ops at 17 .. 64 rows (pytest -m gpu): mdt_op_attention, mdt_op_attn_fwd_train and mdt_op_attn_bwd against
float64 torch, held to their buffers as tests/test_gpu_train_ops_bounds.py::test_training_attention_forward_and_backward holds
the 16-row kernels -- guard bands, padded strides, both layouts, the dense twin's bits -- at that test's tolerances.

Shapes: one row into a second 16-row tile, one short of and one past two tiles, full tiles, the top of the range; rectangular scores
of the decoder's cross-attention (few keys, top-left aligned causal mask) and more keys than queries.  Every case runs H = 1, 3 and
8; the batch alternates between 1 and 3 with the shape, the head dim and the head count, so that each (head dim, H) pair meets both."""
import ctypes as C

import pytest
import torch

from tests import dropout_masks as DM
from tests.guarded import NAN, canary, same_bits
from tests.helpers import assert_close
from tests.test_gpu_ops import ref_attn, stream
from tests.test_gpu_ops_bounds import Lay, seeded
from tests.test_gpu_train_ops import G_TOL, _rot
from tests.test_gpu_train_ops_bounds import SEED, SITE, TOL_ATTN_FWD, TOL_FWD, agree, both

pytestmark = pytest.mark.gpu

SHAPES = [(17, 17), (31, 31), (32, 32), (33, 33), (48, 48), (63, 63), (64, 64), (17, 1), (64, 4), (33, 16), (64, 5), (5, 40)]
HDS = [32, 48, 64]
TOL_ATTN = dict(rtol=1e-4, atol=1e-5)   # the attention tests of tests/test_gpu_ops.py


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


HEADS = (1, 3, 8)


def heads_and_batches(hd, Tq, Tk):
    """(H, B) for every head count."""
    i, j = SHAPES.index((Tq, Tk)), HDS.index(hd)
    return [(H, (1, 3)[(i + j + n) % 2]) for n, H in enumerate(HEADS)]


def rope_tables():
    """(64 positions, 16 frequencies) cos / sin, as the handle uploads them."""
    from oracle.mdt_oracle import rotary_tables
    cos, sin = rotary_tables(64, torch.float64)
    return cos[:, ::2].float().contiguous(), sin[:, ::2].float().contiguous()


def operands(L, layout, B, Tq, Tk, Dm, q, k, v):
    """q / k / v pointers and strides: column blocks of one row of stride 3 Dm + 4 (what neither uses holds NaN), or q rows beside
    separate K | V rows of stride 2 Dm + 4."""
    if layout == "qkv":
        t = torch.full((B * max(Tq, Tk), 3 * Dm), NAN)
        t[:B * Tq, :Dm], t[:k.shape[0], Dm:2 * Dm], t[:k.shape[0], 2 * Dm:] = q, k, v
        src = L.inp("qkv", t, pad=4)
        return src.at(0, 0), src.at(0, Dm), src.at(0, 2 * Dm), src.ld, src.ld
    qs, kvs = L.inp("q", q, pad=4), L.inp("kv", torch.cat([k, v], 1), pad=4)
    return qs.ptr, kvs.at(0, 0), kvs.at(0, Dm), qs.ld, kvs.ld


def run_inference(lib, layout, q, k, v, B, H, hd, Tq, Tk, causal, rope, what, ctx_div=1):
    Dm = H * hd

    def run(guarded):
        L = Lay(guarded)
        qp, kp, vp, ldq, ldkv = operands(L, layout, B, Tq, Tk, Dm, q, k, v)
        out = L.out("out", B * Tq, Dm, pad=4)
        a = lib.AttnArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, out=out.ptr, ldo=out.ld, B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=causal, rope=rope)
        if ctx_div == 1:
            lib.check(lib.load().mdt_op_attention(C.byref(a), stream()))
        else:
            lib.check(lib.load().mdt_op_attention_shared(C.byref(a), ctx_div, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        return {"out": out.host()}

    dense, got = both(run)
    agree(got, dense, what)
    again = run(True)
    assert same_bits(again["out"], got["out"]), f"{what}: two runs differ"
    return got["out"]


@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("hd", HDS)
def test_inference_attention(lib, hd, Tq, Tk):
    """mdt_op_attention: H = 1, 3, 8; causal off and on, RoPE off and on, both layouts."""
    for H, B in heads_and_batches(hd, Tq, Tk):
        inference_case(lib, hd, Tq, Tk, H, B)


def inference_case(lib, hd, Tq, Tk, H, B):
    Dm = H * hd
    g = seeded("long attention", hd, Tq, Tk, H)
    q, k, v = (torch.randn(B, T, Dm, generator=g) for T in (Tq, Tk, Tk))
    for causal in (0, 1):
        for rope in (0, 1):
            want = ref_attn(q, k, v, H, bool(causal), rope=bool(rope))
            for layout in ("qkv", "kv"):
                what = f"attention hd {hd}, H {H}, B {B}, {Tq} x {Tk}, causal {causal}, rope {rope}, {layout}"
                got = run_inference(lib, layout, q.reshape(-1, Dm), k.reshape(-1, Dm), v.reshape(-1, Dm), B, H, hd, Tq, Tk, causal, rope, what)
                assert_close(got.reshape(B, Tq, Dm), want, what=what, **TOL_ATTN)


def test_inference_attention_at_70_samples(lib):
    """B = 70 (where the 16-row kernel splits its heads over two workgroups), H = 8, hd 48, 33 x 33 causal and 64 x 5."""
    H, hd, B = 8, 48, 70
    Dm = H * hd
    for Tq, Tk in ((33, 33), (64, 5)):
        g = seeded("long attention B 70", Tq, Tk)
        q, k, v = (torch.randn(B, T, Dm, generator=g) for T in (Tq, Tk, Tk))
        what = f"attention B 70, {Tq} x {Tk}"
        got = run_inference(lib, "qkv", q.reshape(-1, Dm), k.reshape(-1, Dm), v.reshape(-1, Dm), B, H, hd, Tq, Tk, 1, 0, what)
        assert_close(got.reshape(B, Tq, Dm), ref_attn(q, k, v, H, True), what=what, **TOL_ATTN)


def test_inference_attention_with_shared_contexts(lib):
    """ctx_div = 3 (the candidates of a sampler call): six query samples over two contexts, 40 x 5 causal at hd 48 and 17 x 16 with
    RoPE at hd 64; the k / v buffer holds the two contexts' rows and nothing else."""
    for hd, H, Tq, Tk, rope in ((48, 8, 40, 5, 0), (64, 3, 17, 16, 1)):
        B, div = 6, 3
        Dm = H * hd
        g = seeded("long attention shared", hd, Tq, Tk)
        q = torch.randn(B, Tq, Dm, generator=g)
        k, v = (torch.randn(B // div, Tk, Dm, generator=g) for _ in range(2))
        want = ref_attn(q, k.repeat_interleave(div, 0), v.repeat_interleave(div, 0), H, True, rope=bool(rope))
        what = f"attention with ctx_div 3, hd {hd}, {Tq} x {Tk}"
        got = run_inference(lib, "kv", q.reshape(-1, Dm), k.reshape(-1, Dm), v.reshape(-1, Dm), B, H, hd, Tq, Tk, 1, rope, what, ctx_div=div)
        assert_close(got.reshape(B, Tq, Dm), want, what=what, **TOL_ATTN)


@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("hd", HDS)
def test_training_attention_forward_and_backward(lib, hd, Tq, Tk):
    """mdt_op_attn_fwd_train and mdt_op_attn_bwd: H = 1, 3, 8; causal on and off, RoPE on and off, p = 0 and p = 0.3 against float64
    with the restated mask, accumulate_kv 0 and 1, both layouts; gradient rows no sample owns keep the canary."""
    for H, B in heads_and_batches(hd, Tq, Tk):
        training_case(lib, hd, Tq, Tk, H, B)


def training_case(lib, hd, Tq, Tk, H, B):
    Dm = H * hd
    g = seeded("long train attention", hd, Tq, Tk, H)
    q, k, v = (torch.randn(B * T, Dm, generator=g) for T in (Tq, Tk, Tk))
    do, dkv0 = torch.randn(B * Tq, Dm, generator=g), torch.randn(B * Tk, 2 * Dm, generator=g)
    rc, rs = rope_tables()
    split = lambda t, T: t.view(B, T, H, hd).transpose(1, 2)
    for causal in (0, 1):
        for rope in (0, 1):
            for p in (0.0, 0.3):
                mask = torch.from_numpy(DM.scale(SEED, SITE, (B, H, Tq, Tk), p)) if p else 1.0
                q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
                att = _rot(split(q64, Tq), rope) @ _rot(split(k64, Tk), rope).transpose(-1, -2) / hd ** 0.5
                if causal:
                    att = att.masked_fill(~torch.ones(Tq, Tk, dtype=torch.bool).tril(), float("-inf"))
                y = ((att.softmax(-1) * mask) @ split(v64, Tk)).transpose(1, 2).reshape(B * Tq, Dm)
                y.backward(do.double())
                for layout in ("qkv", "kv"):
                    for acc in (0, 1):
                        what = (f"training attention hd {hd}, H {H}, B {B}, {Tq} x {Tk}, causal {causal}, rope {rope}, p {p}, {layout}, "
                                f"accumulate_kv {acc}")

                        def run(guarded):
                            L = Lay(guarded)
                            rows = B * max(Tq, Tk)
                            qp, kp, vp, ldq, ldkv = operands(L, layout, B, Tq, Tk, Dm, q, k, v)
                            if layout == "qkv":
                                start = canary(rows, 3 * Dm)
                                start[:B * Tq, :Dm] = NAN
                                start[:B * Tk, Dm:] = dkv0 if acc else NAN
                                grad = L.out("dqkv", rows, 3 * Dm, pad=4, fill=start)
                                dqp, dkp, dvp, ld_dq, ld_dkv = grad.at(0, 0), grad.at(0, Dm), grad.at(0, 2 * Dm), grad.ld, grad.ld
                            else:
                                dqo, grad = L.out("dq", B * Tq, Dm, pad=4), L.out("dkv", B * Tk, 2 * Dm, pad=4, fill=dkv0 if acc else None)
                                dqp, dkp, dvp, ld_dq, ld_dkv = dqo.ptr, grad.at(0, 0), grad.at(0, Dm), dqo.ld, grad.ld
                            out, dod = L.out("out", B * Tq, Dm, pad=4), L.inp("d_out", do, pad=4)
                            rcd, rsd = L.inp("rope_cos", rc), L.inp("rope_sin", rs)
                            kw = dict(B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=causal, p=p, site=SITE, seed=SEED, rope=rope, rope_cos=rcd.ptr,
                                      rope_sin=rsd.ptr)
                            a = lib.AttnTrainArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, out=out.ptr, ldo=out.ld, **kw)
                            lib.check(lib.load().mdt_op_attn_fwd_train(C.byref(a), stream()))
                            L.check(what + ": forward")
                            out.check(what + ": out", written=True)
                            gb = lib.AttnBwdArgs(q=qp, ldq=ldq, k=kp, v=vp, ldkv=ldkv, d_out=dod.ptr, ld_do=dod.ld, dq=dqp, ld_dq=ld_dq,
                                                 dk=dkp, dv=dvp, ld_dkv=ld_dkv, accumulate_kv=acc, **kw)
                            lib.check(lib.load().mdt_op_attn_bwd(C.byref(gb), stream()))
                            L.check(what + ": backward")
                            gh = grad.host()
                            if layout == "qkv":
                                skipped = torch.ones(rows, 3 * Dm, dtype=torch.bool)
                                skipped[:B * Tq, :Dm] = False
                                skipped[:B * Tk, Dm:] = False
                                assert same_bits(gh[skipped], canary(rows, 3 * Dm)[skipped]), f"{what}: gradient rows no sample owns were touched"
                                r = {"dq": gh[:B * Tq, :Dm], "dkv": gh[:B * Tk, Dm:]}
                            else:
                                r = {"dq": dqo.host(), "dkv": gh}
                            r["out"] = out.host()
                            for name, t in r.items():
                                assert not t.isnan().any(), f"{what}: NaN left in {name}"
                            return r

                        dense, got = both(run)
                        assert_close(got["out"], y.detach(), what=what + ": out", **(TOL_FWD if p else TOL_ATTN_FWD))
                        assert_close(got["dq"], q64.grad, what=what + ": dq", **G_TOL)
                        base = dkv0.double() if acc else 0
                        assert_close(got["dkv"][:, :Dm].double() - (base[:, :Dm] if acc else 0), k64.grad, what=what + ": dk", **G_TOL)
                        assert_close(got["dkv"][:, Dm:].double() - (base[:, Dm:] if acc else 0), v64.grad, what=what + ": dv", **G_TOL)
                        agree(got, dense, what)


@pytest.mark.parametrize("hd,Tq,Tk", [(48, 65, 65), (16, 17, 17), (48, 5, 65)])
def test_shapes_outside_the_envelope_are_refused_with_nothing_written(lib, hd, Tq, Tk):
    """More than 64 rows, or more than 16 at head dim 16: each of the three ops returns a non-zero status and leaves the canary of
    its outputs in place."""
    B, H = 2, 2
    Dm = H * hd
    g = seeded("long attention refused", hd, Tq, Tk)
    q, k, v, do = (torch.randn(B * T, Dm, generator=g) for T in (Tq, Tk, Tk, Tq))
    rc, rs = rope_tables()
    L = Lay(True)
    qd, kd, vd, dod = L.inp("q", q), L.inp("k", k), L.inp("v", v), L.inp("d_out", do)
    rcd, rsd = L.inp("rope_cos", rc), L.inp("rope_sin", rs)
    outs = {n: L.out(n, B * T, Dm, fill=canary(B * T, Dm)) for n, T in (("out", Tq), ("out_train", Tq), ("dq", Tq), ("dk", Tk), ("dv", Tk))}
    Lh = lib.load()
    a = lib.AttnArgs(q=qd.ptr, ldq=Dm, k=kd.ptr, v=vd.ptr, ldkv=Dm, out=outs["out"].ptr, ldo=Dm, B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=1, rope=0)
    assert Lh.mdt_op_attention(C.byref(a), stream()) != 0
    kw = dict(B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, causal=1, p=0.0, site=SITE, seed=SEED, rope=0, rope_cos=rcd.ptr, rope_sin=rsd.ptr)
    t = lib.AttnTrainArgs(q=qd.ptr, ldq=Dm, k=kd.ptr, v=vd.ptr, ldkv=Dm, out=outs["out_train"].ptr, ldo=Dm, **kw)
    assert Lh.mdt_op_attn_fwd_train(C.byref(t), stream()) != 0
    gb = lib.AttnBwdArgs(q=qd.ptr, ldq=Dm, k=kd.ptr, v=vd.ptr, ldkv=Dm, d_out=dod.ptr, ld_do=Dm, dq=outs["dq"].ptr, ld_dq=Dm, dk=outs["dk"].ptr,
                         dv=outs["dv"].ptr, ld_dkv=Dm, accumulate_kv=0, **kw)
    assert Lh.mdt_op_attn_bwd(C.byref(gb), stream()) != 0
    L.check(f"refused hd {hd}, {Tq} x {Tk}")
    for n, o in outs.items():
        assert o.keeps(), f"refused hd {hd}, {Tq} x {Tk}: {n} was written"
