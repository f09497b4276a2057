"""The kernel-level ops of include/mdt_hip_train.h held to their buffers (pytest -m gpu): the rule and the
assertions (a) - (e) of tests/test_gpu_ops_bounds.py, at the tolerances of tests/test_gpu_train_ops.py (G_TOL or the op's own),
tests/test_gpu_optim.py and tests/test_gpu_optim_amp.py."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests import dropout_masks as DM
from tests.guarded import GUARD_BITS, SENTINEL, Guarded, GuardedSet, bits, canary, same_bits
from tests.helpers import assert_close
from tests.test_gpu_ops import expected_pack, stream
from tests.test_gpu_ops_bounds import Lay, ptr, seeded
from tests.test_gpu_train_ops import G_TOL, _rot

pytestmark = pytest.mark.gpu

TOL_FWD = {}                                    # assert_close's defaults, as the forward checks of tests/test_gpu_train_ops.py
TOL_ACT_FWD = dict(rtol=1e-4, atol=2e-6)        # test_activation_forward_backward
TOL_ACT_BWD = dict(rtol=1e-4, atol=5e-6)
TOL_COLSUM = dict(rtol=1e-4, atol=1e-4)         # test_merge_gate_backward_and_colsum
TOL_ATTN_FWD = dict(rtol=1e-4, atol=1e-5)       # test_attention_train_forward_without_dropout
TOL_P = dict(rtol=2e-6, atol=2e-7)              # tests/test_gpu_optim.py: parameter, exp_avg, exp_avg_sq, ema
TOL_M = dict(rtol=2e-6, atol=5e-7)
TOL_V = dict(rtol=5e-6, atol=1e-9)
TOL_EMA = dict(rtol=1e-6, atol=1e-7)
SEED, SITE = 2 ** 40 + 12345, DM.site_id(9, DM.XRESID)


def tol_gate(rps):
    return dict(rtol=1e-3, atol=2e-5 * max(1.0, (rps / 10) ** 0.5))   # d_gate in tests/test_gpu_train_ops.py


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def both(run):
    """run(guarded) -> {name: host tensor}: the dense call, then the guarded one."""
    return run(False), run(True)


def agree(got, dense, what):
    for k in got:
        assert same_bits(got[k], dense[k]), f"{what}: {k} differs from the dense call's bits"


# ------------------------------------------------------------------------------------------------
# LayerNorm forward / backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mod", "mod, accumulate", "mod, d_mod accumulates", "no d_mod", "plain, no pb", "no stats"])
@pytest.mark.parametrize("B,rps", [(1, 1), (3, 10), (2, 77)])
@pytest.mark.parametrize("D", [30, 64, 512])
def test_layernorm_train_forward_and_backward(lib, D, B, rps, variant):
    """mdt_op_ln_fwd_train and mdt_op_ln_bwd: D = 30 takes the scalar kernels, (2, 77) runs the backward with row_chunks = 2 (no
    d_mod then); ld_dh = D + 4; mod rows [unused | shift | scale] with a padded stride, d_mod rows laid out alike -- their first
    D columns keep the canary --; pw / pb are exactly B * max(row_chunks, 1) rows; dx overwritten and accumulated into; d_mod
    given, accumulated into, or NULL; pb NULL; stats NULL in the forward."""
    M, chunks = B * rps, 2 if rps == 77 else 0
    mod = variant != "plain, no pb"
    acc = variant == "mod, accumulate"
    want_dmod = variant in ("mod", "mod, accumulate", "mod, d_mod accumulates") and chunks == 0
    acc_dmod = variant == "mod, d_mod accumulates"
    g = seeded("ln train", D, B, rps)
    x, w, b = torch.randn(M, D, generator=g), 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    modt, dh, dx0 = torch.randn(B, 3 * D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    dmod0 = torch.randn(B, 2 * D, generator=g)
    x64, w64, b64, m64 = (t.double().requires_grad_() for t in (x, w, b, modt))
    n = F.layer_norm(x64, (D,), w64, b64, 1e-5)
    rows = torch.arange(M) // rps
    h = m64[rows, D:2 * D] + n * m64[rows, 2 * D:] if mod else n
    h.backward(dh.double())
    what = f"LayerNorm D {D}, B {B}, rps {rps}, {variant}"

    def run(guarded):
        L, r = Lay(guarded), {}
        xd, wd, bd = L.inp("x", x), L.inp("w", w), L.inp("b", b)
        md = L.inp("mod", modt, pad=4) if mod else None
        out = L.out("out", M, D)
        stats = L.out("stats", M, 2) if variant != "no stats" else None
        a = lib.LnTrainArgs(x=xd.ptr, w=wd.ptr, b=bd.ptr, mod=ptr(md), mod_stride=md.ld if mod else 0, shift_off=D if mod else -1,
                            scale_off=2 * D if mod else -1, rows_per_sample=rps, out=out.ptr, stats=ptr(stats), M=M, D=D)
        lib.check(lib.load().mdt_op_ln_fwd_train(C.byref(a), stream()))
        L.check(what + ": forward")
        out.check(what + ": out", written=True)
        r["out"] = out.host()
        if stats is None:
            return r
        stats.check(what + ": stats", written=True)
        dhd = L.inp("dh", dh, pad=4)
        dx = L.out("dx", M, D, fill=dx0 if acc else None)
        nrow = B * max(chunks, 1)
        pw, pb = L.out("pw", nrow, D), (L.out("pb", nrow, D) if variant != "plain, no pb" else None)
        dm = None
        if want_dmod:
            start = canary(B, 3 * D)
            if acc_dmod:
                start[:, D:] = dmod0
            dm = L.out("d_mod", B, 3 * D, pad=4, fill=start)
        gb = lib.LnBwdArgs(x=xd.ptr, stats=stats.ptr, w=wd.ptr, b=bd.ptr, mod=ptr(md), mod_stride=md.ld if mod else 0,
                           shift_off=D if mod else -1, scale_off=2 * D if mod else -1, dh=dhd.ptr, ld_dh=dhd.ld, dx=dx.ptr,
                           accumulate=int(acc), d_mod=ptr(dm), d_mod_stride=dm.ld if dm else 0, pw=pw.ptr, pb=ptr(pb), B=B,
                           rows_per_sample=rps, D=D, row_chunks=chunks, accumulate_dmod=int(acc_dmod))
        lib.check(lib.load().mdt_op_ln_bwd(C.byref(gb), stream()))
        L.check(what + ": backward")
        for name, o in (("dx", dx), ("pw", pw), ("pb", pb)):
            if o is not None:
                o.check(f"{what}: {name}", written=True)
                r[name] = o.host()
        if dm is not None:
            r["d_mod"] = dm.host()
        return r

    dense, got = both(run)
    assert_close(got["out"], h.detach(), what=what + ": forward", **TOL_FWD)
    if "dx" in got:
        assert_close(got["dx"].double() - (dx0.double() if acc else 0), x64.grad, what=what + ": dx", **G_TOL)
        assert_close(got["pw"].double().sum(0), w64.grad, what=what + ": dw", **G_TOL)
        if "pb" in got:
            assert_close(got["pb"].double().sum(0), b64.grad, what=what + ": db", **G_TOL)
        if "d_mod" in got:
            assert same_bits(got["d_mod"][:, :D], canary(B, 3 * D)[:, :D]), f"{what}: the unused columns of d_mod were touched"
            assert_close(got["d_mod"][:, D:].double() - (dmod0.double() if acc_dmod else 0), m64.grad[:, D:], what=what + ": d_mod", **G_TOL)
    agree(got, dense, what)


# ------------------------------------------------------------------------------------------------
# training attention, forward and backward
# ------------------------------------------------------------------------------------------------
def rope_tables():
    from oracle.mdt_oracle import rotary_tables
    cos, sin = rotary_tables(16, torch.float64)
    return cos[:, ::2].float().contiguous(), sin[:, ::2].float().contiguous()


@pytest.mark.parametrize("Tq,Tk", [(1, 1), (10, 4), (16, 16), (5, 11)])
@pytest.mark.parametrize("hd", [16, 32, 48, 64])
def test_training_attention_forward_and_backward(lib, hd, Tq, Tk):
    """mdt_op_attn_fwd_train and mdt_op_attn_bwd at B = 3, H = 4: causal on and off, RoPE where hd >= 32 (the scalar kernels; the
    MFMA ones otherwise), p = 0 and p = 0.1 against float64 with the restated mask, accumulate_kv 0 and 1, and both layouts -- q | k |
    v and dq | dk | dv as column blocks of one row of stride 3 H hd + 4, or q / dq rows beside separate K | V rows of stride
    2 H hd + 4."""
    B, H = 3, 4
    Dm = H * hd
    g = seeded("train attention", hd, Tq, Tk)
    q, k, v = (torch.randn(B * T, Dm, generator=g) for T in (Tq, Tk, Tk))
    do, dkv0 = torch.randn(B * Tq, Dm, generator=g), torch.randn(B * Tk, 2 * Dm, generator=g)
    rc, rs = rope_tables()
    split = lambda t, T: t.view(B, T, H, hd).transpose(1, 2)
    for causal in (0, 1):
        for rope in ((0, 1) if hd >= 32 else (0,)):
            for p in (0.0, 0.1):
                mask = torch.from_numpy(DM.scale(SEED, SITE, (B, H, Tq, Tk), p)) if p else 1.0
                q64, k64, v64 = (t.double().requires_grad_() for t in (q, k, v))
                att = _rot(split(q64, Tq), rope) @ _rot(split(k64, Tk), rope).transpose(-1, -2) / hd ** 0.5
                if causal:
                    att = att.masked_fill(~torch.ones(Tq, Tk, dtype=torch.bool).tril(), float("-inf"))
                y = ((att.softmax(-1) * mask) @ split(v64, Tk)).transpose(1, 2).reshape(B * Tq, Dm)
                y.backward(do.double())
                for layout in ("qkv", "kv"):
                    for acc in (0, 1):
                        what = f"training attention hd {hd}, {Tq} x {Tk}, causal {causal}, rope {rope}, p {p}, {layout}, accumulate_kv {acc}"

                        def run(guarded):
                            L = Lay(guarded)
                            rows = B * max(Tq, Tk)
                            nan = float("nan")
                            if layout == "qkv":
                                t = torch.full((rows, 3 * Dm), nan)
                                t[:B * Tq, :Dm], t[:B * Tk, Dm:2 * Dm], t[:B * Tk, 2 * Dm:] = q, k, v
                                src = L.inp("qkv", t, pad=4)
                                qp, kp, vp, ldq, ldkv = src.at(0, 0), src.at(0, Dm), src.at(0, 2 * Dm), src.ld, src.ld
                                start = canary(rows, 3 * Dm)
                                start[:B * Tq, :Dm] = nan
                                start[:B * Tk, Dm:] = dkv0 if acc else nan
                                grad = L.out("dqkv", rows, 3 * Dm, pad=4, fill=start)
                                dqp, dkp, dvp, ld_dq, ld_dkv = grad.at(0, 0), grad.at(0, Dm), grad.at(0, 2 * Dm), grad.ld, grad.ld
                            else:
                                qs, kvs = L.inp("q", q, pad=4), L.inp("kv", torch.cat([k, v], 1), pad=4)
                                qp, kp, vp, ldq, ldkv = qs.ptr, kvs.at(0, 0), kvs.at(0, Dm), qs.ld, kvs.ld
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


# ------------------------------------------------------------------------------------------------
# activations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,fn", [(1, F.gelu), (2, F.mish), (3, F.silu)])
@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 1025])
def test_activation_forward_and_backward(lib, n, act, fn):
    """mdt_op_act_fwd / mdt_op_act_bwd: one element, a count below / at one float4, one below / at one workgroup, one element into
    a fifth."""
    g = seeded("act", n)
    u, dy = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
    u64 = u.double().requires_grad_()
    y = fn(u64)
    y.backward(dy.double())
    what = f"activation {act}, n {n}"

    def run(guarded):
        L = Lay(guarded)
        ud, dyd, out, du = L.inp("u", u), L.inp("dy", dy), L.out("out", 1, n), L.out("du", 1, n)
        lib.check(lib.load().mdt_op_act_fwd(ud.ptr, out.ptr, n, act, stream()))
        lib.check(lib.load().mdt_op_act_bwd(ud.ptr, dyd.ptr, du.ptr, n, act, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        du.check(what + ": du", written=True)
        return {"out": out.host().reshape(-1), "du": du.host().reshape(-1)}

    dense, got = both(run)
    assert_close(got["out"], y.detach(), what=what, **TOL_ACT_FWD)
    assert_close(got["du"], u64.grad, what=what + ": gradient", **TOL_ACT_BWD)
    agree(got, dense, what)


# ------------------------------------------------------------------------------------------------
# branch merge and the fused pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("B,rps,D", [(1, 1, 30), (3, 5, 64), (2, 19, 512)])
def test_merge_and_the_fused_pairs(lib, B, rps, D, gated, p):
    """mdt_op_merge_fwd / mdt_op_merge_bwd and the fused pairs mdt_op_merge_ln_fwd / mdt_op_ln_bwd_merge (D = 30: the scalar
    kernels and the two-launch route inside the pairs): gate and dgate at column D of a wider row of padded stride whose other
    columns -- of the d_mod row -- keep the canary; gate NULL; dropout by the restated mask."""
    M = B * rps
    g = seeded("merge", B, rps, D)
    x, a, mod = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(B, 3 * D, generator=g)
    w, b = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    dx, dh, dx0 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    mask = torch.from_numpy(DM.scale(SEED, SITE, (M, D), p)) if p else 1.0
    a64, g64 = a.double().requires_grad_(), mod[:, D:2 * D].double().requires_grad_()
    gate_rows = g64.repeat_interleave(rps, 0) if gated else 1.0
    x1 = x.double() + gate_rows * (a64 * mask)
    x1.retain_grad()
    h = F.layer_norm(x1, (D,), w.double(), b.double(), 1e-5)
    da_ref = (gate_rows * mask * dx.double()).detach()                             # the two ops on their own, upstream gradient dx
    dg_ref = (dx.double() * a.double() * mask).view(B, rps, D).sum(1)
    ((h * dh.double()).sum() + (x1 * dx0.double()).sum()).backward()
    what = f"merge B {B}, rps {rps}, D {D}, gate {gated}, p {p}"

    def run(guarded):
        L, r = Lay(guarded), {}
        Lh = lib.load()
        xd, ad, wd, bd = L.inp("x", x), L.inp("a", a), L.inp("w", w), L.inp("b", b)
        md = L.inp("mod", mod, pad=4) if gated else None

        def margs(xin, out, dgate=None):
            return lib.MergeArgs(x=xin.ptr, a=ad.ptr, gate=md.at(0, D) if gated else None, gate_stride=md.ld if gated else 0, out=out.ptr,
                                 dgate=dgate.at(0, D) if dgate is not None else None, dgate_stride=dgate.ld if dgate is not None else 0,
                                 B=B, rows_per_sample=rps, D=D, p=p, site=SITE, seed=SEED)

        def dgate_row(name):
            return L.out(name, B, 3 * D, pad=4, fill=canary(B, 3 * D)) if gated else None

        def keep_dgate(o, name):
            if o is not None:
                hst = o.host()
                assert same_bits(hst[:, :D], canary(B, 3 * D)[:, :D]) and same_bits(hst[:, 2 * D:], canary(B, 3 * D)[:, 2 * D:]), \
                    f"{what}: {name}: the other columns of the d_mod row were touched"
                assert not hst[:, D:2 * D].isnan().any(), f"{what}: NaN left in {name}"
                r[name] = hst[:, D:2 * D]

        # the two ops on their own
        out = L.out("out", M, D)
        lib.check(Lh.mdt_op_merge_fwd(C.byref(margs(xd, out)), stream()))
        dxd, da, dg = L.inp("dx", dx), L.out("da", M, D), dgate_row("dgate")
        lib.check(Lh.mdt_op_merge_bwd(C.byref(margs(dxd, da, dg)), stream()))
        L.check(what + ": merge_fwd / merge_bwd")
        out.check(what + ": out", written=True)
        da.check(what + ": d_a", written=True)
        r["out"], r["da"] = out.host(), da.host()
        keep_dgate(dg, "dgate")
        # the fused pairs
        x1d, hd_, st = L.out("x1", M, D), L.out("h", M, D), L.out("stats", M, 2)
        lf = lib.LnTrainArgs(x=xd.ptr, w=wd.ptr, b=bd.ptr, mod=None, mod_stride=0, shift_off=-1, scale_off=-1, rows_per_sample=rps,
                             out=hd_.ptr, stats=st.ptr, M=M, D=D)
        lib.check(Lh.mdt_op_merge_ln_fwd(C.byref(margs(xd, x1d)), C.byref(lf), stream()))
        L.check(what + ": merge_ln_fwd")
        for name, o in (("x1", x1d), ("h", hd_), ("stats", st)):
            o.check(f"{what}: {name}", written=True)
        r["x1"], r["h"] = x1d.host(), hd_.host()
        dhd, dxa = L.inp("dh", dh, pad=4), L.out("dx1", M, D, fill=dx0)
        da2, dg2, pw, pb = L.out("da2", M, D), dgate_row("dgate2"), L.out("pw", B, D), L.out("pb", B, D)
        gb = lib.LnBwdArgs(x=x1d.ptr, stats=st.ptr, w=wd.ptr, b=bd.ptr, mod=None, mod_stride=0, shift_off=-1, scale_off=-1, dh=dhd.ptr,
                           ld_dh=dhd.ld, dx=dxa.ptr, accumulate=1, d_mod=None, d_mod_stride=0, pw=pw.ptr, pb=pb.ptr, B=B,
                           rows_per_sample=rps, D=D, row_chunks=0)
        lib.check(Lh.mdt_op_ln_bwd_merge(C.byref(gb), C.byref(margs(dxa, da2, dg2)), stream()))
        L.check(what + ": ln_bwd_merge")
        for name, o in (("dx1", dxa), ("da2", da2), ("pw", pw), ("pb", pb)):
            o.check(f"{what}: {name}", written=True)
            r[name] = o.host()
        keep_dgate(dg2, "dgate2")
        return r

    dense, got = both(run)
    assert_close(got["out"], x1.detach(), what=what + ": x + g drop(a)", **TOL_FWD)
    assert_close(got["da"], da_ref, what=what + ": d_a", **G_TOL)
    assert_close(got["x1"], x1.detach(), what=what + ": merged rows", **TOL_FWD)
    assert_close(got["h"], h.detach(), what=what + ": LayerNorm of the merged rows", **TOL_FWD)
    assert_close(got["dx1"], x1.grad, what=what + ": d_x1", **G_TOL)
    assert_close(got["da2"], a64.grad, what=what + ": d_a of the fused pair", **G_TOL)
    if gated:
        assert_close(got["dgate"], dg_ref, what=what + ": d_gate", **tol_gate(rps))
        assert_close(got["dgate2"], g64.grad, what=what + ": d_gate of the fused pair", **tol_gate(rps))
    agree(got, dense, what)


# ------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,N,pad", [(1, 1, 0), (37, 7, 3), (512, 16, 4), (513, 100, 1), (5, 16384, 0), (13, 16384, 3)])
def test_colsum(lib, M, N, pad, accumulate):
    """mdt_op_colsum: one element; a ragged column group; the sliced two-stage reduction from 512 rows on, with rows that divide
    into its 64 slices and one more; the 16-byte kernel at 16384 columns, and the odd stride that keeps the general kernel there.
    The stride is the call's own (ldx = N + pad), so the dense twin has it too."""
    g = seeded("colsum", M, N, pad)
    X, out0 = torch.randn(M, N, generator=g), torch.randn(N, generator=g)
    what = f"colsum {M} x {N}, ldx {N + pad}, accumulate {accumulate}"

    def run(guarded):
        L = Lay(guarded)
        Xd, out = L.inp("X", X, pad=pad, fixed=True), L.out("out", 1, N, fill=out0 if accumulate else None)
        lib.check(lib.load().mdt_op_colsum(Xd.ptr, Xd.ld, M, N, out.ptr, accumulate, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        return {"out": out.host().reshape(-1)}

    dense, got = both(run)
    assert_close(got["out"].double() - (out0.double() if accumulate else 0), X.double().sum(0), what=what, **TOL_COLSUM)
    agree(got, dense, what)


# ------------------------------------------------------------------------------------------------
# the training path's packers
# ------------------------------------------------------------------------------------------------
def test_pack_weight_t_at_a_k_offset_from_padded_rows(lib):
    """mdt_op_pack_weight_t: a (48, 32; ld 33) source into the image of W^T (N' = 32, K' = 80) at k offset 16: the k16 blocks
    outside [16, 64) keep the canary."""
    rows, cols, k_off, k_total = 48, 32, 16, 80
    W = torch.randn(rows, cols, generator=seeded("pack_t"))
    L = GuardedSet()
    src = L.inp("w", W, ld=cols + 1)
    img = L.out("image", cols * k_total // 256, 256, fill=canary(cols * k_total // 256, 256))
    lib.check(lib.load().mdt_op_pack_weight_t(src.ptr, rows, cols, src.ld, img.ptr, k_off, k_total, stream()))
    torch.cuda.synchronize()
    L.check("pack_weight_t")
    full = torch.zeros(cols, k_total)
    full[:, k_off:k_off + rows] = W.T
    want = torch.from_numpy(expected_pack(full)).reshape(cols // 16, k_total // 16, 256)
    got, keep = img.host().reshape(cols // 16, k_total // 16, 256), canary(cols * k_total).reshape(cols // 16, k_total // 16, 256)
    lo, hi = k_off // 16, (k_off + rows) // 16
    assert same_bits(got[:, lo:hi], want[:, lo:hi]), "pack_weight_t: image differs from the host packer's"
    assert same_bits(got[:, :lo], keep[:, :lo]) and same_bits(got[:, hi:], keep[:, hi:]), "pack_weight_t: a block outside the k range was touched"


def test_pack_many_into_images_laid_back_to_back(lib):
    """mdt_op_pack_many: three weights, the forward images back to back in ONE Guarded with guard-pattern gaps between them, the
    transposed images likewise with wt[1] NULL (its place keeps the guard pattern)."""
    shapes = [(16, 32), (48, 96), (32, 16)]
    g = seeded("pack_many")
    Ws = [torch.randn(N, K, generator=g) for N, K in shapes]
    gap = 64
    offs, total = [], 0
    for N, K in shapes:
        offs.append(total)
        total += N * K + gap
    total -= gap
    L = GuardedSet()
    srcs = [L.inp(f"w{i}", W) for i, W in enumerate(Ws)]
    blank = torch.empty(total)
    blank.view(torch.int32).fill_(GUARD_BITS)
    for (N, K), o in zip(shapes, offs):
        blank[o:o + N * K] = float("nan")
    wp, wt = L.out("wp", 1, total, fill=blank), L.out("wt", 1, total, fill=blank)
    n = len(shapes)
    arr = lambda vals: (C.c_void_p * n)(*vals)
    Ns, Ks = (C.c_int32 * n)(*[s[0] for s in shapes]), (C.c_int32 * n)(*[s[1] for s in shapes])
    lib.check(lib.load().mdt_op_pack_many(n, arr([s.ptr for s in srcs]), Ns, Ks, arr([wp.ptr + 4 * o for o in offs]),
                                          arr([None if i == 1 else wt.ptr + 4 * o for i, o in enumerate(offs)]), stream()))
    torch.cuda.synchronize()
    L.check("pack_many")
    want_p, want_t = blank.clone(), blank.clone()
    for i, ((N, K), o, W) in enumerate(zip(shapes, offs, Ws)):
        want_p[o:o + N * K] = torch.from_numpy(expected_pack(W))
        if i != 1:
            want_t[o:o + N * K] = torch.from_numpy(expected_pack(W.T.contiguous()))
    assert same_bits(wp.host().reshape(-1), want_p), "pack_many: a forward image differs, or a gap between two images was written"
    assert same_bits(wt.host().reshape(-1), want_t), "pack_many: a transposed image differs, or the place of the NULL one was written"


# ------------------------------------------------------------------------------------------------
# the multi-tensor optimizer ops
# ------------------------------------------------------------------------------------------------
NUMEL = [1, 3, 4095, 4096, 4097, 8195]


class Flat:
    """One member (p, g, m, v or ema) of every tensor in ONE flat Guarded, one separator float behind each tensor: most tensors
    are 4-byte aligned only, and each ends inside or just behind a 4096-element chunk.  The separators are the guard pattern, or
    -- finite=True -- a finite sentinel: an update in place of a guard NaN (p *= ..., m = b1 m + ...) hands the NaN on with its
    payload, so only a finite separator shows a read-modify-write of the float behind a tensor."""

    def __init__(self, values, finite=False):
        self.offs, total = [], 0
        for t in values:
            self.offs.append(total)
            total += t.numel() + 1
        flat = torch.empty(total)
        flat.view(torch.int32).fill_(GUARD_BITS)
        if finite:
            flat.fill_(SENTINEL)
        self.sep = torch.ones(total, dtype=torch.bool)
        for o, t in zip(self.offs, values):
            flat[o:o + t.numel()] = t
            self.sep[o:o + t.numel()] = False
        self.g = Guarded(1, total, fill=flat)
        self.start = bits(self.g.region).reshape(-1)

    def ptr(self, i):
        return self.g.ptr + 4 * self.offs[i]

    def tensors(self):
        h = self.g.host().reshape(-1)
        return [h[o:o + n] for o, n in zip(self.offs, NUMEL)]

    def check(self, what, unchanged=False):
        self.g.check(what)
        now = bits(self.g.region).reshape(-1)
        bad = (now != self.start) & self.sep
        assert not bool(bad.any()), f"{what}: the float behind a tensor was written (offset {int(bad.nonzero()[0]) if bad.any() else -1})"
        if unchanged:
            assert torch.equal(now, self.start), f"{what}: changed"


def opt_members(seed):
    g = seeded("optimizer", seed)
    mk = lambda scale=1.0: [torch.randn(n, generator=g) * scale for n in NUMEL]
    return dict(p=mk(), g=mk(), m=mk(0.1), v=[t.abs() * 0.01 for t in mk()], ema=mk())


def opt_table(lib, F_):
    tab = (lib.OptTensor * len(NUMEL))()
    for i, n in enumerate(NUMEL):
        tab[i] = lib.OptTensor(**{k: (F_[k].ptr(i) if k in F_ else None) for k in ("p", "g", "m", "v", "ema")}, numel=n)
    return tab


def adamw_ref(mem, lr, b1, b2, eps, wd, t):
    out = {"p": [], "m": [], "v": []}
    for p, g, m, v in zip(*(mem[k] for k in ("p", "g", "m", "v"))):
        p, g, m, v = (x.double() for x in (p, g, m, v))
        p = p * (1 - lr * wd)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * (m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))
        for k, x in (("p", p), ("m", m), ("v", v)):
            out[k].append(x)
    return out


HYPER = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1)


def check_adamw(F_, mem, t, what):
    ref = adamw_ref(mem, t=t, **HYPER)
    for k, tol in (("p", TOL_P), ("m", TOL_M), ("v", TOL_V)):
        F_[k].check(f"{what}: {k}")
        for i, (got, want) in enumerate(zip(F_[k].tensors(), ref[k])):
            assert_close(got, want, what=f"{what}: {k} of tensor {i} ({NUMEL[i]} elements)", **tol)
    F_["g"].check(f"{what}: g", unchanged=True)


@pytest.mark.parametrize("finite", [False, True])
def test_multi_adamw_on_tensors_one_float_apart(lib, finite):
    """mdt_op_multi_adamw (step 3) on p, g, m, v laid out as Flat: whole 16-byte aligned chunks take the float4 path, everything else
    the scalar tail, whose last element sits against the separator."""
    mem = opt_members(1)
    F_ = {k: Flat(mem[k], finite) for k in ("p", "g", "m", "v")}
    h = HYPER
    lib.check(lib.load().mdt_op_multi_adamw(opt_table(lib, F_), len(NUMEL), h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], 3, stream()))
    torch.cuda.synchronize()
    check_adamw(F_, mem, 3, "multi_adamw")


@pytest.mark.parametrize("finite", [False, True])
@pytest.mark.parametrize("found_inf", [0.0, 1.0])
def test_multi_adamw_dev_steps_or_leaves_every_bit(lib, found_inf, finite):
    """mdt_op_multi_adamw_dev with step and found_inf as guarded device scalars: the update of step + 1, or -- found_inf set --
    every bit of p, m, v and step left in place."""
    mem = opt_members(2)
    F_ = {k: Flat(mem[k], finite) for k in ("p", "g", "m", "v")}
    S = GuardedSet()
    step, inf = S.out("step", 1, 1, fill=2.0), S.inp("found_inf", torch.tensor([found_inf]))
    h = HYPER
    lib.check(lib.load().mdt_op_multi_adamw_dev(opt_table(lib, F_), len(NUMEL), h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step.ptr,
                                                None, inf.ptr, None, 0.0, None, stream()))
    torch.cuda.synchronize()
    S.check("multi_adamw_dev")
    if found_inf:
        for k in F_:
            F_[k].check(f"skipped step: {k}", unchanged=True)
        assert step.keeps(), "skipped step: the step count changed"
    else:
        assert float(step.host()) == 3.0
        check_adamw(F_, mem, 3, "multi_adamw_dev")


@pytest.mark.parametrize("finite", [False, True])
def test_multi_ema_on_tensors_one_float_apart(lib, finite):
    """mdt_op_multi_ema: ema = decay ema + (1 - decay) p on the same layout; p keeps its bits."""
    mem = opt_members(3)
    F_ = {k: Flat(mem[k], finite) for k in ("p", "ema")}
    lib.check(lib.load().mdt_op_multi_ema(opt_table(lib, F_), len(NUMEL), 0.999, stream()))
    torch.cuda.synchronize()
    F_["p"].check("multi_ema: p", unchanged=True)
    F_["ema"].check("multi_ema: ema")
    for i, (got, e, p) in enumerate(zip(F_["ema"].tensors(), mem["ema"], mem["p"])):
        assert_close(got, 0.999 * e.double() + (1 - 0.999) * p.double(), what=f"ema of tensor {i}", **TOL_EMA)


@pytest.mark.parametrize("which", [0, 1])
def test_multi_sumsq_with_exactly_its_scratch(lib, which):
    """mdt_op_multi_sumsq over the g or the p members: partials is a Guarded of exactly mdt_op_multi_sumsq_scratch floats; the
    norm within 1e-6 relative of float64 (tests/test_gpu_optim_amp.py), no non-finite element counted -- the separators are NaN."""
    mem = opt_members(4)
    key = "p" if which else "g"
    F_ = {key: Flat(mem[key])}
    tab = opt_table(lib, F_)
    Lh = lib.load()
    need = Lh.mdt_op_multi_sumsq_scratch(tab, len(NUMEL))
    assert need == 2 * sum((n + 4095) // 4096 for n in NUMEL)
    S = GuardedSet()
    out, partials = S.out("out", 1, 2), S.out("partials", 1, need)
    lib.check(Lh.mdt_op_multi_sumsq(tab, len(NUMEL), which, out.ptr, partials.ptr, need, stream()))
    torch.cuda.synchronize()
    S.check("multi_sumsq")
    out.check("multi_sumsq: out", written=True)
    partials.check("multi_sumsq: partials", written=True)
    F_[key].check(f"multi_sumsq: {key}", unchanged=True)
    got, count = (float(v) for v in out.host().reshape(-1))
    want = float(torch.linalg.vector_norm(torch.cat([t.double() for t in mem[key]])))
    assert abs(math.sqrt(got) - want) <= 1e-6 * want and count == 0.0
