"""mdt_op_head at action widths of 17 .. 64 (the tiled head of mdt_head_wide.hip; pytest -m gpu) against a float64 torch
evaluation of the same formula, every operand between the guard bands of tests/guarded.py (the op's rows are dense: it has no
stride), at the tolerance tests/test_gpu_ops_bounds.py holds the narrow head to (its TOL_HEAD).

Shapes: A one column into the second 16-column tile, aligned, one into the third, one short of and at the top of the range; D
below / at / above one float4 per lane and at the limit, 112 and 144 no multiple of 128; M one row, one short of / at / one past
a 16-row tile, two tiles with a ragged second one, three tiles (several workgroups).  Variants: with and without the LayerNorm
bias, denoiser mode (no next embedding) and DDIM mode with and without the next embedding, the last DDIM step (sigma_next = 0)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.guarded import NAN, same_bits
from tests.helpers import assert_close
from tests.test_gpu_ops import stream
from tests.test_gpu_ops_bounds import TOL_HEAD, Lay, seeded

pytestmark = pytest.mark.gpu

T, SD = 3, 0.5   # rows per sample, sigma_data
# (mode, LayerNorm bias, next embedding, sigma_next)
VARIANTS = [("denoised", True, False, None), ("ddim", False, True, 2.5), ("ddim", True, True, 0.0), ("ddim", False, False, 2.5)]


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def operands(A, D, M, key):
    g = seeded("wide head", A, D, M, key)
    nb = (M + T - 1) // T
    return dict(y=torch.randn(M, D, generator=g) * 2, ln_w=torch.randn(D, generator=g) * 0.1 + 1, ln_b=torch.randn(D, generator=g) * 0.1,
                Wp=torch.randn(A, D, generator=g) / 20, bp=torch.randn(A, generator=g), Wa=torch.randn(A, D, generator=g),
                ba=torch.randn(D, generator=g), x=torch.randn(M, A, generator=g) * 10, sigma=torch.rand(nb, generator=g) * 20 + 0.05)


def expected(o, mode, ln_bias, embed, sig_next, step):
    """The head's formula in `o`'s dtype (float64: the yardstick; float32: the figure a tolerance would be derived from)."""
    dt = o["y"].dtype
    M, D = o["y"].shape
    h = F.layer_norm(o["y"], (D,), o["ln_w"], o["ln_b"] if ln_bias else None, 1e-5)
    Fv = h @ o["Wp"].T + o["bp"]
    s = o["sigma"][torch.arange(M) // T][:, None]
    den = Fv * (s * SD / (s ** 2 + SD ** 2).sqrt()) + o["x"] * (SD ** 2 / (s ** 2 + SD ** 2))
    want = {"out": den if mode == "denoised" else step[0].to(dt) * o["x"] + step[1].to(dt) * den}
    if embed:
        want["y_next"] = (want["out"] / math.sqrt(sig_next ** 2 + SD ** 2)) @ o["Wa"] + o["ba"]
    return want


def call(lib, L, o, A, D, M, mode, ln_bias, embed, step):
    """One mdt_op_head call on the operands `o` laid out by L (rows M / A of `o` may hold more: the call names M and A)."""
    d = {k: L.inp(k, v) for k, v in o.items() if k != "sigma"}
    d["step"] = L.inp("step", step)
    sg = L.inp("sigma", o["sigma"].reshape(-1, 1))
    out = L.out("out", M, A)
    yn = L.out("y_next", M, D) if embed else None
    a = lib.HeadArgs()
    a.y, a.ln_w, a.ln_b, a.Wp, a.bp, a.x = d["y"].ptr, d["ln_w"].ptr, d["ln_b"].ptr if ln_bias else None, d["Wp"].ptr, d["bp"].ptr, d["x"].ptr
    a.sigma, a.sigma_stride, a.out = sg.ptr, 1, out.ptr
    a.M, a.D, a.A, a.rows_per_sample, a.mode, a.sigma_data, a.step = M, D, A, T, lib.HEAD[mode], SD, d["step"].ptr
    if embed:
        a.y_next, a.Wa, a.ba = yn.ptr, d["Wa"].ptr, d["ba"].ptr
    lib.check(lib.load().mdt_op_head(C.byref(a), stream()))
    return out, yn


def run(lib, guarded, o, A, D, M, mode, ln_bias, embed, sig_next, what):
    step = torch.tensor([0.3, 0.7, 2.5 if sig_next is None else sig_next])
    L = Lay(guarded)
    out, yn = call(lib, L, o, A, D, M, mode, ln_bias, embed, step)
    L.check(what)   # every input intact and unchanged, every output's bands intact
    out.check(what + ": out", written=True)
    got = {"out": out.host()}
    if embed:
        yn.check(what + ": y_next", written=True)
        got["y_next"] = yn.host()
    return got, step


@pytest.mark.parametrize("M", [1, 15, 16, 17, 20, 40])
@pytest.mark.parametrize("D", [112, 144, 384, 512])
@pytest.mark.parametrize("A", [17, 32, 33, 63, 64])
def test_wide_action_head(lib, A, D, M):
    """Every variant against float64 at TOL_HEAD; the guarded call leaves its bands intact and gives the dense call's bits."""
    for vi, (mode, ln_bias, embed, sig_next) in enumerate(VARIANTS):
        what = f"wide head {mode}, A {A}, D {D}, M {M}, ln bias {ln_bias}, embed {embed}, sigma_next {sig_next}"
        o = operands(A, D, M, vi)
        dense, _ = run(lib, False, o, A, D, M, mode, ln_bias, embed, sig_next, what + " (dense)")
        got, step = run(lib, True, o, A, D, M, mode, ln_bias, embed, sig_next, what)
        want = expected({k: v.double() for k, v in o.items()}, mode, ln_bias, embed, sig_next or 0.0, step.double())
        assert set(got) == set(want)
        for k, w in want.items():
            assert_close(got[k], w, what=f"{what}: {k}", **TOL_HEAD)
            assert same_bits(got[k], dense[k]), f"{what}: {k} differs from the dense call's bits"


def test_padded_rows_and_columns_feed_nothing(lib):
    """The narrowest case (A = 17, D = 112, M = 1) twice, on operands one row longer than the call names: row M of y and x (the
    tile's first padded row) and row A of action_pred / action_emb, element A of the bias (the second column tile's first padded
    column) hold finite values the first time and NaN the second.  The outputs are bit-identical."""
    A, D, M = 17, 112, 1
    o = operands(A, D, M, "twin")
    g = seeded("wide head twin rows")
    extra = dict(y=torch.randn(1, D, generator=g), x=torch.randn(1, A, generator=g), Wp=torch.randn(1, D, generator=g),
                 Wa=torch.randn(1, D, generator=g), bp=torch.randn(1, generator=g))
    step = torch.tensor([0.3, 0.7, 2.5])
    res = []
    for poison in (False, True):
        p = dict(o)
        for k, v in extra.items():
            p[k] = torch.cat([o[k], torch.full_like(v, NAN) if poison else v])
        out, yn = call(lib, Lay(False), p, A, D, M, "ddim", True, True, step)
        torch.cuda.synchronize()
        res.append((out.host(), yn.host()))
    assert not res[0][0].isnan().any() and not res[0][1].isnan().any()
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    want = expected({k: v.double() for k, v in o.items()}, "ddim", True, True, 2.5, step.double())
    assert_close(res[0][0], want["out"], what="twin: out", **TOL_HEAD)
    assert_close(res[0][1], want["y_next"], what="twin: y_next", **TOL_HEAD)
