"""The four element-wise kernels of the steered samplers, kernel by kernel, against float64 (pytest -m gpu): mdt_op_steer_seed,
mdt_op_steer_step, mdt_op_steer_first and mdt_op_steer_plan of include/mdt_hip_debug.h -- each the launch its entry point makes --
on the operands of tests/guarded.py: every buffer between guard bands, outputs pre-filled with the canary, inputs held to their
bits.

References, cases and bounds are those of tests/steer_ops_cases.py: the numpy restatement of each kernel in float64, and per output
(roundings on its path) 2^-24 sum|terms|, the counts stated there.  tests/test_cpu_steer_ops_reference.py shows on the host that a
correctly rounded fp32 execution is inside every bound and each planted defect outside.

Sizes (N elements, R sigma rows; a trip of the grid-stride loop is 1024 x 256 = 262144 indices): one partly filled block; a ragged
last block; N + R exactly one trip; the one index of the second trip a sigma row; second-trip elements and sigma rows; one
64 x 64 chunk; and k_steer_step over no elements, as fill_sigma calls it.

Measured on the MI355X: see DESIGN.md 4.3i."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import steer_ops_cases as S
from tests.guarded import Guarded, bits, canary
from tests.test_gpu_ops import stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def rows():
    return S.plan_rows()


class Ops:
    """The operands of one call: inputs (must keep their bits) and outputs (in-place operands among them), every one a Guarded of
    dense rows of ``cols`` columns."""

    def __init__(self, cols):
        self.cols, self.inputs, self.outputs = cols, {}, {}

    def _lay(self, n):
        cols = self.cols if n % self.cols == 0 else 1
        return n // cols, cols

    def inp(self, name, a):
        """An input from a numpy array of any shape (flattened)."""
        r, c = self._lay(a.size)
        self.inputs[name] = Guarded(r, c, fill=torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(r, c))
        return self.inputs[name]

    def out(self, name, n, fill=None):
        """An output of n floats: the canary, or the numpy array ``fill`` (an operand updated in place)."""
        r, c = self._lay(n)
        t = canary(r, c) if fill is None else torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float32)).reshape(r, c)
        self.outputs[name] = Guarded(r, c, fill=t)
        return self.outputs[name]

    def check(self, what):
        for name, gd in self.inputs.items():
            gd.check(f"{what}: input {name}", unchanged=True)
        for name, gd in self.outputs.items():
            gd.check(f"{what}: output {name}")


def flat(gd, shape=None):
    a = gd.host().numpy().reshape(-1)
    return a if shape is None else a.reshape(shape)


def sigma_rows_hold(sig, value, R, what):
    got = flat(sig)
    assert got.shape == (R,) and S.same_bits32(got, np.full(R, np.float32(value))), f"{what}: sig_rows is {got[:4]} .., not {value}"


@pytest.mark.parametrize("size", sorted(S.SIZES))
@pytest.mark.parametrize("sigma", [80.0, 0.5, 0.001])
def test_steer_seed(lib, size, sigma):
    """D, e and dF at every size and sigma (the grid covers N alone: at "second_trip" the loop's second trip)."""
    N, R, A = S.SIZES[size]
    L, what = lib.load(), f"steer_seed {size} sigma {sigma}"
    op = S.seed_operands(N)
    O = Ops(S.cols_of(N, A))
    F, x, known, w = (O.inp(k, op[k]) for k in ("F", "x", "known", "weight"))
    D, e, dF = (O.out(k, N) for k in ("D", "e", "dF"))
    lib.check(L.mdt_op_steer_seed(F.ptr, x.ptr, known.ptr, w.ptr, sigma, S.SD, N, D.ptr, e.ptr, dF.ptr, stream()))
    torch.cuda.synchronize()
    O.check(what)
    want, b = S.seed_ref(op, sigma, S.SD), S.seed_bounds(op, sigma, S.SD)
    for k, gd in (("D", D), ("e", e), ("dF", dF)):
        gd.check(f"{what}: {k}", written=True)
        bad = S.outside(flat(gd), want[k], b[k])
        print(f"{what}: {k} largest error / bound {S.ratio(flat(gd), want[k], b[k]):.3f}")
        assert bad is None, f"{what}: {k} element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"


@pytest.mark.parametrize("size", sorted(S.SIZES))
@pytest.mark.parametrize("aliased", [False, True], ids=["distinct", "aliased"])
@pytest.mark.parametrize("bounded", [False, True], ids=["free", "bounded"])
def test_steer_step(lib, size, aliased, bounded):
    """x_out = ratio x_in + coef D', aliased with x_in and distinct, with and without bounds (one column has lo > hi and gives hi);
    the R sigma rows hold sigma_next's bits.  Bounds need rows of A columns: the two sizes that are no multiple of 7 run free."""
    N, R, A = S.SIZES[size]
    if bounded and N % A:
        N = N // A * A          # the nearest size below that has whole rows: still past the capacity at "second_trip"
        assert size in ("capacity", "second_trip") and (N > S.CAP) == (size == "second_trip")
    L, what = lib.load(), f"steer_step {size} N {N} {'aliased' if aliased else 'distinct'} {'bounded' if bounded else 'free'}"
    op = S.step_operands(N, A, bounded)
    O = Ops(S.cols_of(N, A))
    small, e, D = (O.inp(k, op[k]) for k in ("small", "e", "D"))
    lo = O.inp("lo", op["lo"]) if bounded else None
    hi = O.inp("hi", op["hi"]) if bounded else None
    x_in = O.out("x", N, fill=op["x_in"]) if aliased else O.inp("x_in", op["x_in"])
    x_out = x_in if aliased else O.out("x_out", N)
    sig = O.out("sig_rows", R)
    p = S.STEP
    lib.check(L.mdt_op_steer_step(small.ptr, e.ptr, D.ptr, x_in.ptr, p["sigma"], S.SD, p["scale"], p["ratio"], p["coef"],
                                  lo.ptr if lo else None, hi.ptr if hi else None, A, p["sigma_next"], N, R, x_out.ptr, sig.ptr,
                                  stream()))
    torch.cuda.synchronize()
    O.check(what)
    x_out.check(what + ": x_out", written=True)
    got, want, b = flat(x_out), S.step_ref(op, A), S.step_bound(op)
    bad = S.outside(got, want, b)
    print(f"{what}: largest error / bound {S.ratio(got, want, b):.3f}")
    assert bad is None, f"{what}: element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"
    sigma_rows_hold(sig, p["sigma_next"], R, what)
    if bounded:
        col = np.arange(N) % A
        assert (got <= op["hi"][col]).all() and (got[col == 1 % A] == op["hi"][1 % A]).all(), f"{what}: outside the bounds"
        assert S.same_bits32(got[want == op["hi"][col]], want[want == op["hi"][col]].astype(np.float32))


def test_steer_step_over_no_elements_fills_the_sigma_rows(lib):
    """N = 0, R = 5, every element pointer null: what fill_sigma launches before the first forward."""
    N, R, A = S.SIGMA_ONLY
    L = lib.load()
    sig = Guarded(1, R, fill=canary(1, R))
    lib.check(L.mdt_op_steer_step(None, None, None, None, 1.0, 1.0, 0.0, 0.0, 0.0, None, None, A, 80.0, N, R, None, sig.ptr, stream()))
    torch.cuda.synchronize()
    sig.check("steer_step over no elements", written=True)
    sigma_rows_hold(sig, 80.0, R, "steer_step over no elements")


@pytest.mark.parametrize("size", sorted(S.SIZES))
@pytest.mark.parametrize("form", ["row", "zero_cn", "null_row"])
def test_steer_first(lib, size, form):
    """X = x_T's bits; Y = x_T + cn n0 -- x_T's bits with cn = 0 and a row given, and with a null row --; the four history slots
    zeroed over the canary; the R sigma rows."""
    N, R, A = S.SIZES[size]
    L, what = lib.load(), f"steer_first {size} {form}"
    cn, with_row = (0.0 if form == "zero_cn" else 0.7), form != "null_row"
    op = S.first_operands(N)
    O = Ops(S.cols_of(N, A))
    x_T, n0 = O.inp("x_T", op["x_T"]), O.inp("n0", op["n0"])
    X, Y, hist, sig = O.out("X", N), O.out("Y", N), O.out("hist", 4 * N), O.out("sig_rows", R)
    lib.check(L.mdt_op_steer_first(x_T.ptr, n0.ptr if with_row else None, cn, 80.0, N, R, X.ptr, Y.ptr, hist.ptr, sig.ptr, stream()))
    torch.cuda.synchronize()
    O.check(what)
    assert S.same_bits32(flat(X), op["x_T"]), f"{what}: X is not x_T's bits"
    got, want, b = flat(Y), S.first_ref(op, cn, with_row), S.first_bound(op, cn, with_row)
    bad = S.outside(got, want, b)
    assert bad is None, f"{what}: Y element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"
    if form != "row":
        assert S.same_bits32(got, op["x_T"]), f"{what}: Y is not x_T's bits"
    else:
        print(f"{what}: Y largest error / bound {S.ratio(got, want, b):.3f}")
        assert not S.same_bits32(got, op["x_T"])
    assert not bool(bits(hist.region).any()), f"{what}: a history slot is not +0"
    sigma_rows_hold(sig, 80.0, R, what)


@pytest.mark.parametrize("c", S.PLAN_CASES, ids=S.case_id)
def test_steer_plan(lib, rows, c):
    """One evaluation of a plan per case of steer_ops_cases.PLAN_CASES: X', Y', the record, the history shift and the sigma rows
    against the float64 restatement; what the evaluation leaves alone (a record without begins_step, the history without a push)
    keeps its bits."""
    ev, op, N, R, A = S.plan_case(c, rows)
    L, what = lib.load(), "steer_plan " + S.case_id(c)
    O = Ops(S.cols_of(N, A))
    small, e, D = (O.inp(k, op[k]) for k in ("small", "e", "D"))
    noise = O.inp("noise", op["noise_rows"]) if op["noise_rows"] is not None else None   # allocated even where the call passes null
    lo = O.inp("lo", op["lo"]) if op["lo"] is not None else None
    hi = O.inp("hi", op["hi"]) if op["hi"] is not None else None
    if c["inplace"]:
        X, Y = O.out("X", N, fill=op["X"]), O.out("Y", N, fill=op["Y"])
        x_out, y_out = X, Y
    else:
        X, Y = O.inp("X", op["X"]), O.inp("Y", op["Y"])
        x_out, y_out = O.out("x_out", N), None
    hist = O.out("hist", 4 * N, fill=op["hist"])
    rec = O.out("rec", 2 * N) if op["rec"] else None
    sig = O.out("sig_rows", R)
    scale = float(S.host_scale(S.BETA, ev.sigma, S.SD))
    lib.check(L.mdt_op_steer_plan(C.byref(ev), small.ptr, e.ptr, D.ptr, Y.ptr, X.ptr, x_out.ptr, y_out.ptr if y_out else None, hist.ptr,
                                  noise.ptr if noise is not None and op["noise"] is not None else None, lo.ptr if lo else None,
                                  hi.ptr if hi else None, rec.ptr if rec else None, sig.ptr, N, R, S.SD, scale, op["n_noise"], A,
                                  stream()))
    torch.cuda.synchronize()
    O.check(what)
    got = {"x": flat(x_out), "y": flat(y_out) if y_out else None, "hist": flat(hist, (4, N)), "rec": flat(rec, (2, N)) if rec else None}
    text, worst = S.plan_check(ev, op, A, got, what, y_given=y_out is not None)
    print(f"{what}: largest error / bound {worst:.3f}")
    assert text is None, text
    sigma_rows_hold(sig, ev.sigma_next, R, what)
    if rec is not None and not ev.begins_step:
        assert rec.keeps(), f"{what}: the record's rows changed in an evaluation that begins no step"
    if op["lo"] is not None and ev.ends_step:
        col = np.arange(N) % A
        with np.errstate(invalid="ignore"):
            assert not (got["x"] > op["hi"][col]).any(), f"{what}: X' above hi"
            assert not ((got["x"] < op["lo"][col]) & (op["lo"][col] <= op["hi"][col])).any(), f"{what}: X' below lo"
    if c["nan"]:
        assert np.isnan(got["x"][3]) and np.isnan(got["x"]).sum() == 1, f"{what}: the NaN of D[3] did not stay one NaN"


def test_a_refused_call_writes_nothing(lib):
    """One refusal per hook on real device buffers (tests/test_cpu_steer_ops_abi.py pins every cause): the outputs keep the canary."""
    L = lib.load()
    N, R, A = S.SIZES["one_block"]
    op = S.step_operands(N, A, True)
    O = Ops(A)
    small, e, D, x_in, lo, hi = (O.inp(k, op[k]) for k in ("small", "e", "D", "x_in", "lo", "hi"))
    outs = [O.out(f"out{k}", 4 * N) for k in range(3)] + [O.out("sig", R)]
    a, b, c, sig = outs
    ev = S.plan_rows()["synthetic"]
    s = stream()
    assert L.mdt_op_steer_seed(small.ptr, e.ptr, D.ptr, x_in.ptr, float("nan"), S.SD, N, a.ptr, b.ptr, c.ptr, s) == 1
    assert L.mdt_op_steer_step(small.ptr, e.ptr, D.ptr, x_in.ptr, 2.0, S.SD, 1.0, 0.5, 0.5, lo.ptr, None, A, 1.0, N, R, a.ptr, sig.ptr, s) == 1
    assert L.mdt_op_steer_first(x_in.ptr, None, 0.0, 0.0, N, R, a.ptr, b.ptr, c.ptr, sig.ptr, s) == 1
    assert L.mdt_op_steer_plan(C.byref(ev), small.ptr, e.ptr, D.ptr, x_in.ptr, x_in.ptr, a.ptr, b.ptr, c.ptr, None, lo.ptr, hi.ptr, None,
                               sig.ptr, N - 1, R, S.SD, 1.0, 0, A, s) == 1
    torch.cuda.synchronize()
    O.check("refused calls")
    assert all(o.keeps() for o in outs), "a refused call wrote an output"
