"""The three kernels of mdt_denoising_score, kernel by kernel, against float64 (pytest -m gpu): mdt_op_score_prep,
mdt_op_score_repeat and mdt_op_score_reduce of include/mdt_hip_debug.h -- each the launch the call makes -- on the operands of
tests/guarded.py: every buffer between guard bands, outputs pre-filled with the canary, inputs held to their bits.

References, cases and bounds are those of tests/score_ops_cases.py: the numpy restatement of each kernel in float64 and a bound per
output element derived there from the roundings on its path.  tests/test_cpu_score_ops_reference.py shows on the host that an fp32
execution in the kernel's order is inside every bound and each planted defect outside.

  prep    noised, the rows' sigma and the contexts' sigma are the host's bits (an IEEE product, then an IEEE sum); y is the bits of
          mdt_op_action_embed on the kernel's own noised and sigma rows, and within g(A + 6) sum|terms| of float64
  repeat  bits; with w2 == 0 tok2 is null and tok2_o is a guarded buffer the launch is given, as the call gives its staging buffer,
          and must leave as it was, bands included
  reduce  within g(24 + ceil(E / 64) + ceil(S M / 4)) sum|terms| of float64; twice the same bits; a chunk keeps its bits when every
          other chunk's rows of F and x0 are NaN

Measured on the MI355X: see DESIGN.md 4.3k."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import score_ops_cases as S
from tests.guarded import Guarded, canary
from tests.test_gpu_ops import stream
from tests.test_gpu_steer_ops import Ops, flat

pytestmark = pytest.mark.gpu
WORST = {"prep": 0.0, "reduce": 0.0}


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def floats(a):
    return (C.c_float * len(a))(*[float(v) for v in a])


@pytest.mark.parametrize("name", sorted(S.PREP_CASES))
def test_score_prep(lib, name):
    c = S.PREP_CASES[name]
    B, Sn, K, M, Ta, A, D = (c[k] for k in ("B", "S", "K", "M", "Ta", "A", "D"))
    J, rows = B * Sn * K * M, B * Sn * K * M * Ta
    L, what = lib.load(), f"score_prep {name}"
    op = S.prep_operands(c)
    O = Ops(A)
    x0, noise = O.inp("x0", op["x0"]), O.inp("noise", op["noise"])
    O.cols = D
    WaT, ba = O.inp("WaT", op["WaT"]), O.inp("ba", op["ba"])
    y, y2 = O.out("y", rows * D), O.out("y of mdt_op_action_embed", rows * D)
    O.cols = A
    noised = O.out("noised", rows * A)
    O.cols = 1
    sig, ctx = O.out("sig_rows", J), O.out("ctx_sig", B * Sn)
    lib.check(L.mdt_op_score_prep(x0.ptr, noise.ptr, floats(op["levels"]), Sn, K, M, B, Ta, A, D, S.SD, WaT.ptr, ba.ptr, y.ptr, noised.ptr,
                                  sig.ptr, ctx.ptr if c["ctx"] else None, stream()))
    torch.cuda.synchronize()
    O.check(what)
    for gd, k in ((y, "y"), (noised, "noised"), (sig, "sig_rows")) + (((ctx, "ctx_sig"),) if c["ctx"] else ()):
        gd.check(f"{what}: {k}", written=True)
    if not c["ctx"]:
        assert ctx.keeps(), f"{what}: a null ctx_sig was written all the same"
    assert y2.keeps()
    got = {"y": flat(y, (rows, D)), "noised": flat(noised, (rows, A)), "sig_rows": flat(sig), "ctx_sig": flat(ctx)}
    text, worst = S.prep_check(c, op, got, what)
    WORST["prep"] = max(WORST["prep"], worst)
    print(f"{what}: y largest error / bound {worst:.3f}; over the cases so far {WORST['prep']:.3f}")
    assert text is None, text
    # the embedding the decoder would make of these rows itself
    lib.check(L.mdt_op_action_embed(noised.ptr, sig.ptr, 1, S.SD, WaT.ptr, ba.ptr, y2.ptr, rows, A, D, Ta, stream()))
    torch.cuda.synchronize()
    O.check(what + ", then mdt_op_action_embed")
    assert S.same_bits32(flat(y2), flat(y)), f"{what}: y is not mdt_op_action_embed's bits on the same rows"


@pytest.mark.parametrize("name", sorted(S.REPEAT_CASES))
def test_score_repeat(lib, name):
    c = S.REPEAT_CASES[name]
    B, Sn, (w1, w2, wg) = c["B"], c["S"], c["w"]
    L, what = lib.load(), f"score_repeat {name}"
    op = S.repeat_operands(c)
    want = S.repeat_ref(c, op)
    tok, goal = Guarded(B, w1, fill=torch.from_numpy(op["tok"])), Guarded(B, wg, fill=torch.from_numpy(op["goal"]))
    tok2 = Guarded(B, w2, fill=torch.from_numpy(op["tok2"])) if w2 else None
    tok_o, goal_o = Guarded(B * Sn, w1, fill=canary(B * Sn, w1)), Guarded(B * Sn, wg, fill=canary(B * Sn, wg))
    tok2_o = Guarded(B * Sn, max(w2, 3), fill=canary(B * Sn, max(w2, 3)))   # w2 == 0: given all the same, and nobody may touch it
    lib.check(L.mdt_op_score_repeat(tok.ptr, tok2.ptr if w2 else None, goal.ptr, B, Sn, w1, w2, wg, tok_o.ptr, tok2_o.ptr, goal_o.ptr,
                                    stream()))
    torch.cuda.synchronize()
    for gd, k in ((tok, "tok"), (goal, "goal")) + (((tok2, "tok2"),) if w2 else ()):
        gd.check(f"{what}: input {k}", unchanged=True)
    for gd, k in ((tok_o, "tok_o"), (goal_o, "goal_o")) + (((tok2_o, "tok2_o"),) if w2 else ()):
        gd.check(f"{what}: {k}", written=True)
        assert S.same_bits32(gd.host().numpy(), want[k]), f"{what}: {k} is not row i / S of the input, bit for bit"
    if not w2:
        tok2_o.check(f"{what}: tok2_o", unchanged=True)


def run_reduce(lib, c, op, F=None, x0=None, what="", nan_rows=False):
    """One launch on guarded operands: the score (B K) as numpy.  ``nan_rows``: some chunks' rows are NaN and so are their scores."""
    B, K, Sn, M, E = (c[k] for k in "BKSME")
    O = Ops(E)
    Fd, xd, nd = O.inp("F", op["F"] if F is None else F), O.inp("x0", op["x0"] if x0 is None else x0), O.inp("noise", op["noise"])
    O.cols = 1
    score = O.out("score", B * K)
    lib.check(lib.load().mdt_op_score_reduce(Fd.ptr, xd.ptr, nd.ptr, floats(op["levels"]), floats(op["weights"]), B, Sn, K, M, E, S.SD,
                                             score.ptr, stream()))
    torch.cuda.synchronize()
    O.check(what)
    score.check(what + ": score", written=not nan_rows)
    return flat(score).copy()


@pytest.mark.parametrize("name", sorted(S.REDUCE_CASES))
def test_score_reduce(lib, name):
    c = S.REDUCE_CASES[name]
    B, K, Sn, M, E = (c[k] for k in "BKSME")
    what = f"score_reduce {name}"
    op = S.reduce_operands(c)
    got = run_reduce(lib, c, op, what=what)
    want, bound = S.reduce_ref(c, op)[0], S.reduce_bound(c, op)
    worst = S.ratio(got, want, bound)
    WORST["reduce"] = max(WORST["reduce"], worst)
    print(f"{what}: largest error / bound {worst:.3f}; over the cases so far {WORST['reduce']:.3f}")
    bad = S.outside(got, want, bound)
    assert bad is None, f"{what}: chunk {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"
    if c["weights"] == "all_zero":
        assert (got == 0).all(), f"{what}: all-zero weights give {got}"
    assert S.same_bits32(run_reduce(lib, c, op, what=what + ", again"), got), f"{what}: a second call gives other bits"
    # one writer per element, no cross-read: chunk r alone among NaN
    r = (B * K) // 2
    b, k = divmod(r, K)
    F = np.full_like(op["F"], np.nan).reshape(B, Sn, K, M, E)
    F[b, :, k] = op["F"].reshape(B, Sn, K, M, E)[b, :, k]
    x0 = np.full_like(op["x0"], np.nan)
    x0[r] = op["x0"][r]
    alone = run_reduce(lib, c, op, F=F.reshape(op["F"].shape), x0=x0, what=what + ", the others NaN", nan_rows=True)
    assert S.same_bits32(alone[r:r + 1], got[r:r + 1]), f"{what}: chunk {r} changed when the other chunks' rows became NaN"
    assert np.isnan(np.delete(alone, r)).all(), f"{what}: a chunk of NaN rows scored a number"


def test_a_refused_call_writes_nothing(lib):
    """One refusal per hook on real device buffers (tests/test_cpu_score_ops_abi.py pins every cause): the outputs keep the canary."""
    L = lib.load()
    c = S.PREP_CASES["distinct"]
    op = S.prep_operands(c)
    O = Ops(1)
    a, b, w, ba = (O.inp(k, op[k]) for k in ("x0", "noise", "WaT", "ba"))
    outs = [O.out(f"out{k}", 4096) for k in range(4)]
    lv, s = floats(op["levels"]), stream()
    assert L.mdt_op_score_prep(a.ptr, b.ptr, lv, 3, 5, 65, 2, 3, 7, 64, S.SD, w.ptr, ba.ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                               s) == 1
    assert L.mdt_op_score_repeat(a.ptr, None, b.ptr, 2, 3, 5, 3, 7, outs[0].ptr, outs[1].ptr, outs[2].ptr, s) == 1
    assert L.mdt_op_score_reduce(a.ptr, b.ptr, w.ptr, lv, floats([1.0, float("nan"), 1.0]), 2, 3, 5, 2, 3, S.SD, outs[0].ptr, s) == 1
    torch.cuda.synchronize()
    O.check("refused calls")
    assert all(o.keeps() for o in outs), "a refused call wrote an output"
