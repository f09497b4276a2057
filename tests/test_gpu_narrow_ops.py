"""The narrow linears around the action tokens, kernel by kernel, against float64 (pytest -m gpu): mdt_op_narrow_dw, mdt_op_narrow_out
and mdt_op_narrow_dx of include/mdt_hip_debug.h -- the launchers the training step calls for action_pred.weight, action_emb.weight,
the MLP head's output layer and the proprioceptive token's first layer -- on the operands of tests/guarded.py (guard bands, padded
strides).

The reference is the plain product in float64.  Tolerances are derived: an fp32 fma chain of n terms followed by any summation
order of s partials is within (n + s) 2^-24 sum|terms| of the exact sum, sum|terms| taken in float64 per output element.
  narrow_dw, slab y    n = rows of slice y, s = 0 (a slice without rows: exact zeros)
  summed slabs         n = the longest slice, s = 512
  narrow_out           n + s <= D        narrow_dx    n + s <= A
The inputs have magnitudes in [0.5, 1.5] and random signs: every term of a slab is at least 0.25 in magnitude, so a dropped,
duplicated or misplaced row moves a slab element by at least 0.25, four orders of magnitude above a 16-row slice's bound (4e-5).
tests/test_cpu_narrow_reference.py checks both halves of that on the host: the float64 reference rounded to fp32 is inside every
bound, a reference with one row removed is not."""
import numpy as np
import pytest
import torch

from tests.guarded import GuardedSet, bits
from tests.test_gpu_ops import stream
from tests.test_gpu_ops_bounds import seeded

pytestmark = pytest.mark.gpu

SLICES = 512           # NARROW_SLICES of mdt_train.hip: the step's value, whatever the batch
U = 2.0 ** -24         # unit roundoff of fp32
MLP_HEAD_HIDDEN = 112  # HP: the MDT-V MLP head's 100 hidden units, padded to a multiple of 16 as the model passes them

DW_M_ALL = [1, 3, 511, 512, 513, 2047, 2048, 2600, 8192]
DW_M_TWO = [513, 2600]
# (A, D, transposed, ldy)
DW_FORMS_ALL = [(7, 384, 0, 388), (33, 144, 1, 148)]
DW_FORMS_TWO = [(16, 384, 1, 388), (17, 384, 0, 388), (17, MLP_HEAD_HIDDEN, 0, MLP_HEAD_HIDDEN), (64, 512, 0, 516), (64, 384, 1, 388),
                (9, 768, 1, 768)]   # (9, 768, 1): the proprioceptive layer's form, three 256-column blocks
DW_CASES = [(M,) + f for f in DW_FORMS_ALL for M in DW_M_ALL] + [(M,) + f for f in DW_FORMS_TWO for M in DW_M_TWO]

OUT_M = [1, 3, 4, 5, 2600]   # four rows share a workgroup of k_narrow_out
# every A at two values of D, every D at two values of A
OUT_AD = [(1, 100), (1, 384), (16, 144), (16, 768), (17, 100), (17, 512), (33, 144), (33, 384), (64, 512), (64, 768)]


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def draw(g, rows, cols):
    """Magnitudes in [0.5, 1.5], random signs."""
    mag = 0.5 + torch.rand(rows, cols, generator=g)
    sign = torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1
    return mag * sign


def slice_bounds(M, n_slices=SLICES):
    """Rows [m0, m1) of every slice: slice y owns [M y / n, M (y + 1) / n)."""
    edges = [M * y // n_slices for y in range(n_slices + 1)]
    return list(zip(edges[:-1], edges[1:]))


def dw_inputs(M, A, D):
    g = seeded("narrow_dw", M, A, D)
    return draw(g, M, A), draw(g, M, D)


def dw_reference(G, Y, transposed, skip_row=None):
    """(slabs, sum|terms| of every slab, rows of every slice) in float64; slabs (512, A, D), or (512, D, A) transposed.
    skip_row: leave that row out of its slice (the host check that the bounds notice a dropped row)."""
    M, A, D = G.shape[0], G.shape[1], Y.shape[1]
    G64, Y64 = G.double(), Y.double()
    slabs, mags, rows = torch.zeros(SLICES, A, D, dtype=torch.float64), torch.zeros(SLICES, A, D, dtype=torch.float64), []
    for y, (m0, m1) in enumerate(slice_bounds(M)):
        keep = [m for m in range(m0, m1) if m != skip_row]
        rows.append(m1 - m0)
        if keep:
            slabs[y] = G64[keep].T @ Y64[keep]
            mags[y] = G64[keep].abs().T @ Y64[keep].abs()
    if transposed:
        slabs, mags = slabs.transpose(1, 2).contiguous(), mags.transpose(1, 2).contiguous()
    return slabs, mags, torch.tensor(rows)


def slab_bound(mags, rows):
    """n 2^-24 sum|terms| per element of every slab, n the slice's rows."""
    return rows.double()[:, None, None] * U * mags


def sum_bound(mags, rows):
    """(longest slice + 512) 2^-24 sum|terms| per element of the summed result."""
    return (float(rows.max()) + SLICES) * U * mags.sum(0)


def first_outside(got, want, bound):
    """None, or (index, got, want, bound) of the element furthest outside its bound."""
    excess = (got.double() - want).abs() - bound
    if not bool((excess > 0).any()) and not bool(got.isnan().any()):
        return None
    excess = torch.where(got.isnan(), torch.full_like(excess, float("inf")), excess)
    idx = tuple(int(v) for v in np.unravel_index(int(excess.argmax()), tuple(got.shape)))
    return idx, float(got[idx]), float(want[idx]), float(bound[idx])


@pytest.mark.parametrize("M,A,D,transposed,ldy", DW_CASES)
def test_narrow_dw_slabs_and_their_sum(lib, M, A, D, transposed, ldy):
    """mdt_op_narrow_dw at 512 slices: slab y is the float64 sum over exactly the rows [M y / 512, M (y + 1) / 512) to n 2^-24
    sum|terms| -- a slice without rows is zeros --; every element of `partial` is written, a second call leaves the same bits
    (nothing accumulates), the guard bands hold, the pad columns of Y (NaN) reach nothing; then the column sum of the slabs by
    mdt_op_colsum, as the step forms it, against G^T Y to (longest slice + 512) 2^-24 sum|terms|.
    M < 512: slices of zero or one row; 513: one slice of two rows; 2047: one slice of three rows among 511 of four, which run
    the unrolled four-row trip once and nothing else; 2048: every slice that trip alone; 2600: slices of 5 and 6 rows, both
    loops; 8192: four trips; 513, 2047 and 2600 are no multiples of 512."""
    L = lib.load()
    G, Y = dw_inputs(M, A, D)
    slabs, mags, rows = dw_reference(G, Y, transposed)
    assert int(rows.sum()) == M and int(rows.max()) - int(rows.min()) <= 1
    what = f"narrow_dw M {M}, A {A}, D {D}, transposed {transposed}, ldy {ldy}"
    S = GuardedSet()
    Gd, Yd = S.inp("G", G), S.inp("Y", Y, ld=ldy)
    part = S.out("partial", SLICES, A * D)
    total = S.out("sum", 1, A * D)
    lib.check(L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, ldy, part.ptr, SLICES, M, A, D, transposed, stream()))
    torch.cuda.synchronize()
    S.check(what)
    part.check(what + ": partial", written=True)
    got = part.host().reshape(slabs.shape)
    empty = rows == 0
    assert not bool(got[empty].view(torch.int32).any()), f"{what}: a slice without rows is not written as zeros"
    bad = first_outside(got, slabs, slab_bound(mags, rows))
    print(f"{what}: slices of {int(rows.min())} .. {int(rows.max())} rows, largest slab bound {float(slab_bound(mags, rows).max()):.3e}")
    assert bad is None, f"{what}: slab element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e} ({int(rows[bad[0][0]])} rows)"
    first = bits(part.region)
    lib.check(L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, ldy, part.ptr, SLICES, M, A, D, transposed, stream()))
    torch.cuda.synchronize()
    assert part.keeps(first), f"{what}: a second call onto its own result changes it"
    S.check(what + ", second call")

    lib.check(L.mdt_op_colsum(part.ptr, A * D, SLICES, A * D, total.ptr, 0, stream()))
    torch.cuda.synchronize()
    S.check(what + ", colsum")
    total.check(what + ": sum", written=True)
    bad = first_outside(total.host().reshape(slabs.shape[1:]), slabs.sum(0), sum_bound(mags, rows))
    assert bad is None, f"{what}: summed element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"


def out_inputs(M, A, D):
    g = seeded("narrow_out", M, A, D)
    return draw(g, M, D), draw(g, A, D), draw(g, M, A)


@pytest.mark.parametrize("M", OUT_M)
@pytest.mark.parametrize("A,D", OUT_AD)
def test_narrow_out_and_narrow_dx(lib, M, A, D):
    """mdt_op_narrow_out: out (M, A) = G WT^T with G's row stride padded, to D 2^-24 sum|terms| (lanes stride over D, then a
    wavefront sum: n + s <= D); mdt_op_narrow_dx: out (M, D) = Ga W, to A 2^-24 sum|terms|.  M = 3, 4, 5: one row short of a
    workgroup's four, exactly four, one into the next; 2600 rows: many workgroups."""
    L = lib.load()
    Gr, W, Ga = out_inputs(M, A, D)
    what = f"M {M}, A {A}, D {D}"
    S = GuardedSet()
    Gd, Wd = S.inp("G", Gr, ld=D + 4), S.inp("WT", W)
    out = S.out("out", M, A)
    lib.check(L.mdt_op_narrow_out(Gd.ptr, Gd.ld, Wd.ptr, out.ptr, M, A, D, stream()))
    torch.cuda.synchronize()
    S.check("narrow_out " + what)
    out.check("narrow_out " + what, written=True)
    bad = first_outside(out.host(), Gr.double() @ W.double().T, D * U * (Gr.double().abs() @ W.double().abs().T))
    assert bad is None, f"narrow_out {what}: element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"

    S = GuardedSet()
    Gd, Wd = S.inp("G", Ga), S.inp("W", W)
    out = S.out("out", M, D)
    lib.check(L.mdt_op_narrow_dx(Gd.ptr, Wd.ptr, out.ptr, M, A, D, stream()))
    torch.cuda.synchronize()
    S.check("narrow_dx " + what)
    out.check("narrow_dx " + what, written=True)
    bad = first_outside(out.host(), Ga.double() @ W.double(), A * U * (Ga.double().abs() @ W.double().abs()))
    assert bad is None, f"narrow_dx {what}: element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"


def test_the_hooks_refuse_bad_arguments_before_they_launch(lib):
    """A null pointer, M < 1, A outside 1 .. 64, n_slices < 1, a row stride below the row length: MDT_ERR_INVALID_ARG with a text,
    and the output keeps its fill."""
    L = lib.load()
    M, A, D = 8, 7, 64
    G, Y = dw_inputs(M, A, D)
    S = GuardedSet()
    Gd, Yd, Wd, Gr = S.inp("G", G), S.inp("Y", Y), S.inp("W", draw(seeded("refuse"), A, D)), S.inp("Grow", Y, ld=D + 4)
    part, out, dx = S.out("partial", SLICES, A * D), S.out("out", M, A), S.out("dx", M, D)
    s = stream()
    calls = {
        "dw: G null": lambda: L.mdt_op_narrow_dw(None, Yd.ptr, D, part.ptr, SLICES, M, A, D, 0, s),
        "dw: Y null": lambda: L.mdt_op_narrow_dw(Gd.ptr, None, D, part.ptr, SLICES, M, A, D, 0, s),
        "dw: partial null": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D, None, SLICES, M, A, D, 0, s),
        "dw: M 0": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D, part.ptr, SLICES, 0, A, D, 0, s),
        "dw: A 0": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D, part.ptr, SLICES, M, 0, D, 0, s),
        "dw: A 65": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D, part.ptr, SLICES, M, 65, D, 0, s),
        "dw: no slices": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D, part.ptr, 0, M, A, D, 0, s),
        "dw: ldy below D": lambda: L.mdt_op_narrow_dw(Gd.ptr, Yd.ptr, D - 1, part.ptr, SLICES, M, A, D, 0, s),
        "out: G null": lambda: L.mdt_op_narrow_out(None, D + 4, Wd.ptr, out.ptr, M, A, D, s),
        "out: WT null": lambda: L.mdt_op_narrow_out(Gr.ptr, D + 4, None, out.ptr, M, A, D, s),
        "out: out null": lambda: L.mdt_op_narrow_out(Gr.ptr, D + 4, Wd.ptr, None, M, A, D, s),
        "out: M 0": lambda: L.mdt_op_narrow_out(Gr.ptr, D + 4, Wd.ptr, out.ptr, 0, A, D, s),
        "out: A 0": lambda: L.mdt_op_narrow_out(Gr.ptr, D + 4, Wd.ptr, out.ptr, M, 0, D, s),
        "out: A 65": lambda: L.mdt_op_narrow_out(Gr.ptr, D + 4, Wd.ptr, out.ptr, M, 65, D, s),
        "out: ldg below D": lambda: L.mdt_op_narrow_out(Gr.ptr, D - 1, Wd.ptr, out.ptr, M, A, D, s),
        "dx: G null": lambda: L.mdt_op_narrow_dx(None, Wd.ptr, dx.ptr, M, A, D, s),
        "dx: W null": lambda: L.mdt_op_narrow_dx(Gd.ptr, None, dx.ptr, M, A, D, s),
        "dx: out null": lambda: L.mdt_op_narrow_dx(Gd.ptr, Wd.ptr, None, M, A, D, s),
        "dx: M 0": lambda: L.mdt_op_narrow_dx(Gd.ptr, Wd.ptr, dx.ptr, 0, A, D, s),
        "dx: A 0": lambda: L.mdt_op_narrow_dx(Gd.ptr, Wd.ptr, dx.ptr, M, 0, D, s),
        "dx: A 65": lambda: L.mdt_op_narrow_dx(Gd.ptr, Wd.ptr, dx.ptr, M, 65, D, s),
    }
    for what, call in calls.items():
        assert call() == 1, f"{what}: not refused as MDT_ERR_INVALID_ARG"
        assert L.mdt_last_error().decode().startswith("mdt_op_narrow_" + what.split(":")[0] + ": "), f"{what}: no text"
    torch.cuda.synchronize()
    S.check("refused calls")
    for o in (part, out, dx):
        assert o.keeps(), "a refused call wrote its output"
