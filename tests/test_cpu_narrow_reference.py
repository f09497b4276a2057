"""The bounds of tests/test_gpu_narrow_ops.py on the host, no GPU: they admit a correct result and refuse a wrong one.

A correctly rounded result -- the float64 reference rounded to fp32 -- is inside every slab bound and every summed bound (a slice
without rows: exact zeros).  A reference with ONE row left out of its slice is outside the slab bound at every element of that
slab: the inputs' magnitudes are at least 0.5, so the row's term is at least 0.25, and the bound of the deepest slice here (16 rows)
stays below 1e-4."""
import pytest
import torch

from tests.test_gpu_narrow_ops import DW_CASES, OUT_AD, SLICES, U, dw_inputs, dw_reference, first_outside, out_inputs, slab_bound, slice_bounds, sum_bound

# the deepest and the shallowest slices, a row count that is no multiple of 512, both layouts, both kernel forms
CASES = [(3, 7, 384, 0), (513, 33, 144, 1), (2048, 7, 384, 0), (2600, 64, 384, 1), (2600, 17, 112, 0), (8192, 7, 384, 0), (8192, 33, 144, 1)]


def test_the_cases_are_among_the_gpu_tests():
    assert all(any(c == g[:4] for g in DW_CASES) for c in CASES)
    assert slice_bounds(513)[:3] == [(0, 1), (1, 2), (2, 3)] and slice_bounds(513)[-1] == (511, 513) and slice_bounds(3)[170:172] == [(0, 1), (1, 1)]
    assert sorted({m1 - m0 for m0, m1 in slice_bounds(2600)}) == [5, 6] and {m1 - m0 for m0, m1 in slice_bounds(8192)} == {16}


@pytest.mark.parametrize("M,A,D,transposed", CASES)
def test_a_rounded_reference_is_inside_and_a_dropped_row_outside(M, A, D, transposed):
    G, Y = dw_inputs(M, A, D)
    assert float(G.abs().min()) >= 0.5 and float(Y.abs().min()) >= 0.5 and float(G.abs().max()) <= 1.5 and float(Y.abs().max()) <= 1.5
    slabs, mags, rows = dw_reference(G, Y, transposed)
    bound = slab_bound(mags, rows)
    assert float(bound.max()) <= 16 * U * 16 * 2.25 + 1e-12 and float(bound.max()) < 1e-4
    assert first_outside(slabs.float(), slabs, bound) is None
    assert not bool(slabs[rows == 0].any())
    assert first_outside(slabs.sum(0).float(), slabs.sum(0), sum_bound(mags, rows)) is None
    # the sum of rounded slabs, formed in float64 (any order of fp32 additions is within the 512 further roundings of the bound)
    assert first_outside(slabs.float().double().sum(0).float(), slabs.sum(0), sum_bound(mags, rows)) is None
    for row in sorted({0, M // 2, M - 1}):
        y = next(i for i, (m0, m1) in enumerate(slice_bounds(M)) if m0 <= row < m1)
        wrong, _, _ = dw_reference(G, Y, transposed, skip_row=row)
        assert float((wrong[y] - slabs[y]).abs().min()) >= 0.25 - 1e-12
        assert bool(((wrong[y].float().double() - slabs[y]).abs() > bound[y]).all()), f"row {row} dropped from slice {y}: inside the bound"
        assert first_outside(wrong.float(), slabs, bound) is not None


@pytest.mark.parametrize("A,D", OUT_AD)
def test_a_rounded_product_is_inside_the_out_and_dx_bounds(A, D):
    Gr, W, Ga = out_inputs(5, A, D)
    want = Gr.double() @ W.double().T
    assert first_outside(want.float(), want, D * U * (Gr.double().abs() @ W.double().abs().T)) is None
    want = Ga.double() @ W.double()
    assert first_outside(want.float(), want, A * U * (Ga.double().abs() @ W.double().abs())) is None
    assert first_outside((want + 0.25).float(), want, A * U * (Ga.double().abs() @ W.double().abs())) is not None


def test_slices_is_the_steps_value():
    import os
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdt_policy_amd", "csrc", "mdt_train.hip")
    with open(src) as f:
        assert f"static const int NARROW_SLICES = {SLICES};" in f.read()
