"""The bounds of tests/mae_ops_cases.py, shown on the host to hold what is right and to refuse what is wrong: for every case
of the GPU module tests/test_gpu_mae_ops_bounds.py the float64 reference rounded to fp32 lies inside every bound, and the
reference with the op's planted defect -- the last row dropped from a column sum, the norm's clamp taken on the wrong side, key
T included in the softmax, d_out read at the stride of `out`, the incoming gradient ignored (and, for the three forwards none
of these fits, the SwishGLU halves swapped, the last row's branch left out, the last partial left out) -- lies outside one."""
import pytest
import torch

from tests import mae_ops_cases as K

CASES = K.all_cases()


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_the_reference_is_inside_and_the_planted_defect_outside(name):
    case = dict(CASES)[name]()
    assert set(case.bad) == set(case.want)
    for op, wants in case.want.items():
        for out, w in wants.items():
            assert w.outside(w.value.float()) is None, (op, out, w.outside(w.value.float()))
        caught = {out: w.outside(case.bad[op][out]) for out, w in wants.items()}
        assert any(v is not None for v in caught.values()), f"{op}: the planted defect passes every bound"


def test_the_tables_hold_the_edges_they_were_chosen_for():
    assert {M % 4 for M in K.RMS_M} >= {0, 1} and {D % 64 for D in K.RMS_D} >= {0, 1, 63}
    assert {D // 4 for D in K.SRN_D} >= {63, 64, 65} and any(256 % (D // 4) for D in K.SR_D)
    assert {63, 64, 65} <= set(K.SR_M) and {64, 65} <= set(K.SRN_M)
    ld = K.strides(48)
    assert len(set(ld)) == 4 and all(v % 4 == 0 for v in ld)
    B, H, hd, T = K.MID_HEAD_WALK
    assert T * ld[0] + 3 * H * hd < 2 ** 29
    shapes = {(s[0] * s[1] * (s[3] // s[4]) ** 2, s[0] * (s[3] // s[4]) ** 2, s[4] * s[4] * s[2]) for s in K.PATCH}
    assert max(p for p, _, _ in shapes) > 1024 and max(m for _, m, _ in shapes) > 1024 and min(e for _, _, e in shapes) < 64
    assert [K.mid_backward_fits(hd, T) for _, _, hd, T in K.MID_LDS_EDGE] == [True, True, False, False]
    x = K.clamped_rows(K.seeded("t"), 65)
    assert float(x[4].pow(2).sum()) == 0.0 and float(x[4].double().pow(2).sum()) > 0.0   # the fp32 sum of squares underflows
    assert torch.equal(x[0], torch.zeros(65))
