"""The bounds of tests/test_gpu_score_ops.py on the host, no GPU: they admit a correct result and refuse a wrong one.

For every case of tests/score_ops_cases.py the fp32 emulation of k_score_prep and k_score_reduce -- the kernel's own operation
order -- is inside the derived bound of the float64 restatement, and every planted defect of the restatement that the case can show
(score_ops_cases.DEFECTS, *_shows) is outside it.  A defect the case cannot show (M = 1 for the undivided weight, S = 1 for the
noise row, ...) leaves the restatement's values as they are, so ``shows`` is exactly the set; over the cases every defect is shown.
The largest emulation error / bound per kernel is printed (DESIGN.md records it)."""
import os

import numpy as np
import pytest

from tests import score_ops_cases as S

WORST = {"prep": 0.0, "reduce": 0.0}


def test_the_tables_hold_the_shapes_and_edges():
    P, R, Q = S.PREP_CASES, S.REPEAT_CASES, S.REDUCE_CASES
    dims = lambda c: tuple(c[k] for k in ("B", "S", "K", "M", "Ta", "A", "D"))
    assert dims(P["ones"]) == (1, 1, 1, 1, 1, 1, 16) and dims(P["distinct"]) == (2, 3, 5, 7, 3, 7, 64)
    assert len({P["distinct"][k] for k in "BSKM"}) == 4
    assert {(c["A"], c["D"]) for c in P.values()} >= {(A, D) for A in (1, 7, 17, 64) for D in (16, 144, 384, 512)}
    assert any(c["Ta"] == 64 for c in P.values())
    assert any(c["S"] == 64 and c["M"] == 1 for c in P.values()) and any(c["M"] == 64 and c["S"] == 1 for c in P.values())
    assert {c["ctx"] for c in P.values()} == {True, False} and any(c["extreme"] for c in P.values())
    c = P["past_grid_cap"]
    assert dims(c) == (2, 5, 41, 2, 10, 3, 512) and c["B"] * c["S"] * c["K"] * c["M"] * c["Ta"] * (c["D"] // 4) > S.CAP
    assert {(c["w"], c["S"], c["B"]) for c in R.values()} >= {(w, s, b) for w in S.WIDTHS for s in (1, 3, 64) for b in (1, 3)}
    c = R["past_grid_cap"]
    assert c["w"][1] == 0 and c["B"] * c["S"] * sum(c["w"]) > S.CAP
    assert {c["E"] for c in Q.values()} >= set(S.ES) and {(c["B"], c["K"]) for c in Q.values()} >= set(S.BKS)
    assert {(c["S"], c["M"]) for c in Q.values()} >= set(S.SMS) and Q["s64_m64_e3"]["E"] == 3
    assert {c["weights"] for c in Q.values()} == {"trapezoid", "some_zero", "all_zero", "one_1e6"}
    assert any(c["extreme"] for c in Q.values()) and any(c["K"] == 1 and c["B"] > 1 for c in Q.values())
    lv = S.levels_of(5)
    assert lv[0] == np.float32(80.0) and lv[-1] == np.float32(0.001) and (np.diff(lv) < 0).all()
    assert S.levels_of(2, True).tolist() == [np.float32(1e4), np.float32(1e-6)]


def test_the_launch_constants_are_the_kernels():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdt_policy_amd", "csrc")
    with open(os.path.join(src, "mdt_score.hip")) as f:
        text = f.read()
    assert "constexpr int SCORE_THREADS = 256;" in text and "constexpr int SCORE_MAX_BLOCKS = 4096;" in text
    with open(os.path.join(src, "mdt_internal.h")) as f:
        assert "constexpr int MDT_SCORE_MAX = 64;" in f.read()
    assert (S.THREADS, S.MAX_BLOCKS, S.SCORE_MAX) == (256, 4096, 64)


@pytest.mark.parametrize("name", sorted(S.PREP_CASES))
def test_an_emulated_prep_is_inside_and_every_defect_it_can_show_outside(name):
    c = S.PREP_CASES[name]
    op = S.prep_operands(c)
    text, worst = S.prep_check(c, op, S.prep_emulate(c, op), name)
    WORST["prep"] = max(WORST["prep"], worst)
    print(f"prep {name}: emulation, largest y error / bound {worst:.3f}; over the cases so far {WORST['prep']:.3f}")
    assert text is None, text
    assert worst <= 1.0
    plain, can = S.prep_ref(c, op), S.prep_shows(c)
    for defect in S.PREP_DEFECTS:
        wrong = S.prep_ref(c, op, defect)
        got = {k: S.as_f32(wrong[k]) for k in ("noised", "y", "sig_rows", "ctx_sig")}
        if defect in can:
            text, _ = S.prep_check(c, op, got, defect)
            assert text is not None, f"{name}: the defect {defect} ({S.DEFECTS[defect]}) is inside every bound"
        else:
            print(f"prep {name}: {defect} is unobservable here")
            for k in ("noised", "y", "sig_rows") + (("ctx_sig",) if c["ctx"] else ()):
                assert np.array_equal(wrong[k], plain[k], equal_nan=True), f"{name}: {defect} shows in {k}, `prep_shows` says it cannot"
    if c["ctx"]:
        assert not np.isnan(plain["ctx_sig"]).any()


@pytest.mark.parametrize("name", sorted(S.REDUCE_CASES))
def test_an_emulated_reduce_is_inside_and_every_defect_it_can_show_outside(name):
    c = S.REDUCE_CASES[name]
    op = S.reduce_operands(c)
    want, terms = S.reduce_ref(c, op)
    bound = S.reduce_bound(c, op)
    got = S.reduce_emulate(c, op)
    worst = S.ratio(got, want, bound)
    WORST["reduce"] = max(WORST["reduce"], worst)
    print(f"reduce {name}: emulation, largest error / bound {worst:.3f}; over the cases so far {WORST['reduce']:.3f}")
    bad = S.outside(got, want, bound)
    assert bad is None, f"{name}: chunk {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"
    assert (terms >= -want).all()
    if c["weights"] == "all_zero":
        assert (got == 0).all() and (bound == 0).all()
    can = S.reduce_shows(c, op)
    for defect in S.REDUCE_DEFECTS:
        wrong = S.reduce_ref(c, op, defect)[0]
        if defect in can:
            assert S.outside(S.as_f32(wrong), want, bound) is not None, \
                f"{name}: the defect {defect} ({S.DEFECTS[defect]}) is inside the bound of every chunk"
        else:
            print(f"reduce {name}: {defect} is unobservable here")
            assert np.array_equal(wrong, want), f"{name}: {defect} shows, `reduce_shows` says it cannot"


def test_every_defect_is_shown_by_some_case():
    seen = set()
    for c in S.PREP_CASES.values():
        seen |= S.prep_shows(c)
    for c in S.REDUCE_CASES.values():
        seen |= S.reduce_shows(c, S.reduce_operands(c))
    assert seen == set(S.DEFECTS), set(S.DEFECTS) - seen


def test_repeat_restates_the_rows():
    c = S.REPEAT_CASES["w5_3_7_s3_b3"]
    op = S.repeat_operands(c)
    out = S.repeat_ref(c, op)
    assert out["tok_o"].shape == (9, 5) and S.same_bits32(out["tok_o"][4], op["tok"][1]) and S.same_bits32(out["tok2_o"][8], op["tok2"][2])
    assert len({r.tobytes() for r in op["goal"]}) == 3
    assert S.repeat_ref(S.REPEAT_CASES["w5_0_7_s3_b3"], S.repeat_operands(S.REPEAT_CASES["w5_0_7_s3_b3"]))["tok2_o"] is None
