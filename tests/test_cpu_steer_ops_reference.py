"""The bounds of tests/test_gpu_steer_ops.py on the host, no GPU: they admit a correct result and refuse a wrong one.

For every case of tests/steer_ops_cases.py the float64 restatement of the kernel, rounded to fp32 after every operation in the
kernel's order, is inside every derived bound; and every planted defect of the plan restatement that the case can show -- the
record holding D, not D'; the history shifted in the wrong order; ``scale`` taken at sigma_next; Y' formed from the unclamped X';
a noise index >= n_noise read as row 0 -- is outside one.  A defect the case cannot show (steer_ops_cases.shows) leaves the
float64 restatement's bits as they are, so ``shows`` is exactly the set; over the cases every defect is shown."""
import numpy as np
import pytest

from tests import steer_ops_cases as S


@pytest.fixture(scope="module")
def rows():
    return S.plan_rows()


def rounded_outputs(ev, op, A, defect=None):
    r = S.plan_ref(ev, op, A, q=S.rounded, defect=defect)
    rec = None if r["rec"] is None else S.as_f32(r["rec"])
    return {"x": S.as_f32(r["x"]), "y": S.as_f32(r["y"]), "hist": S.as_f32(r["hist"]), "rec": rec, "sig": r["sig"]}


def test_the_rows_are_the_plans_and_the_cases_cover_the_features(rows):
    assert rows["heun_second"].ends_step == 1 and rows["heun_second"].cy[S.NREG] != 0
    assert rows["dpmpp_2m_third"].push != S.PUSH_NONE and rows["lms4_fifth"].push != S.PUSH_NONE
    assert max(rows["dpmpp_sde_eta1"].noise) >= 0 and max(rows["dpm_2_ancestral"].noise) >= 0
    assert all(v != 0 for v in rows["synthetic"].cx) and all(v != 0 for v in rows["synthetic"].cy)
    assert set(c["row"] for c in S.PLAN_CASES) == set(rows) and set(c["size"] for c in S.PLAN_CASES) == set(S.SIZES)
    assert len({S.case_id(c) for c in S.PLAN_CASES}) == len(S.PLAN_CASES)
    sig = {(c["sigma"]) for c in S.PLAN_CASES}
    assert {80.0, 0.5, 0.001} <= sig
    assert {c["push"] for c in S.PLAN_CASES} >= {S.PUSH_NONE, S.PUSH_D, S.PUSH_DD}
    assert {c["inplace"] for c in S.PLAN_CASES} == {True, False}
    assert any(c["bounds"] and c["ends_step"] == 0 for c in S.PLAN_CASES) and any(c["bounds"] == "inverted" for c in S.PLAN_CASES)
    assert any(c["rec"] and c["begins_step"] == 0 for c in S.PLAN_CASES) and any(c["nan"] for c in S.PLAN_CASES)
    assert any(c["noise_null"] for c in S.PLAN_CASES) and any(c["slots"] and -1 in c["slots"] for c in S.PLAN_CASES)
    # the sizes: the grid's capacity, one sigma row past it, elements past it
    N, R, A = S.SIZES["capacity"]
    assert N + R == S.CAP
    N, R, A = S.SIZES["sigma_past_cap"]
    assert N == S.CAP - 2 and N + R == S.CAP + 1 and N % A == 0
    N, R, A = S.SIZES["second_trip"]
    assert N > S.CAP
    for N, R, A in S.SIZES.values():
        assert N % S.cols_of(N, A) == 0 and S.cols_of(N, A) <= 64


@pytest.mark.parametrize("c", S.PLAN_CASES, ids=S.case_id)
def test_a_rounded_plan_evaluation_is_inside_and_every_defect_it_can_show_outside(c, rows):
    ev, op, N, R, A = S.plan_case(c, rows)
    assert all(len({h.tobytes() for h in op["hist"]}) == 4 and np.all(h != 0) for h in [op["hist"]])
    text, worst = S.plan_check(ev, op, A, rounded_outputs(ev, op, A), S.case_id(c), y_given=c["inplace"])
    print(f"{S.case_id(c)}: rounded reference, largest error / bound {worst:.3f}")
    assert text is None, text
    assert worst <= 1.0
    if c["bounds"] and ev.ends_step:   # the clamp acts, on both sides
        x = S.plan_ref(ev, op, A)["x"]
        col = np.arange(N) % A
        assert (x == op["hi"][col]).any() and ((x == op["lo"][col]) | (op["lo"][col] > op["hi"][col])).any()
        assert np.nanmax(x - op["hi"][col]) <= 0
    if c["nan"]:
        ref = S.plan_ref(ev, op, A)
        assert np.isnan(ref["x"][3]) and np.isnan(ref["x"]).sum() == 1
    can = S.shows(c, ev, op)
    plain = S.plan_ref(ev, op, A)
    for defect in S.DEFECTS:
        if defect in can:
            text, _ = S.plan_check(ev, op, A, rounded_outputs(ev, op, A, defect), defect, y_given=c["inplace"])
            assert text is not None, f"{S.case_id(c)}: the defect {defect} is inside every bound"
        else:
            wrong = S.plan_ref(ev, op, A, defect=defect)
            for k in ("x", "y", "hist") if c["inplace"] else ("x", "hist"):   # (y_out is null in the last evaluation's form)
                assert np.array_equal(wrong[k], plain[k], equal_nan=True), f"{S.case_id(c)}: {defect} shows in {k}, `shows` says it cannot"
            assert (wrong["rec"] is None) == (plain["rec"] is None)
            assert wrong["rec"] is None or np.array_equal(wrong["rec"], plain["rec"], equal_nan=True)


def test_every_defect_is_shown_by_some_case(rows):
    seen = set()
    for c in S.PLAN_CASES:
        ev, op, N, R, A = S.plan_case(c, rows) if S.SIZES[c["size"]][0] < 5000 else (None, None, None, None, None)
        if ev is not None:
            seen |= S.shows(c, ev, op)
    assert seen == set(S.DEFECTS), set(S.DEFECTS) - seen


@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_rounded_seed_step_and_first_are_inside_their_bounds(size):
    N, R, A = S.SIZES[size]
    for sigma in (80.0, 0.5, 0.001):
        op = S.seed_operands(N)
        want, got, b = S.seed_ref(op, sigma, S.SD), S.seed_ref(op, sigma, S.SD, S.rounded), S.seed_bounds(op, sigma, S.SD)
        for k in ("D", "e", "dF"):
            assert S.outside(S.as_f32(got[k]), want[k], b[k]) is None, (size, sigma, k)
            assert S.outside(S.as_f32(got[k]) + np.float32(0.01), want[k], b[k]) is not None   # the bound is far below the values
    for bounded in (False, True):
        if bounded and N % A:
            continue
        op = S.step_operands(N, A, bounded)
        for sigma in (80.0, 2.0, 0.001):
            kw = dict(sigma=sigma, scale=float(S.host_scale(S.BETA, sigma, S.SD)))
            want, got = S.step_ref(op, A, **kw), S.step_ref(op, A, S.rounded, **kw)
            assert S.outside(S.as_f32(got), want, S.step_bound(op, **kw)) is None, (size, sigma, bounded)
        if bounded:
            col = np.arange(N) % A
            want = S.step_ref(op, A)
            assert (want <= op["hi"][col]).all()
            assert (want[col == 1 % A] == op["hi"][1 % A]).all()   # lo > hi gives hi
            moved = (want != S.step_ref(dict(op, lo=None, hi=None), A))[col != 1 % A]
            assert moved.any() and not moved.all()                  # elsewhere the clamp acts on some elements, not on all
    op = S.first_operands(N)
    for cn, with_row in ((0.7, True), (0.0, True), (0.7, False)):
        want, got = S.first_ref(op, cn, with_row), S.first_ref(op, cn, with_row, S.rounded)
        assert S.outside(S.as_f32(got), want, S.first_bound(op, cn, with_row)) is None
        if cn == 0.0 or not with_row:
            assert S.same_bits32(S.as_f32(got), op["x_T"])


def test_the_grids_capacity_is_the_kernels():
    import os
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mdt_policy_amd", "csrc", "mdt_steer.hip")
    with open(src) as f:
        text = f.read()
    assert "constexpr int STEER_THREADS = 256;" in text and "constexpr int STEER_MAX_BLOCKS = 1024;" in text
