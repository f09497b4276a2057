"""The sampler options on the configurations of tests/envelope_configs.ENVELOPE, CPU tier: on the float64 host loops of
tests/sampler_envelope.py alone, the conditions without which the comparisons of tests/test_gpu_sampler_envelope.py would be
vacuous, and the helper against the oracles that exist.  Every test prints the measured gap next to its threshold (pytest -s).

Measured with these loops (B = 3, schedule 80 -> 1 -> 0 in 4 steps, float64, over the nine configurations):

Pin, |pinned - unpinned| max on the keep == 1 elements against 100 x tol, and on the keep == 0 ones against 10 x tol:
    ddim       0.64 .. 3.60 against 0.025 .. 0.199;  0.220 .. 0.523 against 0.0129 .. 0.0204
    heun       0.64 .. 3.53 against 0.022 .. 0.199;  0.274 .. 0.642 against 0.0135 .. 0.0205
    dpmpp_2m   0.64 .. 3.59 against 0.025 .. 0.199;  0.222 .. 0.525 against 0.0129 .. 0.0204
    lms        0.64 .. 3.61 against 0.024 .. 0.202;  0.256 .. 0.610 against 0.0135 .. 0.0206
    dpmpp_sde  0.64 .. 3.71 against 0.042 .. 0.195;  0.243 .. 0.693 against 0.0133 .. 0.0177
    (3, 5) candidate rows, ddim / dpmpp_2m: 2.10 .. 3.80 against 0.097 .. 0.202;  0.255 .. 0.676 against 0.0136 .. 0.0207
    lambda = 2.5, heun / dpmpp_2m (guided tolerance): 0.88 .. 6.31 against 0.066 .. 0.361;  0.391 .. 1.287 against 0.0197 .. 0.0297
  The one exception is h1_d64_min on keep == 0: every sample is a single element, so a keep == 0 sample cannot feel the pin and the
  gap is exactly 0 under every kind.  There the condition is replaced by its opposite: the pinned result equals the unpinned one
  on those samples, bit for bit (on the GPU: batch independence).
  ddim and dpmpp_2m end with x' = D': their pinned elements are ``known`` bit for bit.  heun, lms and dpmpp_sde end with
  x' = x + sum c_j d_j and arrive to rounding (lms: 8e-9 in float64, the quadrature of its coefficients).
Bounds, the per-column 30 % / 70 % quantiles of the unclamped result of the same options, heun and lms, with a pin and without:
  the share of elements a clip_output call changes is at least 0.333 at every step (0.34 without h1_d64_min, whose three elements
  move in thirds); |clamped - unclamped| max 0.31 .. 1.91 against 100 x tol 0.043 .. 0.124.  The 15 % / 85 % quantiles the work
  started from missed the 10 % share in 8 of the 36 cases (down to 0.036 at mdt_h6_a12 lms step 2, and 0 at h1_d64_min with a
  pin), so the quantiles moved inward for every configuration, to the values tests/test_gpu_sampler_bounds.py uses.
Guidance, lambda = 2.5, heun and dpmpp_2m: |guided - unguided| max 0.56 .. 1.86 against 100 x tol 0.166 .. 0.379.
Steer, weights (1, 0.25, 0), beta = 5, 3-step DDIM 80 -> 0.01 -> 0: the weighted error falls by 6.8 x .. 13 x (a16_ctx16
  179.3 -> 18.6, h1_d64_min 1.55 -> 0.23, plain_ta16 115.3 -> 17.3); |steered - unsteered| max 1.16 .. 3.63 against 100 x the
  trajectory tolerance 0.73 .. 2.00.  With a last level of 1 instead of 0.01 plain_ta16 went 111.1 -> 118.4: see
  sampler_envelope.steered_ddim.  One evaluation: s |J^T e| max is 730 .. 6900 tolerances at sigma = 1, 8 .. 81 at sigma = 80.
Log-likelihood, (B, K) = (2, 3), sigma 0.001 .. 80, one sign probe: 74 evaluations in float64 (rope_ta16: 68); |ll| 0.06 .. 1.7
  at h1_d64_min (per = 1), 16 .. 147 elsewhere.
Steered plan samplers (mdt_sample_steer; tests/test_gpu_steer_plan_envelope.py), heun and dpmpp_2m on the nine configurations,
  lms (six steps) and dpmpp_sde on LL_NAMES, under steer_of: a 2^-23 relative perturbation of x_T moves the float64 loop by
  9.0e-7 .. 6.5e-4 of the gate (1 + beta) (ATOL + RTOL |want|) per element, against 1e-2; |steered - unsteered| max 0.98 .. 6.2
  against 100 x the gate 0.54 .. 3.0 (at least 1.27 x that).  Bounds at the 0.3 / 0.7 quantiles of the steered result, heun and
  dpm_2 on a16_ctx16 and mdt_h6_a12: clip_output changes 0.988 .. 0.992 of the elements at the first step, 0.38 .. 0.77 at the
  others; dpmpp_2m never calls it.
The whole module takes about a minute and a half at 8 threads.
"""
import pytest
import torch

from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from tests import sampler_envelope as E
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, inputs_of, load_fixture, params_of

B = 3


def guided_tol():
    """tests/test_gpu_guidance.tol(2.5) (that module is GPU-only: restated, and compared in the GPU tier)."""
    return dict(rtol=1e-3, atol=1e-4 * (abs(E.LAM) + abs(1 - E.LAM)))


def test_the_pattern_reaches_every_lane_and_value():
    for name in E.NAMES:
        Ta, A = E.shape_of(name)
        keep = E.pattern(B, Ta, A)
        assert keep.shape == (B, Ta, A) and set(keep.unique().tolist()) == {0.0, 0.5, 1.0}, name
        for c in range(A):  # every column of the action head meets all three values
            assert set(keep[:, :, c].unique().tolist()) == {0.0, 0.5, 1.0}, (name, c)
        assert float(keep[0, 0, 0]) == 1.0 and float(keep[1, 0, 0]) == 0.5 and float(keep[2, 0, 0]) == 0.0
    assert sorted(E.shape_of(n)[0] * E.shape_of(n)[1] for n in E.LL_NAMES) == [1, 70, 112, 112, 120, 160]
    assert E.GUIDED_NAMES == E.NAMES  # every configuration of the envelope carries a goal token


@pytest.mark.parametrize("kind", sorted(E.KINDS))
@pytest.mark.parametrize("name", E.NAMES)
def test_pin_changes_the_result_everywhere(name, kind):
    free, known, pinned = E.loops(name, kind, B)
    E.conditions(f"{name} {kind}", free, pinned, known, E.pattern(*free.shape), lone=E.is_lone(name))
    assert bool(torch.isfinite(pinned).all())
    if kind in ("ddim", "dpmpp_2m"):  # the last update is x' = D': the pinned elements are ``known`` (as float32) bit for bit
        hard = E.pattern(*free.shape) == 1
        assert torch.equal(pinned[hard], E.pin_of(name, kind, B).known.double()[hard])


@pytest.mark.parametrize("name", E.NAMES)
def test_pin_over_the_candidate_rows(name):
    """(B, K) = (3, 5): the pattern over the 15 chunk rows of the expanded observations."""
    for kind in ("ddim", "dpmpp_2m"):
        free, known, pinned = E.loops(name, kind, B, repeat=5)
        assert free.shape[0] == 15
        E.conditions(f"{name} {kind} K=5", free, pinned, known, E.pattern(*free.shape), lone=E.is_lone(name))


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("kind", ["heun", "lms"])
@pytest.mark.parametrize("name", E.NAMES)
def test_bounds_clip_at_every_step(name, kind, pinned):
    lo, hi, want, seen, changed, plain = E.bounded(name, kind, B, pinned)
    gap, tol = float((want - plain).abs().max()), E.tol_of(want)
    print(f"{name} {kind} pin={pinned}: clip_output changed {[round(c, 3) for c in changed]}; |clamped - unclamped| max {gap:.4f} "
          f"(100 tol {100 * tol:.4f})")
    assert len(changed) == E.N == len(seen)
    assert min(changed) >= 0.10, f"{name} {kind}: a clip_output call changed {min(changed):.3f} of the elements"
    assert gap > 100 * tol, f"{name} {kind}: clamped and unclamped differ by {gap:.3e} only"
    assert bool((want >= lo.double()).all()) and bool((want <= hi.double()).all())
    if pinned:  # the callback sees D': the pinned elements of every step's denoised value are ``known``
        known = E.loops(name, kind, B)[1]
        hard = E.pattern(*want.shape) == 1
        for _, den in seen:
            assert torch.equal(den[hard], E.pin_of(name, kind, B).known.double()[hard])
            assert_close(den[hard], known[hard], rtol=1e-6, atol=0)


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("name", E.GUIDED_NAMES)
def test_guidance_changes_the_result(name, kind):
    t = guided_tol()
    free, known, pinned = E.loops(name, kind, B, lam=E.LAM)
    plain = E.loops(name, kind, B)[0]
    gap, tol = float((free - plain).abs().max()), E.tol_of(free, t["atol"], t["rtol"])
    print(f"{name} {kind}: |guided - unguided| max {gap:.4f} (100 tol {100 * tol:.4f})")
    assert gap > 100 * tol, f"{name} {kind}: guided and unguided differ by {gap:.3e} only"
    E.conditions(f"{name} {kind} lambda={E.LAM}", free, pinned, known, E.pattern(*free.shape), atol=t["atol"], rtol=t["rtol"],
                 lone=E.is_lone(name))


@pytest.mark.parametrize("name", E.NAMES)
def test_steer_lowers_the_weighted_error(name):
    steered, plain = E.steered_ddim(name, B)
    steer = E.steer_of(name, B)
    e_steered, e_plain = E.werr(steer, steered), E.werr(steer, plain)
    gap, tol = float((steered - plain).abs().max()), (1 + E.BETA) * E.tol_of(steered)
    print(f"{name}: weighted error {e_plain:.4e} -> {e_steered:.4e}; |steered - unsteered| max {gap:.4f} (100 tol {100 * tol:.4f})")
    assert e_steered < e_plain, (e_steered, e_plain)
    assert gap > 100 * tol, f"{name}: steered and unsteered differ by {gap:.3e} only"
    assert set(steer.weight.unique().tolist()) == {0.0, 0.25, 1.0}


@pytest.mark.parametrize("name", E.NAMES)
def test_one_steered_evaluation_is_the_host_loops(name):
    """EnvelopeOracle's ``steer=`` (one evaluation, what the GPU tier compares with) is the D' the host loop forms around a
    foreign model (gc_sampling._SteeredModel), and the Jacobian term is not negligible."""
    model, steer = E.oracle_of(name), E.steer_of(name, B)
    state, goal, x, _, _ = E.chunk_case(name, B)
    state, goal = E.wide(state), E.wide(goal)
    for sigma in (80.0, E.SD * (E.BETA - 1) ** 0.5, 1.0):
        xs = (-steer.known.double() + sigma * x.double() / E.SMAX)
        sg = torch.full((B,), sigma, dtype=torch.float64)
        want, d, j = model.steered(state, xs, goal, sg, steer)
        got = gs._SteeredModel(model, steer)(state, xs, goal, sg)
        assert_close(model(state, xs, goal, sg, steer=steer), got, rtol=1e-12, atol=1e-12, what=f"{name} sigma={sigma}")
        share = float((steer.scale(sigma, E.SD) * j).abs().max()) / (ATOL + RTOL * float(d.abs().max()))
        print(f"{name} sigma={sigma:g}: s |J^T e| max / tol = {share:.1f}")
        assert share > 100 or sigma == 80.0, f"{name} sigma={sigma}: the steer moves D by {share:.2f} tolerances only"


@pytest.mark.parametrize("name", E.LL_NAMES)
def test_log_likelihood_reference(name, monkeypatch):
    ll, latent, delta, info = E.loglik_reference(name, monkeypatch)
    print(f"{name}: ll {[round(float(v), 3) for v in ll]}, fevals {info['fevals']}, |latent| max {float(latent.abs().max()):.2f}")
    assert ll.shape == (6,) and bool(torch.isfinite(ll).all()) and latent.shape[0] == 6
    assert info["fevals"] == 2 + 6 * info["steps"]
    # the candidates differ: the three chunks of an observation do not score alike
    assert float((ll.reshape(2, 3).max(1).values - ll.reshape(2, 3).min(1).values).min()) > 0.05 * 3


# ---- the helper against the oracles that exist -------------------------------------------------------------------------------
def test_envelope_oracle_pin_equals_the_action_pin_oracle():
    from tests.test_action_pin import OracleModel, keep_of
    meta, _ = load_fixture("g7_samplers.npz")
    state, goal, noise = inputs_of(dict(meta, B=2, input_seed=702), dtype=torch.float64)
    mine = E.EnvelopeOracle("g7", dict(cfg=cfg_of(meta), arch=meta["arch"]), params_of(meta))
    theirs = OracleModel(meta)
    known = torch.from_numpy(E.synthetic.normal("known", tuple(noise.shape), 3)).double()
    for pin in (None, ActionPin(known, keep_of(noise.shape[1])), ActionPin(known, E.pattern(*noise.shape))):
        for sigma in (80.0, 0.3):
            sg = torch.full((2,), sigma, dtype=torch.float64)
            a, b = mine(state, noise * sigma, goal, sg, pin=pin), theirs(state, noise * sigma, goal, sg, pin=pin)
            assert_close(a, b, rtol=1e-12, atol=1e-12, what=f"pin {pin} sigma {sigma}")
            assert_close(mine(state, noise * sigma, goal, sg, pin=pin), b, rtol=1e-12, atol=1e-12, what="kept context")


def test_envelope_oracle_guided_ddim_equals_the_guidance_oracle(monkeypatch):
    from tests import test_gpu_guidance as guid
    name, lam = "mdt_h6_a12", E.LAM
    monkeypatch.setitem(guid._MODELS, name, (None, E.params(name)))  # its weights without its device
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    want = guid.oracle_guided_ddim(name, B, E.SEED, sig, lam)
    state, goal, x, _ = E.case(name, B)
    with torch.no_grad():
        got = gs.sample_ddim(E.oracle_of(name), E.wide(state), x.double(), goal.double(), sig, extra_args={"cond_lambda": lam})
    # (the host loop forms its step scalars in float32, the guidance oracle in float64)
    assert_close(got, want, rtol=1e-5, atol=1e-6, what="guided DDIM")
    assert guid.tol(lam) == guided_tol()


# ---- the steered plan samplers: what tests/test_gpu_steer_plan_envelope.py relies on ----------------------------------------------
@pytest.mark.parametrize("name,kind", E.PLAN_CASES)
def test_steered_plan_loops_are_well_conditioned_and_moved_by_the_steer(name, kind):
    """The float64 steered loop moves by at most 1e-2 of the gate (1 + beta) (ATOL + RTOL |want|) under a 2^-23 relative
    perturbation of x_T -- an fp32 run of the same loop has room inside the gate -- and steered and unsteered differ by more than
    100 x the gate."""
    steered, plain = E.steered_plan(name, kind, B)
    moved = E.steered_plan(name, kind, B, x_scale=1.0 + 2.0 ** -23)
    share = float(((moved - steered).abs() / E.steer_gate(steered)).max())
    gap, tol = float((steered - plain).abs().max()), (1 + E.BETA) * E.tol_of(steered)
    print(f"{name} {kind}: a 2^-23 perturbation of x_T moves the result by {share:.2e} of the gate; |steered - unsteered| max "
          f"{gap:.4f} (100 tol {100 * tol:.4f}); weighted error {E.werr(E.steer_of(name, B), plain):.4e} -> "
          f"{E.werr(E.steer_of(name, B), steered):.4e}")
    assert bool(torch.isfinite(steered).all()) and steered.dtype == torch.float64
    assert share < 1e-2, f"{name} {kind}: the float64 loop itself moves by {share:.3e} of the gate"
    assert gap > 100 * tol, f"{name} {kind}: steered and unsteered differ by {gap:.3e} only"


@pytest.mark.parametrize("tag", sorted(E.NOISE_KINDS))
def test_the_noise_kinds_read_noise_rows_and_record_every_step(tag):
    kind, params, n, sig, plan = E.noise_plan(tag)
    coef = [abs(plan.e[k].cx[8 + j]) + abs(plan.e[k].cy[8 + j]) for k in range(plan.n_evals) for j in range(2) if plan.e[k].noise[j] >= 0]
    assert plan.n_noise > 0 and (any(c > 0 for c in coef) or (plan.y0_noise >= 0 and plan.y0_cn != 0)), (tag, plan.n_noise)
    steps = [plan.e[k].step for k in range(plan.n_evals) if plan.e[k].begins_step]
    assert steps == list(range(len(steps))) and len(steps) >= 2


@pytest.mark.parametrize("kind", sorted(E.CLIP_KINDS))
@pytest.mark.parametrize("name", E.CLIP_NAMES)
def test_steered_bounds_clip_a_share_of_the_elements_at_every_step(name, kind):
    """Every clip_output call of the float64 steered loop changes between 0.1 and 0.9 of the elements -- but the first, which
    changes nearly all and is held to that: after the first step x is still N(0, sigma_1^2)-sized, sigma_1 = 80^(2/3) = 18.6,
    while lo and hi are quantiles of the final result, less than 2 apart, so an element stays inside with probability about
    (hi - lo) / (sigma_1 sqrt(2 pi)) < 0.05.  (Measured: 0.988 .. 0.992 at the first step, 0.38 .. 0.77 at the others.)"""
    lo, hi, want, changed, plain = E.steered_bounded(name, kind, B)
    print(f"{name} steered {kind}: clip_output changed {[round(c, 3) for c in changed]}; |clamped - unclamped| max "
          f"{float((want - plain).abs().max()):.4f}")
    assert float((hi - lo).max()) < 2.0 and float(E.sched()[1]) > 18.0
    assert len(changed) == E.N and 0.1 <= min(changed) and max(changed[1:]) <= 0.9 and 0.95 <= changed[0] < 1.0, changed
    assert bool((want >= lo.double()).all()) and bool((want <= hi.double()).all())


@pytest.mark.parametrize("name", E.CLIP_NAMES)
def test_steered_dpmpp_2m_never_reads_its_scaler(name):
    lo, hi, want, changed, plain = E.steered_bounded(name, "dpmpp_2m", B)
    assert changed == [] and torch.equal(want, plain)
    assert int(((plain < lo.double()) | (plain > hi.double())).sum()) > 0
