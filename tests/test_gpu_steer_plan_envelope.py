"""Every steered plan sampler as one native call (mdt_sample_steer) on the configurations of tests/envelope_configs.ENVELOPE and on
the 17-64 families' largest shapes, on the MI355X (pytest -m gpu), against float64 references that share no kernel with it:

  a  the kinds without noise rows -- heun, dpmpp_2m on all nine configurations, lms (order 4, six steps) and dpmpp_sde (eta 1, one
     fixed noise tensor) on LL_NAMES -- against gc_sampling's own loop over EnvelopeOracle, a foreign model it steers through
     torch.autograd;
  b  the kinds that read noise rows, with the per-step record and (B, K) = (2, 3) candidates under a per-chunk steer, against the
     float64 plan interpreter (tests/steer_ops_cases.apply_plan, the host loop by tests/test_native_sampler_plan.py) over the plan
     of _lib.sampler_plan with D' from EnvelopeOracle.steered;
  c  bounds at the 0.3 / 0.7 column quantiles of the float64 unclamped steered result: heun and dpm_2 clip after every step,
     dpmpp_2m never reads them;
  d  a Ta = 64 chunk, an A = 64 action, a 64-token context and ctx64_ta64_hd64, with each family's own case / model_of /
     oracle_of, heun and dpmpp_2m, (B, K) = (2, 2), three steps of the families' steered-DDIM schedule.

Gate: (1 + beta) (RTOL, ATOL) per element, the project's gate for steered trajectories (tests/test_gpu_steer.py).  The conditions
that keep a comparison from being vacuous -- the float64 loop moves by less than 1e-2 of the gate under a 2^-23 perturbation of
x_T, steered and unsteered differ by more than 100 gates, the clamp changes a share of the elements at every step -- are asserted
on the float64 loops alone in tests/test_sampler_envelope.py.  The float64 loops are computed once per (configuration, kind).

Measured on the MI355X: see DESIGN.md 4.3i."""
import pytest
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import sampler_envelope as E
from tests.helpers import ATOL, RTOL, assert_close
from tests.test_gpu_sampler_envelope import cuda, gpu_case

pytestmark = pytest.mark.gpu
B = 3
GATE = dict(rtol=(1 + E.BETA) * RTOL, atol=(1 + E.BETA) * ATOL)


def share_of_gate(got, want):
    return float(((got.double() - want).abs() / E.steer_gate(want)).max())


# ---- a: the noise-free kinds against gc_sampling's own float64 loop --------------------------------------------------------------
@pytest.mark.parametrize("name,kind", E.PLAN_CASES)
def test_noise_free_kinds_against_the_float64_loop(name, kind):
    want, unsteered = E.steered_plan(name, kind, B)
    steer = E.steer_of(name, B)
    assert float((want - unsteered).abs().max()) > 100 * (1 + E.BETA) * E.tol_of(want), f"{name} {kind}: the steer changes too little"
    model, state, goal, x, fixed = gpu_case(name, B)
    with E.never_forward_steered() as seen:
        got = E.run_plan_loop(kind, model, state, x, goal, fixed, E.plan_sched(kind), {"steer": E.native_steer(steer)},
                              **E.PLAN_KINDS[kind][0]).cpu()
    assert not seen.calls, f"{name} {kind}: the call went through forward(steer=), not through mdt_sample_steer"
    e_got, e_want = E.werr(steer, got), E.werr(steer, want)
    print(f"{name} {kind}: max |native - float64| {float((got.double() - want).abs().max()):.3e} (|want| max "
          f"{float(want.abs().max()):.3f}), largest err / gate {share_of_gate(got, want):.3f}; weighted error native {e_got:.4e}, "
          f"float64 {e_want:.4e}, bound on the difference {E.werr_bound(steer, want):.3e}")
    assert_close(got, want, what=f"{name}: steered {kind}", **GATE)
    assert abs(e_got - e_want) <= E.werr_bound(steer, want)


# ---- b: the kinds that read noise rows, the record, candidates -------------------------------------------------------------------
def interpreted_case(name, tag, batch, K):
    want, begins, rows, steer = E.interpreted(name, tag, batch, K)
    kind, params, n, sig, plan = E.noise_plan(tag)
    model, state, goal, x, _ = gpu_case(name, batch, repeat=K)
    assert x.shape[0] == batch * K and goal.shape[0] == batch and rows.shape == (plan.n_noise,) + tuple(x.shape)
    with E.never_forward_steered() as seen:
        out, rec = model.sample_steered(state, x, goal, torch.tensor(sig), steer, kind=kind, noise=rows.cuda(), n_steps=n, record=True,
                                        candidates=K, **params)
    assert not seen.calls
    what = f"{name} {tag} (B, K) = ({batch}, {K})"
    print(f"{what}: max |native - float64| {float((out.cpu().double() - want).abs().max()):.3e} (|want| max "
          f"{float(want.abs().max()):.3f}), largest err / gate {share_of_gate(out.cpu(), want):.3f}; record: "
          f"{max(share_of_gate(rec['denoised'][s].cpu(), d) for s, _, d in begins):.3f} of the gate on D'")
    assert rec["x"].shape == rec["denoised"].shape == (len(begins),) + tuple(x.shape)
    for step, y, dp in begins:
        assert_close(rec["x"][step].cpu(), y, what=f"{what}: the record's x[{step}]", **GATE)
        assert_close(rec["denoised"][step].cpu(), dp, what=f"{what}: the record's denoised[{step}] (D')", **GATE)
    assert_close(out.cpu(), want, what=what, **GATE)
    return model


@pytest.mark.parametrize("tag", sorted(E.NOISE_KINDS))
@pytest.mark.parametrize("name", E.NOISE_NAMES)
def test_noise_kinds_and_their_record_against_the_plan_interpreter(name, tag):
    interpreted_case(name, tag, B, 1)


@pytest.mark.parametrize("name", E.NOISE_NAMES)
def test_candidates_with_a_per_chunk_steer_against_the_expanded_interpreter(name):
    model = interpreted_case(name, "heun_churn", 2, 3)
    steer = E.interpreted(name, "heun_churn", 2, 3)[3]
    assert not torch.equal(steer.known[0], steer.known[1])                        # chunks of one observation, different known parts
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == 2              # one context per observation


# ---- c: bounds -------------------------------------------------------------------------------------------------------------------
def native_bounded(name, kind, lo, hi, params):
    model, state, goal, x, fixed = gpu_case(name, B)
    steer = E.steer_of(name, B)
    with E.never_forward_steered() as seen:
        got = model.sample_steered(state, x, goal, E.plan_sched(kind), steer, kind=kind, bounds=(lo, hi), **params).cpu()
        free = model.sample_steered(state, x, goal, E.plan_sched(kind), steer, kind=kind, **params).cpu()
    assert not seen.calls
    return got, free


@pytest.mark.parametrize("kind", sorted(E.CLIP_KINDS))
@pytest.mark.parametrize("name", E.CLIP_NAMES)
def test_bounds_clamp_where_the_float64_loops_scaler_clamps(name, kind):
    lo, hi, want, changed, plain = E.steered_bounded(name, kind, B)
    assert len(changed) == E.N and min(changed) >= 0.1, changed
    got, free = native_bounded(name, kind, lo, hi, E.CLIP_KINDS[kind])
    print(f"{name} steered {kind} in bounds: max |native - float64| {float((got.double() - want).abs().max()):.3e}, largest err / gate "
          f"{share_of_gate(got, want):.3f}; {int((got == lo).sum())} at lo, {int((got == hi).sum())} at hi")
    assert bool((got >= lo).all()) and bool((got <= hi).all()), f"{name} {kind}: outside [lo, hi]"
    assert int((got == lo).sum()) > 0 and int((got == hi).sum()) > 0 and not torch.equal(got, free)
    assert_close(got, want, what=f"{name}: clamped steered {kind}", **GATE)


@pytest.mark.parametrize("name", E.CLIP_NAMES)
def test_dpmpp_2m_accepts_bounds_and_never_applies_them(name):
    lo, hi, want, changed, plain = E.steered_bounded(name, "dpmpp_2m", B)
    got, free = native_bounded(name, "dpmpp_2m", lo, hi, {})
    outside = int(((got < lo) | (got > hi)).sum())
    print(f"{name} steered dpmpp_2m under bounds: {outside} elements outside")
    assert torch.equal(got, free) and outside > 0
    assert_close(got, want, what=f"{name}: steered dpmpp_2m under a scaler", **GATE)


# ---- d: the 17-64 families -------------------------------------------------------------------------------------------------------
def family(which):
    """(the family's option module, configuration): its own case / model_of / oracle_of on the family's largest shape.  The
    long-chunk module builds its configurations from a table of overrides; the Ta = 64 row is put into that table here (its
    parametrised tests have read the table's names already)."""
    import importlib
    module, name = {"ta64": ("long_chunk", "ta64"), "a64": ("wide_action", "a64_ta24_rope_hd64"),
                    "ctx64": ("long_context", "ctx64_rope_hd32"), "ctx64_ta64": ("long_context", "ctx64_ta64_hd64")}[which]
    T = importlib.import_module(f"tests.test_gpu_{module}_options")
    if which == "ta64":
        T.OPTION_CASES.setdefault(name, dict(T._SMALL, action_seq_len=64))
    return T, name


_FAMILY = {}


def family_loops(which, kind):
    """(state, goal, x_T of the B * K rows, steer, schedule, float64 steered loop on the expanded observations), computed once."""
    if (which, kind) not in _FAMILY:
        T, name = family(which)
        Bf, K = 2, 2
        state, goal, _, _ = T.case(name, Bf)
        _, _, x, _ = T.case(name, Bf * K)
        known = 0.5 * torch.from_numpy(synthetic.normal("steer_plan_family", (Bf,) + tuple(x.shape[1:]), 37))
        steer = ActionSteer(known, E.pattern(*known.shape, values=(1.0, 0.25, 0.0)), E.BETA)
        sig = gs.get_sigmas_exponential(3, E.STEER_SMIN, E.SMAX)
        st = {k: (v.repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
        wide_steer = ActionSteer(known.repeat_interleave(K, 0), steer.weight.repeat_interleave(K, 0), E.BETA)
        want = E.run_plan_loop(kind, T.oracle_of(name), E.wide(st), E.wide(x), E.wide(goal.repeat_interleave(K, 0)), None, sig,
                               {"steer": wide_steer}, **E.PLAN_KINDS[kind][0])
        _FAMILY[(which, kind)] = (state, goal, x, steer, sig, want)
    return _FAMILY[(which, kind)]


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("which", ["ta64", "a64", "ctx64", "ctx64_ta64"])
def test_the_families_largest_shapes_against_the_float64_loop(which, kind):
    """Where k_head_wide's twin of the plan update (A = 64) and the prefix cross-attention backward (64-token context) meet the steer."""
    T, name = family(which)
    state, goal, x, steer, sig, want = family_loops(which, kind)
    K = x.shape[0] // goal.shape[0]
    model = T.model_of(name)
    with E.never_forward_steered() as seen:
        got = E.run_plan_loop(kind, model, cuda(state), x.cuda(), goal.cuda(), None, sig,
                              {"steer": E.native_steer(steer), "candidates": K}, **E.PLAN_KINDS[kind][0]).cpu()
    assert not seen.calls
    print(f"{name} (Ta, A) = {tuple(x.shape[1:])} {kind}: max |native - float64| {float((got.double() - want).abs().max()):.3e} "
          f"(|want| max {float(want.abs().max()):.3f}), largest err / gate {share_of_gate(got, want):.3f}")
    assert 64 in tuple(x.shape[1:]) or "ctx64" in name
    assert_close(got, want, what=f"{name}: steered {kind}", **GATE)
