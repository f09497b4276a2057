"""Every steered sampler as one native call (include/mdt_hip_train.h mdt_sample_steer; GCDenoiser.sample_steered(kind=...);
through gc_sampling with a steer built with ``plan_native=True``, as every steer of this file is):
the native call against the host loop over ``GCDenoiser.forward(..., steer=)`` it replaces (a no-op ``callback`` forces that
loop and proves it ran), ten steps against the float64 loop that gc_sampling itself runs over the oracle as a foreign model,
the weighted error steering is for, bounds where the loops clip, the per-step record, and what the call promises about itself.

Tolerances.  Native against host loop: helpers.RTOL / ATOL -- both sides run the same taped decoder forward and the same
backward, and differ in the encoder's kernels (last place) and in the order of the update's fp32 operations.  That gate is
absolute (1e-4) where the result is small, so the 3-4 step schedules of those tests run from SMAX = 2 to SMIN = 0.05, not from
80 to 0.001: a second-order step forms its intermediate input as x + (sigma' - sigma) d with |x| up to 4 sigma_max, a
cancellation that leaves one spacing of x (3e-5 at 280, 1e-6 at 8) between two orders of the same operations, and the step's
second evaluation multiplies it by (sigma - sigma') / sigma_mid -- 21 (heun) to 45 (dpm_2_ancestral) on the first of four steps
from 80 to 0.001, where the unsteered native call and its host loop differ by 1.6e-3 on these inputs too (measured, MI355X),
against at most 3.4 per step from 2 to 0.05, 4e-5 over three steps.  [SMIN, SMAX] holds both branches of
s(sigma) = min(beta, 1 + sigma^2 / sigma_d^2): clipped at 2, free below 1.  The float64 runs keep the fixtures' 80 .. 0.001 over
ten steps.  Against float64: (1 + beta) (RTOL, ATOL), the project's
gate for steered trajectories (tests/test_gpu_steer.py).  The weighted error E = sum W (known - out)^2: with t the per-element
gate of out, |E_native - E_oracle| <= sum W (2 |known - out| t + t^2)."""
import functools
import warnings

import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_bounds import ActionBounds
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests.helpers import ATOL, RTOL, assert_close
from tests.test_gpu_steer import BETA, SD, noise, setup, take, werr
from tests.test_log_likelihood import OracleModel, to_cuda

pytestmark = pytest.mark.gpu

# name -> (gc_sampling's sample_<kind>, its keyword arguments; "fixed": a noise_sampler that returns one fixed tensor)
KINDS = {
    "euler_churn": ("euler", dict(s_churn=1.0)),
    "heun": ("heun", {}),
    "heun_churn": ("heun", dict(s_churn=1.0, s_noise=0.9)),
    "dpm_2": ("dpm_2", {}),
    "lms_1": ("lms", dict(order=1)),
    "lms_4": ("lms", dict(order=4)),
    "dpmpp_2m": ("dpmpp_2m", {}),
    "euler_ancestral": ("euler_ancestral", {}),
    "dpm_2_ancestral": ("dpm_2_ancestral", {}),
    "dpmpp_2s_ancestral": ("dpmpp_2s_ancestral", {}),
    "dpmpp_sde_fixed": ("dpmpp_sde", dict(noise_sampler="fixed")),
    "dpmpp_sde_tree": ("dpmpp_sde", {}),
    "dpm_fast_4": ("dpm_fast", dict(n=4)),
    "dpm_fast_6": ("dpm_fast", dict(n=6)),
}


def hard_steer(action, hard=3, soft=0, executed=2):
    """tests/test_gpu_steer.hard_steer -- the receding-horizon steer of a replan, the previous chunk the fixture's action chunk --
    asking for the native plan call."""
    return ActionSteer.overlap(action, executed, hard, soft, plan_native=True)


def run(kind, model, state, x, goal, sigmas, extra_args, seed=7, **kw):
    """One gc_sampling call of ``kind`` from a fixed seed (the loops' and the native routes' draws come from torch's generator)."""
    kw = dict(kw)
    if kw.get("noise_sampler") == "fixed":
        fixed = noise(tuple(x.shape), 61, "steer_plan_sde").to(x.device)
        kw["noise_sampler"] = lambda s0, s1: fixed
    torch.manual_seed(seed)
    if kind == "dpm_fast":
        smin, smax = float(sigmas[-2]), float(sigmas[0])
        return gs.sample_dpm_fast(model, state, x, goal, smin, smax, kw.pop("n"), extra_args=extra_args, **kw)
    return getattr(gs, "sample_" + kind)(model, state, x, goal, sigmas, extra_args=extra_args, **kw)


def both_ways(kind, model, state, x, goal, sigmas, extra_args, **kw):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    calls, steered = [], GCDenoiser._steered
    GCDenoiser._steered = lambda self, *a, **k: calls.append(1) or steered(self, *a, **k)
    try:
        native = run(kind, model, state, x, goal, sigmas, extra_args, **kw)
        assert not calls  # one native call: no evaluation went through forward(steer=)
        seen = []
        host = run(kind, model, state, x, goal, sigmas, extra_args, callback=lambda d: seen.append(d["i"]), **kw)
        assert calls
    finally:
        GCDenoiser._steered = steered
    assert seen and seen == list(range(len(seen)))  # the host loop ran
    return native, host


SMIN, SMAX = 0.05, 2.0  # the short schedules' range (the module's docstring)


def inputs(name, B, K, seed, steps=4):
    meta, cfg, model, state, goal, action = setup(name)
    B = min(B, action.shape[0])
    x = (SMAX * noise((B * K,) + tuple(action.shape[1:]), seed)).cuda()
    return model, to_cuda(take(state, B)), goal[:B].cuda(), action[:B], x, gs.get_sigmas_exponential(steps, SMIN, SMAX)


# ----------------------------------------------------------------------------------------------------------------
# the native call against the host loop over forward
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (2, 40)])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_native_matches_the_host_loop(name, B, K):
    """R = 1: one row, 70 elements in two waves; R = 15: 1050 elements and 15 sigma entries, five workgroups with a ragged last
    one; R = 80 is past the 32-sample attention threshold, with a per-observation steer expanded by ``on``."""
    kind, kw = KINDS[name]
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", B, K, 71, steps=3 if "sde" in name else 4)
    if K == 5:  # per chunk: every chunk its own known part
        prev = action.repeat_interleave(K, 0) + 0.1 * noise(tuple(x.shape), 72)
        steer = hard_steer(prev, hard=2, soft=3)
    else:       # per observation
        steer = hard_steer(action, hard=3, soft=2)
    x_before = x.clone()
    native, host = both_ways(kind, model, st, x, g, sigmas, {"steer": steer, "candidates": K}, **kw)
    plain = run(kind, model, st, x, g, sigmas, {"candidates": K}, **kw)
    print(f"{name} B={B} K={K}: max |native - host| {float((native - host).abs().max()):.3e} (max |host| "
          f"{float(host.abs().max()):.3e}), max |steered - plain| {float((native - plain).abs().max()):.3e}")
    assert torch.equal(x, x_before)  # x_T is only read
    assert native.shape == x.shape
    assert_close(native.cpu(), host.cpu(), what=f"{name}: native against the host loop")
    assert not torch.equal(native, plain)  # ... and the steer moved the chunk


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("config,B,K", [("mdt_tiny", 2, 3), ("mdtv_no_ada", 2, 3), ("mdtv_noise_block", 2, 1)])
def test_native_matches_the_host_loop_on_the_other_configurations(config, B, K, name):
    """MDT (two state tokens); use_ada_conditioning=False, where sigma is a context token and the context is encoded again before
    every evaluation; the NoiseBlock decoder."""
    kind, kw = KINDS[name]
    model, st, g, action, x, sigmas = inputs(config, B, K, 73, steps=3)
    steer = hard_steer(action, hard=3, soft=2)
    native, host = both_ways(kind, model, st, x, g, sigmas, {"steer": steer, "candidates": K}, **kw)
    print(f"{config} {name}: max |native - host| {float((native - host).abs().max()):.3e}")
    assert_close(native.cpu(), host.cpu(), what=f"{config} {name}: native against the host loop")


@pytest.mark.parametrize("family,config", [("long_chunk", "adaln_ta24"), ("wide_action", "a17")])
def test_native_heun_matches_the_host_loop_at_other_chunk_sizes(family, config):
    """Ta = 24 (168 elements per chunk) and A = 17 (170): Ta * A is not the 70 the steer kernels were first run at."""
    import importlib
    T = importlib.import_module(f"tests.test_gpu_{family}_options")
    state, goal, x, _ = T.case(config)
    x = x * (SMAX / T.E.SMAX)  # x_T = SMAX noise
    model = T.model_of(config)
    known = 0.5 * noise(tuple(x.shape), 74)
    steer = ActionSteer(known, torch.tensor([1.0, 1.0, 0.5, 0.25] + [0.0] * (x.shape[1] - 4)), plan_native=True)
    sigmas = gs.get_sigmas_exponential(3, SMIN, SMAX)
    native, host = both_ways("heun", model, T.cuda(state), x.cuda(), goal.cuda(), sigmas, {"steer": steer})
    print(f"{config} (Ta, A) = {tuple(x.shape[1:])}: max |native - host| {float((native - host).abs().max()):.3e}")
    assert_close(native.cpu(), host.cpu(), what=f"{config}: native heun against the host loop")


# ----------------------------------------------------------------------------------------------------------------
# ten steps against float64, and what steering is for
# ----------------------------------------------------------------------------------------------------------------
ORACLE_KINDS = {"heun": {}, "dpmpp_2m": {}, "lms": {}, "dpmpp_sde": dict(noise_sampler="fixed")}


def trajectory_inputs(B=3, n=10):
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    x = meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 41)
    return meta, cfg, model, take(state, B), goal[:B], action[:B], x, gs.get_sigmas_exponential(n, meta["sigma_min"], meta["sigma_max"])


@functools.lru_cache(maxsize=None)
def oracle_trajectory(kind, steered: bool):
    """Ten steps of gc_sampling's own loop in float64 over the oracle, a foreign model: gc_sampling steers it through autograd."""
    meta, cfg, _, st, g, action, x, sigmas = trajectory_inputs()
    ref = OracleModel(meta, cfg, torch.float64)
    ref.sigma_data = SD  # what _SteeredModel reads s(sigma) with
    ea = {"steer": hard_steer(action)} if steered else None
    return run(kind, ref, st, x.double(), g, sigmas, ea, **ORACLE_KINDS[kind])


def native_trajectory(kind, steered: bool):
    meta, cfg, model, st, g, action, x, sigmas = trajectory_inputs()
    ea = {"steer": hard_steer(action)} if steered else None
    return run(kind, model, to_cuda(st), x.cuda(), g.cuda(), sigmas, ea, **ORACLE_KINDS[kind]).cpu()


@pytest.mark.parametrize("kind", sorted(ORACLE_KINDS))
def test_ten_steps_against_the_float64_loop_over_the_oracle(kind):
    """Measured on MI355X (mdtv_tiny, B = 3, 10 steps): see DESIGN.md 4.3i."""
    want, got = oracle_trajectory(kind, True), native_trajectory(kind, True)
    err = (got.double() - want).abs()
    tol = (1 + BETA) * (ATOL + RTOL * want.abs())
    print(f"{kind}: max |native - oracle| {float(err.max()):.3e} (|oracle| max {float(want.abs().max()):.3e}), "
          f"largest err / bound {float((err / tol).max()):.3f}")
    assert_close(got, want, rtol=(1 + BETA) * RTOL, atol=(1 + BETA) * ATOL, what=f"steered {kind} against the oracle")


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
def test_steering_lowers_the_weighted_error(kind):
    meta, cfg, model, st, g, action, x, sigmas = trajectory_inputs()
    steer = hard_steer(action)  # weight 1 on the first three tokens
    # first on the oracle alone: the chosen inputs have the property at all
    o_steered, o_plain = oracle_trajectory(kind, True), oracle_trajectory(kind, False)
    assert werr(steer, o_steered) < werr(steer, o_plain), (werr(steer, o_steered), werr(steer, o_plain))
    n_steered, n_plain = native_trajectory(kind, True), native_trajectory(kind, False)
    known, w = steer.on("cpu", tuple(o_steered.shape))
    t = (1 + BETA) * (ATOL + RTOL * o_steered.abs())
    bound = float((w.double() * (2 * (known.double() - o_steered).abs() * t + t * t)).sum())
    print(f"{kind} weighted error: oracle {werr(steer, o_plain):.4e} -> {werr(steer, o_steered):.4e}, native "
          f"{werr(steer, n_plain):.4e} -> {werr(steer, n_steered):.4e}; |native - oracle| "
          f"{abs(werr(steer, n_steered) - werr(steer, o_steered)):.3e}, bound {bound:.3e}")
    assert abs(werr(steer, n_steered) - werr(steer, o_steered)) <= bound
    assert werr(steer, n_steered) < werr(steer, n_plain), (werr(steer, n_steered), werr(steer, n_plain))


# ----------------------------------------------------------------------------------------------------------------
# bounds, the record
# ----------------------------------------------------------------------------------------------------------------
def tight_bounds(free, A):
    """Bounds that bind on the result itself (and far inside the sigma-sized states of the early steps): its 20 % and 80 % points."""
    lo = torch.tensor([float(free.quantile(0.2))] * A)
    hi = torch.tensor([float(free.quantile(0.8))] * A)
    return lo, hi, ActionBounds(lo.tolist(), hi.tolist())


def test_heuns_bounds_clamp_where_the_host_loops_scaler_clamps():
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", 3, 1, 75, steps=4)
    steer = hard_steer(action, hard=3, soft=2)
    free = run("heun", model, st, x, g, sigmas, {"steer": steer})
    lo, hi, scaler = tight_bounds(free, x.shape[2])
    native, host = both_ways("heun", model, st, x, g, sigmas, {"steer": steer}, scaler=scaler)
    at_lo, at_hi = int((native.cpu() == lo).sum()), int((native.cpu() == hi).sum())
    print(f"heun bounds [{float(lo[0]):.4f}, {float(hi[0]):.4f}]: max |native - host| {float((native - host).abs().max()):.3e}, "
          f"{at_lo} at lo, {at_hi} at hi")
    assert_close(native.cpu(), host.cpu(), what="clamped native heun against the host loop")
    assert bool((native.cpu() >= lo).all()) and bool((native.cpu() <= hi).all()) and not torch.equal(native, free)
    assert at_lo > 0 and at_hi > 0  # the clamp acted on the last step too


@pytest.mark.parametrize("name", ["dpmpp_2m", "dpm_fast_6"])
def test_bounds_are_accepted_and_not_applied_where_the_loop_never_reads_its_scaler(name):
    kind, kw = KINDS[name]
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", 3, 1, 76, steps=4)
    steer = hard_steer(action, hard=3, soft=2)
    free = run(kind, model, st, x, g, sigmas, {"steer": steer}, **kw)
    lo, hi, scaler = tight_bounds(free, x.shape[2])
    native, host = both_ways(kind, model, st, x, g, sigmas, {"steer": steer}, scaler=scaler, **kw)
    outside = int(((native.cpu() < lo) | (native.cpu() > hi)).sum())
    print(f"{name}: {outside} elements outside [{float(lo[0]):.4f}, {float(hi[0]):.4f}]")
    assert_close(native.cpu(), host.cpu(), what=f"{name} under a scaler against the host loop")
    assert torch.equal(native, free) and outside > 0  # a clamp would have moved these


def test_the_record_is_what_the_host_loops_callback_saw():
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", 3, 2, 77, steps=4)
    steer = hard_steer(action, hard=3, soft=2)
    params = dict(s_churn=1.0, s_noise=0.9)
    seen = []
    torch.manual_seed(9)
    host = gs.sample_heun(model, st, x, g, sigmas, extra_args={"steer": steer, "candidates": 2},
                          callback=lambda d: seen.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in d.items()}), **params)
    torch.manual_seed(9)
    rows = gs._randn_rows(x, len(sigmas) - 1)
    out, rec = model.sample_steered(st, x, g, sigmas, steer, candidates=2, kind="heun", noise=rows, record=True, **params)
    replayed = []
    gs.replay_callback(rec, replayed.append)
    plain_rec = model.sample_native("heun", st, x, g, sigmas, noise=rows, candidates=2, record=True, **params)[1]
    assert len(replayed) == len(seen) == len(sigmas) - 1
    for a, b in zip(replayed, seen):
        assert a["i"] == b["i"]
        assert float(a["sigma"]) == float(b["sigma"]) and float(a["sigma_hat"]) == pytest.approx(float(b["sigma_hat"]), rel=1e-6)
        assert_close(a["x"].cpu(), b["x"].cpu(), what=f"step {a['i']}: x")
        assert_close(a["denoised"].cpu(), b["denoised"].cpu(), what=f"step {a['i']}: D'")
    assert not torch.equal(rec["denoised"][0], plain_rec["denoised"][0])  # D', not D
    assert_close(out.cpu(), host.cpu(), what="recorded call against the host loop")
    torch.manual_seed(9)
    assert torch.equal(out, gs.sample_heun(model, st, x, g, sigmas, extra_args={"steer": steer, "candidates": 2}, **params))


# ----------------------------------------------------------------------------------------------------------------
# invariants
# ----------------------------------------------------------------------------------------------------------------
def test_an_all_zero_weight_gives_the_plain_calls_bits_and_identical_calls_identical_bits():
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", 3, 2, 78, steps=4)
    zero = ActionSteer(action, torch.zeros(action.shape[1]), plan_native=True)
    steer = hard_steer(action, hard=3, soft=2)
    for name in ("heun_churn", "dpmpp_2m", "euler_ancestral"):
        kind, kw = KINDS[name]
        plain = run(kind, model, st, x, g, sigmas, {"candidates": 2}, **kw)
        assert torch.equal(run(kind, model, st, x, g, sigmas, {"steer": zero, "candidates": 2}, **kw), plain), name
        x_before = x.clone()
        a = run(kind, model, st, x, g, sigmas, {"steer": steer, "candidates": 2}, **kw)
        b = run(kind, model, st, x, g, sigmas, {"steer": steer, "candidates": 2}, **kw)
        assert torch.equal(a, b) and not torch.equal(a, plain), name
        assert torch.equal(x, x_before), name
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == 3  # the observations' context


def test_a_capturing_stream_is_refused_and_nothing_is_enqueued():
    model, st, g, action, x, sigmas = inputs("mdtv_tiny", 2, 1, 79, steps=3)
    known, weight = hard_steer(action).on("cuda", tuple(x.shape))
    steer = ActionSteer(known, weight)  # on the device in the call's shape: ``on`` has nothing to launch
    before = model.sample_steered(st, x, g, sigmas, steer, kind="heun")  # (parameters uploaded, buffers grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            with pytest.raises(_lib.MDTHipError) as err:
                model.sample_steered(st, x, g, sigmas, steer, kind="heun")
    assert err.value.status == 5 and "mdt_sample_steer" in str(err.value) and "captured" in str(err.value)  # MDT_ERR_STATE
    assert any("Graph is empty" in str(w.message) for w in seen), [str(w.message) for w in seen]
    torch.cuda.synchronize()
    assert torch.equal(model.sample_steered(st, x, g, sigmas, steer, kind="heun"), before)  # the handle is as it was


def test_log_likelihood_and_steered_ddim_have_the_same_bits_before_and_after_a_steered_heun_call():
    """The call borrows mdt_log_likelihood's tapes and backward scratch and shares mdt_sample_ddim_steer's workspace: it hands
    them back as it found them."""
    from tests.test_gpu_loglik_native import signs, tiny
    meta, fx, model, state, goal, action = tiny()
    B = 2
    st, g, rows = take(state, B), goal[:B], action[:B].cuda()
    v = signs((1, B) + tuple(rows.shape[1:]), 12).cuda()
    steer = hard_steer(action[:3], hard=3, soft=2)
    sigmas = gs.get_sigmas_exponential(4, meta["sigma_min"], meta["sigma_max"])
    x2 = (meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 80)).cuda()
    ll_before = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    ddim_before = model.sample_ddim(st, x2, g, sigmas, steer=hard_steer(action[:B]))
    x = (meta["sigma_max"] * noise((3 * 4,) + tuple(action.shape[1:]), 81)).cuda()
    for _ in range(2):  # (more rows than either call: the tapes, the scratch and the workspace grow in between)
        out = model.sample_steered(take(state, 3), x, goal[:3], sigmas, steer, candidates=4, kind="heun")
    assert bool(torch.isfinite(out).all())
    ll_after = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    assert ll_after[3] == ll_before[3] and all(torch.equal(a, b) for a, b in zip(ll_after[:3], ll_before[:3]))
    assert torch.equal(model.sample_ddim(st, x2, g, sigmas, steer=hard_steer(action[:B])), ddim_before)
