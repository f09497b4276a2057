"""Steered sampling on the GPU (utils/action_steer.py; include/mdt_hip_train.h mdt_sample_ddim_steer): one evaluation of
``GCDenoiser.forward(..., steer=)`` against float64 autograd through the oracle, the native call against the host loop over
``forward`` it replaces (a no-op ``callback`` forces that loop), a 10-step trajectory against a float64 loop over the oracle,
and what the call promises about itself: a lower weighted error, no steer for an all-zero weight, x_T untouched, reproducible
bits, bounds where the host loop's scaler clips, no capture, and the tapes and scratch handed back.

Tolerances.  One evaluation: D' = D + s J^T e, so with tau_D (assert_close's defaults, where test_log_likelihood.py pins
``denoise_vjp``'s denoised output against the oracle) and tau_J (rtol 2e-3, atol 2e-3 max|J^T v|, where it pins the product) the
bound is tau_D + s(sigma) tau_J.  Native against host loop: helpers.RTOL / ATOL, both sides run the same decoder kernels.
Trajectory: RTOL / ATOL scaled by 1 + beta, the per-step amplification of that bound."""
import functools
import math
import warnings

import pytest
import torch

from mdt_policy_amd import _lib, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_bounds import ActionBounds
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, inputs_of, load_fixture
from tests.test_log_likelihood import OracleModel, case, gpu_model, to_cuda

pytestmark = pytest.mark.gpu
SD, BETA = 0.5, 5.0  # gpu_model's and OracleModel's sigma_data; the steer's default clip


def take(state, n):
    return {k: (v[:n] if torch.is_tensor(v) else v) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def setup(name):
    """(meta, cfg, model on the GPU, state, goal, action) of a fixture's configuration: state / goal / action on the host."""
    if name in ("mdtv_tiny", "mdt_tiny"):
        meta, _, cfg, state, goal, action = case(name)
    else:  # a decoder variant: the training fixtures' configuration
        meta, _ = load_fixture(f"g11_grads_{name}.npz")
        cfg = cfg_of(meta)
        state, goal, _ = inputs_of(meta)
        action = torch.from_numpy(synthetic.loss_inputs(meta["B"], cfg, meta["loss_seed"])["actions"])
    return meta, cfg, gpu_model(meta, cfg), state, goal, action


def noise(shape, seed, tag="steer_noise"):
    return torch.from_numpy(synthetic.normal(tag, tuple(shape), seed))


def hard_steer(action, hard=3, soft=0, executed=2):
    """The receding-horizon steer of a replan: the previous chunk is the fixture's action chunk."""
    return ActionSteer.overlap(action, executed, hard, soft)


def werr(steer, out):
    known, w = steer.on("cpu", tuple(out.shape))
    return float((w.double() * (known.double() - out.double().cpu()) ** 2).sum())


def ddim_coefficients(sig, i):
    """gc_sampling.sample_ddim's step scalars, formed as it forms them (fp32 host tensors)."""
    t, tn = -sig[i].log(), -sig[i + 1].log()
    return ((-tn).exp() / (-t).exp()).item(), (-(tn - t)).expm1().item()


def oracle_steered(ref, state, goal, x, sigma, steer):
    """(D', D, J^T e) in float64: autograd through the oracle, e = W (known - D) a constant."""
    B = x.shape[0]
    xg = x.detach().double().requires_grad_()
    d = ref(state, xg, goal, torch.full((B,), float(sigma), dtype=torch.float64))
    if steer is None:
        return d.detach(), d.detach(), torch.zeros_like(d)
    known, w = steer.on("cpu", tuple(x.shape))
    e = w.double() * (known.double() - d.detach())
    j, = torch.autograd.grad((d * e).sum(), xg)
    return d.detach() + steer.scale(sigma, SD) * j, d.detach(), j


@functools.lru_cache(maxsize=None)
def oracle_trajectory(steered: bool, n=10, B=3):
    """10-step DDIM over the oracle in float64 from sigma_max-sized noise, with the hard steer or without one."""
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    ref = OracleModel(meta, cfg, torch.float64)
    st, g = take(state, B), goal[:B]
    steer = hard_steer(action[:B]) if steered else None
    sig = gs.get_sigmas_exponential(n, meta["sigma_min"], meta["sigma_max"]).to(torch.float32)
    x = (meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 41)).double()
    for i in range(n):
        d = oracle_steered(ref, st, g, x, float(sig[i]), steer)[0]
        ratio, em1 = ddim_coefficients(sig, i)
        x = ratio * x - em1 * d
    return x


# ----------------------------------------------------------------------------------------------------------------
# one evaluation
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mdtv_tiny", "mdt_tiny"])
def test_one_steered_evaluation_matches_float64_autograd_through_the_oracle(name):
    meta, cfg, model, state, goal, action = setup(name)
    B = 3
    ref = OracleModel(meta, cfg, torch.float64)
    st, g, act = take(state, B), goal[:B], action[:B]
    steer = hard_steer(act, hard=3, soft=2)
    kink = SD * math.sqrt(BETA - 1)
    for sigma in (meta["sigma_max"], kink, meta["sigma_min"]):
        x = act + sigma * noise(act.shape, 42)
        with torch.no_grad():
            got = model(to_cuda(st), x.cuda(), g.cuda(), torch.tensor([sigma], device="cuda"), steer=steer).cpu().double()
        want, d64, j64 = oracle_steered(ref, st, g, x, sigma, steer)
        s = steer.scale(sigma, SD)
        tol = (ATOL + RTOL * d64.abs()) + s * (2e-3 * float(j64.abs().max()) + 2e-3 * j64.abs())
        err = (got - want).abs()
        print(f"{name} sigma={sigma:g}: s={s:g} max |D' - oracle| {float(err.max()):.3e}, largest err / bound "
              f"{float((err / tol).max()):.3f}, max|D| {float(d64.abs().max()):.3e}, max|J^T e| {float(j64.abs().max()):.3e}")
        assert bool((err <= tol).all()), f"sigma={sigma}: {int((err > tol).sum())}/{err.numel()} outside tau_D + s tau_J"


# ----------------------------------------------------------------------------------------------------------------
# the native call against the host loop over forward
# ----------------------------------------------------------------------------------------------------------------
def both_ways(fn, model, state, goal, x, sigmas, extra_args, **kw):
    native = fn(model, state, x, goal, sigmas, extra_args=extra_args, **kw)
    seen = []
    host = fn(model, state, x, goal, sigmas, extra_args=extra_args, callback=lambda d: seen.append(d["i"]), **kw)
    assert seen == list(range(len(sigmas) - 1))  # the host loop ran
    return native, host


@pytest.mark.parametrize("steps", [3, 10])
@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (2, 40)])
def test_native_ddim_matches_the_host_loop(B, K, steps):
    """R = 1 is the single row; R = 15 is 1050 elements and 15 sigma entries, 1065 in all: five workgroups of 256 with a ragged
    last one, and the elements end inside a wave; R = 80 is 5680 entries with a per-observation steer expanded by ``on``."""
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    R = B * K
    x = (meta["sigma_max"] * noise((R,) + tuple(action.shape[1:]), 43)).cuda()
    if K == 5:  # per chunk: every chunk its own known part
        prev = action[:B].repeat_interleave(K, 0) + 0.1 * noise((R,) + tuple(action.shape[1:]), 44)
        steer = hard_steer(prev, hard=2, soft=3)
    else:       # per observation
        steer = hard_steer(action[:B], hard=3, soft=2)
    sigmas = gs.get_sigmas_exponential(steps, meta["sigma_min"], meta["sigma_max"])
    x_before = x.clone()
    native, host = both_ways(gs.sample_ddim, model, st, g, x, sigmas, {"steer": steer, "candidates": K})
    plain = gs.sample_ddim(model, st, x, g, sigmas, extra_args={"candidates": K})
    print(f"B={B} K={K} steps={steps}: max |native - host| {float((native - host).abs().max()):.3e}, "
          f"max |steered - plain| {float((native - plain).abs().max()):.3e}")
    assert torch.equal(x, x_before)  # x_T is only read
    assert native.shape == x.shape
    assert_close(native.cpu(), host.cpu(), what="native against the host loop")
    assert not torch.equal(native, plain)  # ... and the steer moved the chunk
    # the (B, K, Ta, A) shape goes in and comes out, the same bits
    again = gs.sample_ddim(model, st, x.reshape((B, K) + tuple(x.shape[1:])), g, sigmas, extra_args={"steer": steer, "candidates": K})
    assert again.shape == (B, K) + tuple(x.shape[1:]) and torch.equal(again.reshape(native.shape), native)


def test_native_euler_matches_its_host_loop():
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    B, K = 3, 5
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    x = (meta["sigma_max"] * noise((B * K,) + tuple(action.shape[1:]), 45)).cuda()
    steer = hard_steer(action[:B], hard=3, soft=2)
    sigmas = gs.get_sigmas_exponential(10, meta["sigma_min"], meta["sigma_max"])
    native, host = both_ways(gs.sample_euler, model, st, g, x, sigmas, {"steer": steer, "candidates": K})
    print(f"euler: max |native - host| {float((native - host).abs().max()):.3e}")
    assert_close(native.cpu(), host.cpu(), what="native euler against the host loop")
    assert torch.equal(native, gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": steer, "candidates": K}))  # the same call


@pytest.mark.parametrize("name,B,K", [("mdt_tiny", 2, 3), ("mdtv_no_ada", 2, 3), ("mdtv_noise_block", 2, 1)])
def test_native_ddim_matches_the_host_loop_on_the_other_configurations(name, B, K):
    """MDT (two state tokens); use_ada_conditioning=False, where sigma is a context token and the context is encoded again at
    every step; the NoiseBlock decoder."""
    meta, cfg, model, state, goal, action = setup(name)
    B = min(B, action.shape[0])
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    x = (80.0 * noise((B * K,) + tuple(action.shape[1:]), 46)).cuda()
    steer = hard_steer(action[:B], hard=3, soft=2)
    sigmas = gs.get_sigmas_exponential(3, 0.001, 80.0)
    native, host = both_ways(gs.sample_ddim, model, st, g, x, sigmas, {"steer": steer, "candidates": K})
    print(f"{name}: max |native - host| {float((native - host).abs().max()):.3e}")
    assert_close(native.cpu(), host.cpu(), what=f"{name}: native against the host loop")


# ----------------------------------------------------------------------------------------------------------------
# a trajectory against the oracle, and what steering is for
# ----------------------------------------------------------------------------------------------------------------
def native_trajectory(steered: bool, n=10, B=3):
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    x = (meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 41)).cuda()
    sigmas = gs.get_sigmas_exponential(n, meta["sigma_min"], meta["sigma_max"])
    return gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": hard_steer(action[:B])} if steered else None).cpu()


def test_ten_steps_against_a_float64_loop_over_the_oracle():
    """Measured on MI355X (mdtv_tiny, B = 3, 10 steps): see DESIGN.md 4.3i."""
    want = oracle_trajectory(True)
    got = native_trajectory(True)
    err = (got.double() - want).abs()
    tol = (1 + BETA) * (ATOL + RTOL * want.abs())
    print(f"10-step trajectory: max |native - oracle| {float(err.max()):.3e} (|oracle| max {float(want.abs().max()):.3e}), "
          f"largest err / bound {float((err / tol).max()):.3f}")
    assert_close(got, want, rtol=(1 + BETA) * RTOL, atol=(1 + BETA) * ATOL, what="steered DDIM against the oracle")


def test_steering_lowers_the_weighted_error():
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    steer = hard_steer(action[:3])
    # first on the oracle: the chosen inputs have the property at all
    o_steered, o_plain = werr(steer, oracle_trajectory(True)), werr(steer, oracle_trajectory(False))
    assert o_steered < o_plain, (o_steered, o_plain)
    n_steered, n_plain = werr(steer, native_trajectory(True)), werr(steer, native_trajectory(False))
    print(f"weighted error: oracle {o_plain:.4e} -> {o_steered:.4e}, native {n_plain:.4e} -> {n_steered:.4e}")
    assert n_steered < n_plain, (n_steered, n_plain)


def test_an_all_zero_weight_gives_the_plain_calls_bits_and_identical_calls_identical_bits():
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    B, K = 3, 2
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    x = (meta["sigma_max"] * noise((B * K,) + tuple(action.shape[1:]), 47)).cuda()
    sigmas = gs.get_sigmas_exponential(5, meta["sigma_min"], meta["sigma_max"])
    zero = ActionSteer(action[:B], torch.zeros(action.shape[1]))
    plain = gs.sample_ddim(model, st, x, g, sigmas, extra_args={"candidates": K})
    assert torch.equal(gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": zero, "candidates": K}), plain)
    with torch.no_grad():
        sg = torch.tensor([1.0], device="cuda")
        assert torch.equal(model(st, x[:B], g, sg, steer=zero), model(st, x[:B], g, sg))
    steer = hard_steer(action[:B], hard=3, soft=2)
    a = gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": steer, "candidates": K})
    b = gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": steer, "candidates": K})
    assert torch.equal(a, b) and not torch.equal(a, plain)
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == B  # the observations' context


def test_bounds_clamp_where_the_host_loops_scaler_clamps():
    """sample_euler clips after every step, sample_ddim takes a scaler and never reads it: the same in the steered calls."""
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    B = 3
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    A = action.shape[2]
    x = (meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 48)).cuda()
    steer = hard_steer(action[:B], hard=3, soft=2)
    sigmas = gs.get_sigmas_exponential(5, meta["sigma_min"], meta["sigma_max"])
    free = gs.sample_euler(model, st, x, g, sigmas, extra_args={"steer": steer})
    # bounds that bind on the result itself (and far inside the sigma-sized states of the early steps): its 20 % and 80 % points
    lo = torch.tensor([float(free.quantile(0.2))] * A)
    hi = torch.tensor([float(free.quantile(0.8))] * A)
    scaler = ActionBounds(lo.tolist(), hi.tolist())
    native, host = both_ways(gs.sample_euler, model, st, g, x, sigmas, {"steer": steer}, scaler=scaler)
    print(f"bounds [{float(lo[0]):.4f}, {float(hi[0]):.4f}]: max |native - host| {float((native - host).abs().max()):.3e}, "
          f"{int((native.cpu() == lo).sum())} at lo, {int((native.cpu() == hi).sum())} at hi")
    assert_close(native.cpu(), host.cpu(), what="clamped native euler against the host loop")
    assert bool((native.cpu() >= lo).all()) and bool((native.cpu() <= hi).all()) and not torch.equal(native, free)
    assert int((native.cpu() == lo).sum()) > 0 and int((native.cpu() == hi).sum()) > 0  # the clamp acted on the last step too
    ddim = gs.sample_ddim(model, st, x, g, sigmas, extra_args={"steer": steer})
    assert torch.equal(gs.sample_ddim(model, st, x, g, sigmas, scaler=scaler, extra_args={"steer": steer}), ddim)


def test_a_capturing_stream_is_refused_and_nothing_is_enqueued():
    meta, cfg, model, state, goal, action = setup("mdtv_tiny")
    B = 2
    st, g = to_cuda(take(state, B)), goal[:B].cuda()
    x = (meta["sigma_max"] * noise((B,) + tuple(action.shape[1:]), 49)).cuda()
    known, weight = hard_steer(action[:B]).on("cuda", tuple(x.shape))
    steer = ActionSteer(known, weight)  # on the device in the call's shape: ``on`` has nothing to launch
    sigmas = gs.get_sigmas_exponential(3, meta["sigma_min"], meta["sigma_max"])
    before = model.sample_ddim(st, x, g, sigmas, steer=steer)  # (parameters uploaded, buffers grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            with pytest.raises(_lib.MDTHipError) as err:
                model.sample_ddim(st, x, g, sigmas, steer=steer)
    assert err.value.status == 5 and "mdt_sample_ddim_steer" in str(err.value) and "captured" in str(err.value)  # MDT_ERR_STATE
    assert any("Graph is empty" in str(w.message) for w in seen), [str(w.message) for w in seen]
    torch.cuda.synchronize()
    assert torch.equal(model.sample_ddim(st, x, g, sigmas, steer=steer), before)  # the handle is as it was


def test_log_likelihood_has_the_same_bits_before_and_after_a_steered_call():
    """The steered call borrows mdt_log_likelihood's tapes and backward scratch: it hands them back as it found them."""
    from tests.test_gpu_loglik_native import signs, tiny
    meta, fx, model, state, goal, action = tiny()
    B = 2
    st, g, rows = take(state, B), goal[:B], action[:B].cuda()
    v = signs((1, B) + tuple(rows.shape[1:]), 12).cuda()
    before = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    steer = hard_steer(action[:3], hard=3, soft=2)
    x = (meta["sigma_max"] * noise((3 * 4,) + tuple(action.shape[1:]), 50)).cuda()
    sigmas = gs.get_sigmas_exponential(4, meta["sigma_min"], meta["sigma_max"])
    for _ in range(3):  # (more rows than the scoring call: the tapes and the scratch grow in between)
        out = model.sample_ddim(take(state, 3), x, goal[:3], sigmas, steer=steer, candidates=4)
    assert bool(torch.isfinite(out).all())
    after = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    assert after[3] == before[3] and all(torch.equal(a, b) for a, b in zip(after[:3], before[:3]))
