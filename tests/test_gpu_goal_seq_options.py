"""The denoiser's options with a goal of several tokens, on the MI355X (pytest -m gpu): g2_shipped (the shipped width, Te = 5),
g3_plain (the sigma token in the context: the encoder runs per step, the score stages B * S contexts) and mdt_g3_pos (MDT with a
position row per goal token) of tests/goal_seq_configs.py at B = 2, each option checked the way its own test checks it at one goal
token, with that test's reference and tolerance:

  guidance (cond_lambda = 3)       the float64 oracle composition D_u + lambda (D_g - D_u) of tests/sampler_envelope.py, D_u on the goal
                                   with ALL G rows zeroed, at test_gpu_guidance.tol; lambda = 1 gives the unguided call's bits
  candidates = 4 with a pin        the host loop through GCDenoiser.forward on the expanded observations
  denoising_score                  the float64 residual score of tests/score_oracle.py at tests/test_gpu_denoising_score.py's bound
  sample_select                    the bits of the three calls it replaces (tests/test_gpu_sample_select.py)
  a steer                          the float64 host loop, (1 + beta) x the forward tolerance (tests/test_gpu_steer.py)
  log_likelihood                   the host loop over denoise_vjp (tests/test_gpu_loglik_native.py)
  denoise_grad                     float64 autograd through the oracle (tests/test_gpu_denoise_grad.py); d_goal is (B, G, goal_dim)
  sample_heun, bounds and record   the float64 host loop with the clamp and its callback (tests/test_gpu_sampler_bounds.py)"""
import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import sampler_envelope as E
from tests import test_gpu_guidance as guid
from tests.family import OptionFamily
from tests.goal_seq_configs import GOAL_SPEC, GOAL_TE, goal_rows
from tests.guarded import same_bits
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, cuda, params_of
from tests.score_oracle import residual_score
from tests.test_gpu_loglik_native import LL, check_info, chunks_of, parent_path, signs
from tests.test_gpu_native_samplers import _host_loop
from tests.test_gpu_sampler_bounds import no_forward

pytestmark = pytest.mark.gpu

NAMES = ["g2_shipped", "g3_plain", "mdt_g3_pos"]
B = 2
EPS32 = float(np.finfo(np.float32).eps)
assert not any(GOAL_SPEC[n][3] for n in NAMES)


class GoalOptions(OptionFamily):
    def case(self, name, batch=B, seed=E.SEED):
        """(state, goal (batch, G, goal_dim), x_T, fixed noise) in float32 on the host; x_T = 80 noise."""
        state, goal, x, fixed = super().case(name, batch, seed)
        assert tuple(goal.shape) == (batch, goal_rows(name), cfg_of(self.meta_of(name))["goal_dim"])
        return state, goal, x, fixed


F = GoalOptions(GOAL_SPEC, dict(weight_seed=5, input_seed=E.SEED, loss_seed=62, ctx_seed=63), B)
meta_of, model_of, oracle_of, case, float64_loop = F.meta_of, F.model_of, F.oracle_of, F.case, F.float64_loop


@pytest.mark.parametrize("name", NAMES)
def test_guided_ddim_against_the_float64_composition_with_every_goal_row_zeroed(name, monkeypatch):
    lam = 3.0
    want = float64_loop(name, "ddim", {"cond_lambda": lam})
    plain = float64_loop(name, "ddim")
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want, **guid.tol(lam)), "guidance changes too little"
    # zeroing goal row 0 alone is another unconditional model: the composition depends on the other rows
    state, goal, x, fixed = case(name)
    half = goal.clone()
    half[:, 1:] = 0
    assert float((float64_loop(name, "ddim") - E.run("ddim", oracle_of(name), E.wide(state), E.wide(x), E.wide(half), E.wide(fixed))).abs().max()) \
        > 100 * E.tol_of(want), "goal rows past the first do not reach the result"
    with monkeypatch.context() as mp:
        no_forward(mp)
        got = E.run("ddim", model_of(name), cuda(state), x.cuda(), goal.cuda(), fixed.cuda(), extra_args={"cond_lambda": lam}).cpu()
    assert_close(got, want, what=f"{name} guided ddim", **guid.tol(lam))


@pytest.mark.parametrize("name", NAMES)
def test_lambda_one_gives_the_unguided_bits(name):
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    sig = gs.get_sigmas_exponential(5, 0.01, 80.0)
    with torch.no_grad():
        base = gs.sample_ddim(model, state, x, goal, sig)
        assert torch.equal(gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": 1.0}), base)
        base_e = gs.sample_euler(model, state, x, goal, sig)
        assert torch.equal(gs.sample_euler(model, state, x, goal, sig, extra_args={"cond_lambda": 1.0}), base_e)


@pytest.mark.parametrize("name", NAMES)
def test_four_candidates_with_a_pin_against_the_host_loop(name, monkeypatch):
    """K = 4 chunks per observation from one shared context of Te rows, pinned; the host loop runs GCDenoiser.forward on the
    observations repeated four times."""
    K = 4
    model = model_of(name)
    state, goal, _, _ = case(name)
    _, _, x, _ = case(name, B * K)
    known = -float64_loop(name, "ddim").float().repeat_interleave(K, 0)
    keep = E.pattern(*known.shape)
    pin = ActionPin(known, keep)
    sig = E.sched()
    wide_state = {k: (v.repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
    with torch.no_grad():
        want = _host_loop(gs.sample_ddim, model, cuda(wide_state), x.cuda(), goal.repeat_interleave(K, 0).cuda(), sig, extra_args={"pin": pin}).cpu()
        free = _host_loop(gs.sample_ddim, model, cuda(wide_state), x.cuda(), goal.repeat_interleave(K, 0).cuda(), sig).cpu()
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sig, extra_args={"pin": pin, "candidates": K}).cpu()
    assert got.shape[0] == B * K
    assert float((want - free)[keep == 0].abs().max()) > 10 * E.tol_of(want), "the unpinned elements do not feel the pin"
    assert_close(got, want, what=f"{name} 4 candidates, pinned")
    assert torch.equal(got[keep == 1], known[keep == 1])
    assert tuple(model.inner_model.latent_encoder_emb.shape)[:2] == (B, GOAL_TE[name])   # one context per observation


def score_case(name, K, S, M, seed=77):
    cfg = cfg_of(meta_of(name))
    state, goal, _, _ = case(name)
    x0 = torch.from_numpy(synthetic.loss_inputs(B * K, cfg, seed)["actions"])
    noise = torch.from_numpy(synthetic.normal("score_noise", (S, M) + tuple(x0.shape[1:]), seed + 1))
    levels = [float(v) for v in np.exp(np.linspace(np.log(80.0), np.log(0.001), S))]
    return state, goal, x0, levels, noise


@pytest.mark.parametrize("name", NAMES)
def test_denoising_score_against_float64(name):
    K, S, M = 3, 3, 2
    meta = meta_of(name)
    cfg, P = cfg_of(meta), params_of(meta)
    state, goal, x0, levels, noise = score_case(name, K, S, M)
    want, terms = residual_score(P, cfg, meta["arch"], state, goal, x0, levels, noise, K=K, dtype=torch.float64)
    f32, _ = residual_score(P, cfg, meta["arch"], state, goal, x0, levels, noise, K=K, dtype=torch.float32)
    bound = 3 * float((f32.double() - want).abs().max()) + 8 * EPS32 * terms
    with torch.no_grad():
        got = gs.denoising_score(model_of(name), cuda(state), x0.cuda(), goal.cuda(), levels, extra_args={"candidates": K},
                                 noise=noise.cuda()).cpu().double()
    err = (got - want).abs()
    print(f"{name}: max |score - float64| / bound {float((err / bound).max()):.3f}")
    assert tuple(got.shape) == (B * K,) and bool((err <= bound).all()), (err.tolist(), bound.tolist())


@pytest.mark.parametrize("name", NAMES)
def test_sample_select_has_the_bits_of_the_three_calls(name):
    from tests.test_gpu_sample_select import N_STEPS, one_call, three_calls
    K, S, M = 4, 3, 2
    model = model_of(name)
    state, goal, _, _ = case(name)
    shape = tuple(case(name)[2].shape[1:])
    x_T = 80.0 * torch.from_numpy(synthetic.normal("x_T", (B * K,) + shape, 91))
    snoise = torch.from_numpy(synthetic.normal("score_noise", (S, M) + shape, 92))
    rows = torch.from_numpy(synthetic.normal("sampler_noise", (N_STEPS, B * K) + shape, 93))
    levels = [float(v) for v in np.exp(np.linspace(np.log(80.0), np.log(0.001), S))]
    c = dict(state=cuda(state), goal=goal.cuda(), x_T=x_T.cuda(), levels=levels, snoise=snoise.cuda(), rows=rows.cuda(),
             sig=gs.get_sigmas_exponential(N_STEPS, 0.001, 80.0))
    with torch.no_grad():
        for kind in ("ddim", "dpmpp_2m"):
            want = three_calls(model, c, K, kind)
            got = one_call(model, c, K, kind)
            torch.cuda.synchronize()
            for what, g, w in zip(("best", "index", "scores", "chunks", "ctx_out"), got, want):
                assert (torch.equal(g, w) if what == "index" else same_bits(g, w)), (name, kind, what)
            assert tuple(got[4].shape)[:2] == (B, GOAL_TE[name]) and bool(torch.isfinite(got[2]).all())


@pytest.mark.parametrize("name", NAMES)
def test_native_steered_ddim_against_the_float64_loop(name, monkeypatch):
    known = -float64_loop(name, "ddim").float()
    steer = ActionSteer(known, E.pattern(*known.shape, values=(1.0, 0.25, 0.0)), E.BETA)
    state, goal, x, _ = case(name)
    sig = gs.get_sigmas_exponential(3, E.STEER_SMIN, E.SMAX)
    ref = oracle_of(name)
    with torch.no_grad():
        unsteered = gs.sample_ddim(ref, E.wide(state), E.wide(x), E.wide(goal), sig)
        want = gs.sample_ddim(ref, E.wide(state), E.wide(x), E.wide(goal), sig, extra_args={"steer": steer})
    assert E.werr(steer, want) < E.werr(steer, unsteered)
    assert float((want - unsteered).abs().max()) > 100 * (1 + E.BETA) * E.tol_of(want)
    model = model_of(name)
    no_forward(monkeypatch)
    with torch.no_grad():
        got = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sig, extra_args={"steer": steer}).cpu()
    assert_close(got, want, rtol=(1 + E.BETA) * RTOL, atol=(1 + E.BETA) * ATOL, what=f"{name}: steered DDIM")


@pytest.mark.parametrize("name", NAMES)
def test_native_log_likelihood_against_the_host_loop(name):
    K = 2
    model = model_of(name)
    state, goal, _, _ = case(name)
    action = -float64_loop(name, "ddim").float()   # a chunk the model produced
    state, goal = cuda(state), goal.cuda()
    rows = chunks_of(action, K).cuda()
    v = signs((2, B * K) + tuple(rows.shape[1:]), 5).cuda()
    want_ll, want_latent, want_delta, want_fe = parent_path(model, state, goal, rows, v, K, E.LL_SMIN, E.LL_SMAX)
    ll, latent, delta, info = model.log_likelihood(state, rows, goal, v, E.LL_SMIN, E.LL_SMAX, candidates=K)
    assert ll.shape == (B * K,)
    assert_close(latent.cpu(), want_latent, rtol=RTOL, atol=ATOL * E.LL_SMAX, what=f"{name}: latent")
    assert_close(delta.cpu(), want_delta, what=f"{name}: delta", **LL)
    assert_close(ll.cpu(), want_ll, what=f"{name}: log-likelihood", **LL)
    assert 0.3 * want_fe <= info["fevals"] <= 3 * want_fe
    check_info(info)


@pytest.mark.parametrize("name", NAMES)
def test_denoise_grad_against_float64_autograd(name):
    """L = (D . w).sum(): the value, then the gradient of every parameter and input; d_goal comes back (B, G, goal_dim) with every
    row filled."""
    from tests.test_gpu_denoise_grad import all_grads, check_grads, leaves, oracle_run, upstream
    meta = meta_of(name)
    cfg = cfg_of(meta)
    model = model_of(name)
    state, goal, _, _ = case(name, 3, 81)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(3, cfg, 82).items()}
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    token = not cfg["use_ada_conditioning"]   # sigma is a context token: everything but d_sigma (tests/test_gpu_denoise_grad.py)
    if token:
        sigma = sigma.detach()
    w = upstream(x.shape)
    model.zero_grad(set_to_none=True)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    vals = {}

    def objective(denoise, x64, s64, dev):
        vals["den"] = denoise(x64, s64)
        return (vals["den"] * w.double().to(dev)).sum()

    _, ref = oracle_run(meta, cfg, state, goal, li, objective, sigma_grad=not token)
    assert_close(den.detach().cpu(), vals["den"].detach().cpu(), rtol=1e-3, atol=1e-4, what=name + " denoised")
    assert tuple(ggoal.grad.shape) == (3, goal_rows(name), cfg["goal_dim"])
    assert bool((ggoal.grad.abs().amax(dim=(0, 2)) > 0).all()), "a goal row without a gradient"
    got = all_grads(model, gstate, ggoal, x, sigma)
    if token:
        assert got.pop("d_sigma") is None and ref.pop("d_sigma") is None
    check_grads(got, ref, name, at_least=30)
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("name", NAMES)
def test_heun_with_bounds_and_the_per_step_record(name):
    kind = "heun"
    state, goal, x, fixed = case(name)
    ref = oracle_of(name)
    plain = float64_loop(name, kind)
    lo, hi = E.quantile_bounds(plain)
    scaler, seen = E.ClampOnly(lo, hi), []
    want = E.run(kind, ref, E.wide(state), E.wide(x), E.wide(goal), E.wide(fixed), scaler=scaler,
                 callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want)
    model = model_of(name)
    kw = dict(E.KINDS[kind], noise=torch.zeros((E.N,) + tuple(x.shape), device="cuda"), bounds=(lo, hi))
    with torch.no_grad():
        out, rec = model.sample_native(kind, cuda(state), x.cuda(), goal.cuda(), E.sched(), record=True, **kw)
        bare = model.sample_native(kind, cuda(state), x.cuda(), goal.cuda(), E.sched(), **kw)
    assert torch.equal(out, bare), f"{name}: record=True changed the actions"
    assert_close(out.cpu(), want, what=f"{name}: bounded actions")
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs, what=f"{name}: x[{i}]")
        assert_close(rec["denoised"][i].cpu(), den, what=f"{name}: denoised[{i}]")
    assert bool((out.cpu() >= lo).all()) and bool((out.cpu() <= hi).all())
