"""The denoiser's options at action chunks beyond 16 steps, on the MI355X (pytest -m gpu): two small models -- adaLN conditioning
at 24 steps, RoPE at 40 (d 128, 4 heads of 32) -- at B = 2, each option checked the way its own test checks it at 10 steps, with
that test's reference and tolerance:

  heun, dpmpp_2m, guidance, the pin, candidates, bounds and the per-step record, the steered DDIM, denoise_vjp
      the package's host loop on the CPU over the float64 oracle denoiser of tests/sampler_envelope.py (no kernel shared with the
      code under test) at helpers.RTOL / ATOL, test_gpu_guidance.tol for the guided call, (1 + beta) x for the steered one;
  euler_ancestral (seeded), dpmpp_sde on its Brownian tree, dpm_adaptive, log_likelihood with two probes
      the host loop over the model's own per-step calls, as tests/test_gpu_native_samplers.py, test_gpu_brownian.py,
      test_gpu_native_dpm_adaptive.py and test_gpu_loglik_native.py compare them;
  denoise_grad, one train-mode step with the shipped dropouts
      float64 autograd through the oracle (replaying the Philox masks), as tests/test_gpu_denoise_grad.py and
      tests/test_gpu_train_dropout.py hold them."""
import pytest
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import sampler_envelope as E
from tests import test_gpu_denoise_grad as DG
from tests import test_gpu_guidance as guid
from tests import test_gpu_train_dropout as TD
from tests.family import OptionFamily
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, cuda, inputs_of
from tests.test_gpu_brownian import _loop_sampler, _seed_of
from tests.test_gpu_loglik_native import LL, check_info, chunks_of, parent_path, signs
from tests.test_gpu_native_samplers import _host_loop
from tests.test_gpu_sampler_bounds import no_forward

pytestmark = pytest.mark.gpu

_SMALL = dict(embed_dim=128, obs_dim=128, n_heads=4)
OPTION_CASES = {
    "adaln_ta24": dict(_SMALL, action_seq_len=24),
    "rope_ta40": dict(_SMALL, use_rot_embed=True, action_seq_len=40),
}
NAMES = sorted(OPTION_CASES)
B = 2


class _Spec(dict):
    """OPTION_CASES as a SPEC table, read at call time: tests/test_gpu_steer_plan_envelope.py adds a row after the import."""

    def __missing__(self, name):
        return "mdtv", "mdtv_default", OPTION_CASES[name], False


F = OptionFamily(_Spec(), dict(weight_seed=5, input_seed=E.SEED, loss_seed=62, ctx_seed=63), B)
meta_of, model_of, oracle_of, case, both_runs = F.meta_of, F.model_of, F.oracle_of, F.case, F.both_runs


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("name", NAMES)
def test_fixed_step_samplers_against_the_float64_loop(name, kind, monkeypatch):
    got, want = both_runs(name, kind, monkeypatch)
    assert_close(got, want, what=f"{name} {kind}")


@pytest.mark.parametrize("name", NAMES)
def test_guided_sampler_against_the_float64_loop(name, monkeypatch):
    lam = 2.0
    got, want = both_runs(name, "heun", monkeypatch, extra={"cond_lambda": lam})
    _, plain = both_runs(name, "heun", monkeypatch)
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want, **guid.tol(lam)), "guidance changes too little"
    assert_close(got, want, what=f"{name} guided heun", **guid.tol(lam))


def first_tokens_pin(name, n=5):
    """Known actions on the first n tokens of every chunk (the chunk's already-executed prefix): the negated unpinned result of
    another noise seed; keep 1 there, 0 on the rest."""
    state, goal, _, fixed = case(name)
    _, _, x_other, _ = case(name, seed=E.OTHER_SEED)
    known = -E.run("ddim", oracle_of(name), E.wide(state), E.wide(x_other), E.wide(goal), E.wide(fixed))
    keep = torch.zeros(known.shape)
    keep[:, :n] = 1.0
    return ActionPin(known, keep), keep


@pytest.mark.parametrize("name", NAMES)
def test_pin_on_the_first_five_tokens(name, monkeypatch):
    pin, keep = first_tokens_pin(name)
    got, want = both_runs(name, "ddim", monkeypatch, extra={"pin": pin})
    _, free = both_runs(name, "ddim", monkeypatch)
    hard, rest = keep == 1, keep == 0
    known = pin.on("cpu", tuple(want.shape))[0]
    assert float((want - free)[hard].abs().max()) > 100 * E.tol_of(want[hard])
    assert float((want - free)[rest].abs().max()) > 10 * E.tol_of(want[rest]), "the unpinned tokens do not feel the pin"
    assert_close(got, want, what=f"{name} pinned ddim")
    assert torch.equal(got[hard], known[hard]), f"{name}: pinned elements are not known"


@pytest.mark.parametrize("name", NAMES)
def test_three_candidates_per_observation(name, monkeypatch):
    got, want = both_runs(name, "ddim", monkeypatch, repeat=3)
    assert got.shape[0] == 3 * B
    assert_close(got, want, what=f"{name} ddim, 3 candidates")
    assert tuple(model_of(name).inner_model.latent_encoder_emb.shape)[0] == B  # one context per observation


@pytest.mark.parametrize("name", NAMES)
def test_bounds_and_the_per_step_record(name):
    kind = "heun"
    state, goal, x, fixed = case(name)
    ref = oracle_of(name)
    plain = E.run(kind, ref, E.wide(state), E.wide(x), E.wide(goal), E.wide(fixed))
    lo, hi = E.quantile_bounds(plain)
    scaler, seen = E.ClampOnly(lo, hi), []
    want = E.run(kind, ref, E.wide(state), E.wide(x), E.wide(goal), E.wide(fixed), scaler=scaler,
                 callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
    assert len(scaler.changed) == E.N and min(scaler.changed) >= 0.10, scaler.changed
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want)
    model = model_of(name)
    kw = dict(E.KINDS[kind], noise=torch.zeros((E.N,) + tuple(x.shape), device="cuda"), bounds=(lo, hi))
    with torch.no_grad():
        out, rec = model.sample_native(kind, cuda(state), x.cuda(), goal.cuda(), E.sched(), record=True, **kw)
        bare = model.sample_native(kind, cuda(state), x.cuda(), goal.cuda(), E.sched(), **kw)
    assert torch.equal(out, bare), f"{name}: record=True changed the actions"
    assert_close(out.cpu(), want, what=f"{name}: bounded actions")
    assert rec["x"].shape == rec["denoised"].shape == (E.N,) + tuple(x.shape)
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs, what=f"{name}: x[{i}]")
        assert_close(rec["denoised"][i].cpu(), den, what=f"{name}: denoised[{i}]")
    assert bool((out.cpu() >= lo).all()) and bool((out.cpu() <= hi).all())


@pytest.mark.parametrize("name", NAMES)
def test_seeded_euler_ancestral_follows_the_host_loops_random_stream(name):
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    sig = gs.get_sigmas_exponential(6, 0.001, 80.0)
    with torch.no_grad():
        torch.manual_seed(1234)
        want = _host_loop(gs.sample_euler_ancestral, model, state, x, goal, sig, eta=1.)
        after_loop = torch.randn(5, device="cuda")
        torch.manual_seed(1234)
        got = gs.sample_euler_ancestral(model, state, x, goal, sig, eta=1.)
        after_native = torch.randn(5, device="cuda")
    assert_close(got.cpu(), want.cpu(), what=f"{name} euler_ancestral")
    assert torch.equal(after_native, after_loop), "the native call left the generator elsewhere than the host loop"


@pytest.mark.parametrize("name", NAMES)
def test_dpmpp_sde_on_its_native_brownian_tree(name, monkeypatch):
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    sig = gs.get_sigmas_exponential(6, 0.001, 80.0)
    seed = _seed_of(3)
    with torch.no_grad():
        loop = gs.sample_dpmpp_sde(model, state, x, goal, sig, noise_sampler=_loop_sampler(x, sig, seed), callback=lambda d: None)
        with monkeypatch.context() as mp:
            no_forward(mp)
            torch.manual_seed(3)
            got = gs.sample_dpmpp_sde(model, state, x, goal, sig, scaler=None, disable=True)
    assert_close(got.cpu(), loop.cpu(), what=f"{name} dpmpp_sde, tree noise")


@pytest.mark.parametrize("name", NAMES)
def test_dpm_adaptive_native_matches_the_host_loop(name):
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    with torch.no_grad():
        want, winfo = _host_loop(gs.sample_dpm_adaptive, model, state, x, goal, 0.01, 80.0, return_info=True)
        with pytest.MonkeyPatch.context() as mp:
            no_forward(mp)
            got, info = gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, return_info=True)
    assert info == winfo, (info, winfo)
    assert_close(got.cpu(), want.cpu(), rtol=2e-3, atol=5e-4, what=f"{name} dpm_adaptive")   # tests/test_gpu_native_dpm_adaptive.py


@pytest.mark.parametrize("name", NAMES)
def test_native_log_likelihood_with_two_probes(name):
    """mdt_log_likelihood on B observations x 2 chunks with two probe tensors against the host loop it replaces (_dopri5 over
    denoise_vjp on the expanded observations)."""
    K = 2
    model = model_of(name)
    state, goal, x, fixed = case(name)
    action = -E.run("ddim", oracle_of(name), E.wide(state), E.wide(x), E.wide(goal), E.wide(fixed)).float()   # a chunk the model produced
    state, goal = cuda(state), goal.cuda()
    rows = chunks_of(action, K).cuda()
    v = signs((2, B * K) + tuple(rows.shape[1:]), 5).cuda()
    want_ll, want_latent, want_delta, want_fe = parent_path(model, state, goal, rows, v, K, E.LL_SMIN, E.LL_SMAX)
    ll, latent, delta, info = model.log_likelihood(state, rows, goal, v, E.LL_SMIN, E.LL_SMAX, candidates=K)
    print(f"{name}: fevals {info['fevals']} (host loop {want_fe}); max |ll - host| {float((ll.cpu() - want_ll).abs().max()):.3e}")
    assert ll.shape == (B * K,)
    assert_close(latent.cpu(), want_latent, rtol=RTOL, atol=ATOL * E.LL_SMAX, what=f"{name}: latent")
    assert_close(delta.cpu(), want_delta, what=f"{name}: delta", **LL)
    assert_close(ll.cpu(), want_ll, what=f"{name}: log-likelihood", **LL)
    assert 0.3 * want_fe <= info["fevals"] <= 3 * want_fe
    check_info(info)


@pytest.mark.parametrize("name", NAMES)
def test_native_steered_ddim_against_the_float64_loop(name, monkeypatch):
    pin, _ = first_tokens_pin(name)
    known = pin.on("cpu", (B,) + E_shape(name))[0]
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
        plain = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sig).cpu()
    assert_close(got, want, rtol=(1 + E.BETA) * RTOL, atol=(1 + E.BETA) * ATOL, what=f"{name}: steered DDIM")
    assert E.werr(steer, got) < E.werr(steer, plain)


def E_shape(name):
    cfg = cfg_of(meta_of(name))
    return cfg["action_seq_len"], cfg["action_dim"]


def loss_case(name):
    meta = meta_of(name)
    cfg = cfg_of(meta)
    state, goal, _ = inputs_of(meta)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, meta["loss_seed"]).items()}
    return meta, cfg, state, goal, li


@pytest.mark.parametrize("name", NAMES)
def test_denoise_grad_against_float64_autograd(name):
    """L = (D . w).sum() through GCDenoiser.denoise_grad: the value and the gradient of every parameter, the state tokens, the goal,
    the noisy actions and sigma (tests/test_gpu_denoise_grad.py)."""
    meta, cfg, state, goal, li = loss_case(name)
    model = model_of(name)
    model.zero_grad(set_to_none=True)
    gstate, ggoal, x, sigma = DG.leaves(state, goal, li)
    w = DG.upstream(x.shape)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    vals = {}

    def objective(denoise, x64, s64, dev):
        vals["den"] = denoise(x64, s64)
        return (vals["den"] * w.double().to(dev)).sum()

    _, ref = DG.oracle_run(meta, cfg, state, goal, li, objective)
    assert_close(den.detach().cpu(), vals["den"].detach().cpu(), rtol=1e-3, atol=1e-4, what=name + " denoised")
    got = DG.all_grads(model, gstate, ggoal, x, sigma)
    assert got["d_sigma"] is not None and got["d_x"] is not None
    DG.check_grads(got, ref, name, at_least=30)
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("name", NAMES)
def test_train_mode_step_matches_the_masked_float64_oracle(name):
    """One train-mode step with the shipped dropouts (attention 0.3, residual 0.1, MLP 0.05): loss, model output, context and
    every gradient against the float64 oracle that replays the Philox masks (tests/test_gpu_train_dropout.py)."""
    meta, cfg, state, goal, li = loss_case(name)
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    model, seeds = TD.facade(meta, cfg)
    hip = TD.hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    ref = TD.oracle_loss_step(meta, cfg, state, goal, li, seeds[0], None)
    TD.check_step(hip, ref, name, at_least=30)
