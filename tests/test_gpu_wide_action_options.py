"""The denoiser's options at action widths beyond 16, on the MI355X (pytest -m gpu): a17 (the shipped MDT-V, one column into the
second tile) and a64_ta24_rope_hd64 (the top of the range with RoPE and 24-step chunks) of tests/wide_action_configs.py at B = 2,
each option checked the way its own test checks it at action_dim <= 16, with that test's reference and tolerance:

  heun, dpmpp_2m, guidance, the pin, candidates, bounds and the per-step record, the steered DDIM
      the package's host loop on the CPU over the float64 oracle denoiser of tests/sampler_envelope.py (no kernel shared with the
      code under test) at helpers.RTOL / ATOL, test_gpu_guidance.tol for the guided call, (1 + beta) x for the steered one;
  euler, lms, dpm_fast, euler_ancestral (seeded), dpmpp_sde on its Brownian tree, dpm_adaptive, log_likelihood with two probes
      the host loop over the model's own per-step calls, as tests/test_gpu_native_samplers.py, test_gpu_native_dpm.py,
      test_gpu_brownian.py, test_gpu_native_dpm_adaptive.py and test_gpu_loglik_native.py compare them."""
import pytest
import torch

from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import sampler_envelope as E
from tests import test_gpu_guidance as guid
from tests.family import OptionFamily
from tests.helpers import ATOL, RTOL, assert_close, cuda
from tests.test_gpu_brownian import _loop_sampler, _seed_of
from tests.test_gpu_loglik_native import LL, check_info, chunks_of, parent_path, signs
from tests.test_gpu_native_dpm import _close
from tests.test_gpu_native_samplers import _host_loop
from tests.test_gpu_sampler_bounds import no_forward
from tests.wide_action_configs import WIDE_SPEC

pytestmark = pytest.mark.gpu

NAMES = ["a17", "a64_ta24_rope_hd64"]
B = 2
assert all(WIDE_SPEC[n][0] == "mdtv" and not WIDE_SPEC[n][3] for n in NAMES)
F = OptionFamily(WIDE_SPEC, dict(weight_seed=5, input_seed=E.SEED), B)
meta_of, model_of, oracle_of, case = F.meta_of, F.model_of, F.oracle_of, F.case
float64_loop, both_runs, known_of = F.float64_loop, F.both_runs, F.known_of


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("name", NAMES)
def test_fixed_step_samplers_against_the_float64_loop(name, kind, monkeypatch):
    got, want = both_runs(name, kind, monkeypatch)
    assert_close(got, want, what=f"{name} {kind}")


@pytest.mark.parametrize("kind,kw", [("euler", {}), ("lms", {})])
@pytest.mark.parametrize("name", NAMES)
def test_native_samplers_against_the_models_own_host_loop(name, kind, kw, monkeypatch):
    """tests/test_gpu_native_samplers.py's comparison: the native call against the same sampler's host loop over the model."""
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    sig = gs.get_sigmas_exponential(6, 0.001, 80.0)
    fn = getattr(gs, "sample_" + kind)
    with torch.no_grad():
        want = _host_loop(fn, model, state, x, goal, sig, **kw)
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = fn(model, state, x, goal, sig, **kw)
    assert_close(got.cpu(), want.cpu(), what=f"{name} {kind}")


@pytest.mark.parametrize("name", NAMES)
def test_dpm_fast_native_matches_the_host_loop(name, monkeypatch):
    model = model_of(name)
    state, goal, x, _ = case(name)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    n = 6
    with torch.no_grad():
        want = _host_loop(gs.sample_dpm_fast, model, state, x, goal, 0.01, 80.0, n)
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = gs.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, n)
    _close(got, want, n, f"{name} dpm_fast")


@pytest.mark.parametrize("name", NAMES)
def test_guided_sampler_at_lambda_3(name, monkeypatch):
    lam = 3.0
    got, want = both_runs(name, "heun", monkeypatch, extra={"cond_lambda": lam})
    plain = float64_loop(name, "heun")
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want, **guid.tol(lam)), "guidance changes too little"
    assert_close(got, want, what=f"{name} guided heun", **guid.tol(lam))


@pytest.mark.parametrize("name", NAMES)
def test_pin_with_keep_0_1_and_a_half_on_both_sides_of_column_16(name, monkeypatch):
    """keep = (1, 0.5, 0)[(b + t + c) % 3]: every row holds all three values below and above column 16."""
    known = known_of(name)
    keep = E.pattern(*known.shape)
    for side in (keep[0, 0, :16], keep[0, 0, 16:]):
        assert set(side.tolist()) == {0.0, 0.5, 1.0} or side.numel() < 3
    assert {float(keep[0, t, 16]) for t in range(3)} == {0.0, 0.5, 1.0}
    pin = ActionPin(known, keep)
    got, want = both_runs(name, "ddim", monkeypatch, extra={"pin": pin})
    free = float64_loop(name, "ddim")
    E.conditions(f"{name} pinned ddim (float64 loop)", free, want, known, keep)
    assert_close(got, want, what=f"{name} pinned ddim")
    hard = keep == 1
    assert torch.equal(got[hard], pin.on("cpu", tuple(want.shape))[0][hard]), f"{name}: pinned elements are not known"


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
    plain = float64_loop(name, kind)
    lo, hi = E.quantile_bounds(plain)
    assert lo.shape == hi.shape == (x.shape[-1],)
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
    state, goal, _, _ = case(name)
    action = -known_of(name).float()   # a chunk the model produced
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
    known = known_of(name).float()
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
