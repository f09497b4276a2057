"""The denoiser's options at contexts beyond 16 tokens, on the MI355X (pytest -m gpu): ctx17_hd48 (the shipped width, one key into
a second tile) and ctx33_rope_hd64 (RoPE, Te > 2 x 16) of tests/long_context_configs.py at B = 2, each option checked the way its
own test checks it at <= 16 tokens, with that test's reference and tolerance -- the list of tests/test_gpu_long_chunk_options.py:

  heun, dpmpp_2m, guidance, the pin (hard and soft), candidates with and without guidance, bounds and the per-step record, the
  steered DDIM
      the package's host loop on the CPU over the float64 oracle denoiser of tests/sampler_envelope.py (no kernel shared with the
      code under test) at helpers.RTOL / ATOL, test_gpu_guidance.tol for the guided calls, (1 + beta) x for the steered one;
  euler_ancestral (seeded), dpmpp_sde on its Brownian tree, dpm_adaptive, log_likelihood with two probes and best_candidates
      the host loop over the model's own per-step calls, as tests/test_gpu_native_samplers.py, test_gpu_brownian.py,
      test_gpu_native_dpm_adaptive.py and test_gpu_loglik_native.py compare them;
  the plain-C client
      tests/test_gpu_c_client.py's program and checks on the recorded fixtures of the two cases."""
import pytest
import torch

from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer
from tests import sampler_envelope as E
from tests import test_gpu_guidance as guid
from tests.family import OptionFamily
from tests.helpers import ATOL, RTOL, assert_close, cuda
from tests.long_context_configs import CTX_SHAPES, CTX_SPEC
from tests.test_gpu_brownian import _loop_sampler, _seed_of
from tests.test_gpu_loglik_native import LL, check_info, chunks_of, parent_path, signs
from tests.test_gpu_native_samplers import _host_loop
from tests.test_gpu_sampler_bounds import no_forward

pytestmark = pytest.mark.gpu

NAMES = ["ctx17_hd48", "ctx33_rope_hd64"]
B = 2
assert all(CTX_SPEC[n][0] == "mdtv" and not CTX_SPEC[n][3] and CTX_SHAPES[n][1] > 16 for n in NAMES)
F = OptionFamily(CTX_SPEC, dict(weight_seed=5, input_seed=E.SEED, loss_seed=62, ctx_seed=63), B)
meta_of, model_of, oracle_of, case = F.meta_of, F.model_of, F.oracle_of, F.case
float64_loop, both_runs, known_of = F.float64_loop, F.both_runs, F.known_of


@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("name", NAMES)
def test_fixed_step_samplers_against_the_float64_loop(name, kind, monkeypatch):
    got, want = both_runs(name, kind, monkeypatch)
    assert_close(got, want, what=f"{name} {kind}")


@pytest.mark.parametrize("name", NAMES)
def test_guided_sampler_against_the_float64_loop(name, monkeypatch):
    lam = 2.0
    got, want = both_runs(name, "heun", monkeypatch, extra={"cond_lambda": lam})
    plain = float64_loop(name, "heun")
    assert float((want - plain).abs().max()) > 100 * E.tol_of(want, **guid.tol(lam)), "guidance changes too little"
    assert_close(got, want, what=f"{name} guided heun", **guid.tol(lam))


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_pin_hard_and_soft(name, soft, monkeypatch):
    """hard: keep 1 on the first five tokens of every chunk (its already-executed prefix), 0 on the rest; soft: keep =
    (1, 0.5, 0)[(b + t + c) % 3]."""
    known = known_of(name)
    keep = E.pattern(*known.shape) if soft else torch.zeros(known.shape)
    if not soft:
        keep[:, :5] = 1.0
    pin = ActionPin(known, keep)
    got, want = both_runs(name, "ddim", monkeypatch, extra={"pin": pin}, tag="soft" if soft else "hard")
    free = float64_loop(name, "ddim")
    hard, rest = keep == 1, keep == 0
    assert float((want - free)[hard].abs().max()) > 100 * E.tol_of(want[hard])
    assert float((want - free)[rest].abs().max()) > 10 * E.tol_of(want[rest]), "the unpinned elements do not feel the pin"
    assert_close(got, want, what=f"{name} pinned ddim")
    assert torch.equal(got[hard], pin.on("cpu", tuple(want.shape))[0][hard]), f"{name}: pinned elements are not known"


@pytest.mark.parametrize("lam", [None, 2.0])
@pytest.mark.parametrize("name", NAMES)
def test_three_candidates_per_observation(name, lam, monkeypatch):
    """K = 3 chunks per observation from one shared context (the cross-attention reads context b / 3), plain and guided."""
    kind, extra, tol = ("ddim", None, {}) if lam is None else ("heun", {"cond_lambda": lam}, guid.tol(lam))
    got, want = both_runs(name, kind, monkeypatch, extra=extra, repeat=3)
    assert got.shape[0] == 3 * B
    assert_close(got, want, what=f"{name} {kind}, 3 candidates, lambda {lam}", **tol)
    assert tuple(model_of(name).inner_model.latent_encoder_emb.shape)[:2] == (B, CTX_SHAPES[name][1])  # one context per observation


@pytest.mark.parametrize("name", NAMES)
def test_bounds_and_the_per_step_record(name):
    kind = "heun"
    state, goal, x, fixed = case(name)
    ref = oracle_of(name)
    plain = float64_loop(name, kind)
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
def test_native_log_likelihood_with_two_probes_and_best_candidates(name):
    """mdt_log_likelihood on B observations x 2 chunks with two probe tensors against the host loop it replaces (_dopri5 over
    denoise_vjp on the expanded observations); best_candidates on its scores picks what the host loop's scores pick."""
    K = 2
    model = model_of(name)
    state, goal, x, fixed = case(name)
    action = -float64_loop(name, "ddim").float()   # a chunk the model produced
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
    best, index = gs.best_candidates(rows, ll, K)
    want_best, want_index = gs.best_candidates(rows.cpu(), want_ll, K)
    gaps = want_ll.reshape(B, K).sort(1).values
    if bool(((gaps[:, -1] - gaps[:, -2]).abs() > 10 * (LL["atol"] + LL["rtol"] * want_ll.abs().max())).all()):   # no near tie
        assert torch.equal(index.cpu(), want_index) and torch.equal(best.cpu(), want_best)
    assert best.shape == (B,) + tuple(rows.shape[1:])


@pytest.mark.parametrize("name", NAMES)
def test_native_steered_ddim_against_the_float64_loop(name, monkeypatch):
    known = known_of(name)
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


@pytest.mark.parametrize("name", NAMES)
def test_plain_c_client(name, tmp_path):
    """tests/c_client/client.c (no Python in that process) on the case's recorded fixture: the facade's bits, the reference's
    actions and its 17- / 33-token context."""
    from tests.test_gpu_c_client import test_c_host_program_matches_the_python_facade as c_client
    c_client(f"g21_ctx_{name}.npz", tmp_path)
