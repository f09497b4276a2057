"""The sampler options on the configurations of tests/envelope_configs.ENVELOPE, on the MI355X (pytest -m gpu): pinned actions,
bounds and the per-step record, the guided plan head, candidates, denoise_vjp, the steer and mdt_log_likelihood, each against the
package's host loop run on the CPU over the float64 oracle denoiser of tests/sampler_envelope.py -- no kernel is shared with the
code under test.  What the envelope varies is what the action head indexes with: AMAX = 16 (a16_ctx16, mdt_h6_a12), Ta = A = 1
(h1_d64_min: sigma[row / rows_per_sample] with one row per sample), 16, 36 and 128 live lanes of the LayerNorm (D = 64, 144, 512),
the guided twin at row base + M, per = Ta A = 1 / 112 / 120 / 160 in the log-likelihood's row kernels.

Tolerances are the existing ones: helpers.RTOL / ATOL; test_gpu_guidance.tol(2.5) for the guided cases; assert_close's defaults on
D and rtol 2e-3, atol 2e-3 max|J^T v| on the product (test_log_likelihood); tau_D + s(sigma) tau_J for one steered evaluation and
RTOL / ATOL scaled by 1 + beta for the steered trajectory (test_gpu_steer); rtol 2e-3, atol 0.05 on ll and delta, RTOL and
ATOL sigma_max on the latent, fevals within 0.3 x .. 3 x (test_gpu_loglik_native).  The conditions that keep a comparison from
being vacuous are asserted on the float64 loops, here as in tests/test_sampler_envelope.py, whose docstring has the numbers.

Where the pinned elements arrive: every evaluation's denoised value is ``known`` there bit for bit (asserted on the record), and
so are the actions of the kinds whose last update is x' = D' (ddim, dpmpp_2m).  heun, lms and dpmpp_sde end with
x' = x + sum c_j d_j, d = (x - D') / sigma, which reaches ``known`` to rounding only -- in the float64 host loop too (lms: 8e-9,
the quadrature of its coefficients) -- so their actions are held to the float64 loop at RTOL / ATOL, their pinned elements to
8 eps (max |x_last| + max |known|) of ``known``, and their record to the bits.

Measured on the MI355X: pin, max |native - float64| 2.6e-8 .. 1.2e-6 at B = 3 and up to 1.7e-6 at B = 40 (|want| max 0.8 .. 2.5);
the pinned elements of heun / lms / dpmpp_sde are off ``known`` by at most 4.8e-7 (lms), those of ddim and dpmpp_2m by 0.  One
steered evaluation: at most 0.003 of its bound.  Log-likelihood: 74 evaluations (rope_ta16: 68), the float64 run's count, on all
six configurations; |latent - float64| at most 7.1e-4 against 8e-3, |delta - float64| at most 4.6e-4 against 0.05.  The module
takes about 40 s, 1.4 s the slowest case (a16_ctx16 ddim, its three float64 loops) and 2 s the slowest log-likelihood."""
import pytest
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests import sampler_envelope as E
from tests import test_gpu_guidance as guid
from tests.helpers import ATOL, RTOL, assert_close, cuda
from tests.test_gpu_config_envelope import model_of
from tests.test_gpu_loglik_native import LL, check_info
from tests.test_gpu_sampler_bounds import no_forward

pytestmark = pytest.mark.gpu
B = 3
SELECTS_LAST = ("ddim", "dpmpp_2m")  # the last update is x' = D'
PIN_CASES = [(kind, B) for kind in E.KINDS] + [("heun", 40)]  # 40: past the 32-sample attention threshold


def gpu_case(name, batch, repeat=1):
    """(model, state, goal, x_T, fixed noise) on the device: E.chunk_case's inputs."""
    state, goal, x, fixed, _ = E.chunk_case(name, batch, repeat)
    return model_of(name)[0], cuda(state), goal.cuda(), x.cuda(), fixed.cuda()


def pinned_reference(name, kind, batch, lam=1.0, repeat=1, **tol):
    """(pin, keep, known in float32, float64 pinned result, float64 unpinned result); the conditions are asserted here."""
    free, known, want = E.loops(name, kind, batch, lam, repeat)
    keep = E.pattern(*want.shape)
    E.conditions(f"{name} {kind} B={batch} K={repeat} lambda={lam}", free, want, known, keep, lone=E.is_lone(name),
                 atol=tol.get("atol", ATOL), rtol=tol.get("rtol", RTOL))
    pin = E.pin_of(name, kind, batch, lam, repeat)
    return pin, keep, pin.on("cpu", tuple(want.shape))[0], want, free


def native_rows(kind, x, fixed):
    """The noise rows of a sample_native call in the loop's draw order: heun's N draws (s_churn = 0: multiplied by 0),
    dpmpp_sde's two values per step but the last."""
    if kind == "heun":
        return torch.zeros((E.N,) + tuple(x.shape), device=x.device)
    if kind == "dpmpp_sde":
        return fixed.expand((2 * (E.N - 1),) + tuple(x.shape)).contiguous()
    return None


# ---- a: the pin, every kind ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,batch", PIN_CASES)
@pytest.mark.parametrize("name", E.NAMES)
def test_pin_against_the_float64_loop(name, kind, batch, monkeypatch):
    pin, keep, known, want, _ = pinned_reference(name, kind, batch)
    model, state, goal, x, fixed = gpu_case(name, batch)
    with monkeypatch.context() as mp:
        no_forward(mp)
        got = E.run(kind, model, state, x, goal, fixed, extra_args={"pin": pin}).cpu()
        plain = E.run(kind, model, state, x, goal, fixed).cpu() if E.is_lone(name) else None
    hard = keep == 1
    off = int((got[hard] != known[hard]).sum())
    print(f"{name} {kind} B={batch}: max |native - float64| {float((got.double() - want).abs().max()):.3e} (|want| max "
          f"{float(want.abs().max()):.3f}); {off}/{int(hard.sum())} pinned elements off known, by "
          f"{float((got - known)[hard].abs().max()):.3e} at most")
    assert_close(got, want, what=f"{name} {kind} B={batch}")
    if kind in SELECTS_LAST:
        assert torch.equal(got[hard], known[hard]), f"{name} {kind}: {off} pinned elements are not known"
    with torch.no_grad():  # every evaluation's D' is known on the pinned elements, bit for bit
        if kind == "ddim":
            den = model(state, x, goal, torch.tensor([E.SMAX], device="cuda"), pin=pin).cpu()
            assert torch.equal(den[hard], known[hard]), f"{name}: D' is not known on the pinned elements"
        else:
            out, rec = model.sample_native(kind, state, x, goal, E.sched(), noise=native_rows(kind, x, fixed), pin=pin, record=True,
                                           **E.KINDS[kind])
            assert torch.equal(out.cpu(), got), f"{name} {kind}: record=True changed the actions"
            for i in range(E.N):
                assert torch.equal(rec["denoised"][i].cpu()[hard], known[hard]), f"{name} {kind}: the recorded denoised[{i}] is not D'"
            if kind not in SELECTS_LAST:
                # x' = x + sum c_j d_j over at most five float32 terms no larger than max |c| (<= 1.2) times
                # scale = max |x_last| + max |known|: each operation rounds by at most eps / 2 of that, 8 eps scale covers them
                scale = float(rec["x"][E.N - 1].abs().max()) + float(known.abs().max())
                bound = 8 * torch.finfo(torch.float32).eps * scale
                assert float((got - known)[hard].abs().max()) <= bound, f"{name} {kind}: pinned elements off known by more than {bound:.2e}"
    if plain is not None:  # one element per sample: a keep == 0 sample cannot feel the pin (batch independence)
        rest = keep == 0
        assert torch.equal(got[rest], plain[rest]), f"{name} {kind}: a keep == 0 sample changed under the pin of its batch-mates"


# ---- b: bounds and the record ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["heun", "lms"])
@pytest.mark.parametrize("name", E.NAMES)
def test_bounds_and_record_against_the_float64_loop(name, kind):
    model, state, goal, x, fixed = gpu_case(name, B)
    noise = native_rows(kind, x, fixed)
    for pinned in (False, True):
        lo, hi, want, seen, changed, plain = E.bounded(name, kind, B, pinned)
        gap = float((want - plain).abs().max())
        print(f"{name} {kind} pin={pinned}: clip_output changed {[round(c, 3) for c in changed]}; |clamped - unclamped| max {gap:.4f}")
        assert len(changed) == E.N and min(changed) >= 0.10, changed
        assert gap > 100 * E.tol_of(want)
        kw = dict(E.KINDS[kind], noise=noise, bounds=(lo, hi))
        if pinned:
            kw["pin"], keep, known = pinned_reference(name, kind, B)[:3]
        with torch.no_grad():
            out, rec = model.sample_native(kind, state, x, goal, E.sched(), record=True, **kw)
            bare = model.sample_native(kind, state, x, goal, E.sched(), **kw)
        assert torch.equal(out, bare), f"{name} {kind} pin={pinned}: record=True changed the actions"
        assert_close(out.cpu(), want, what=f"{name} {kind} pin={pinned}: actions")
        assert rec["x"].shape == rec["denoised"].shape == (E.N,) + tuple(x.shape)
        for i, (xs, den) in enumerate(seen):
            assert_close(rec["x"][i].cpu(), xs, what=f"{name} {kind} pin={pinned}: x[{i}]")
            assert_close(rec["denoised"][i].cpu(), den, what=f"{name} {kind} pin={pinned}: denoised[{i}]")
            if pinned:
                assert torch.equal(rec["denoised"][i].cpu()[keep == 1], known[keep == 1]), "the recorded denoised is not D'"
        assert bool((out.cpu() >= lo).all()) and bool((out.cpu() <= hi).all())


# ---- c: the guided plan head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["heun", "dpmpp_2m"])
@pytest.mark.parametrize("name", E.GUIDED_NAMES)
def test_guided_plan_head_against_the_float64_loop(name, kind, monkeypatch):
    tol = guid.tol(E.LAM)
    pin, keep, known, want_pinned, want = pinned_reference(name, kind, B, lam=E.LAM, **tol)
    unguided = E.loops(name, kind, B)[0]
    assert float((want - unguided).abs().max()) > 100 * E.tol_of(want, tol["atol"], tol["rtol"]), "guidance changes too little"
    model, state, goal, x, fixed = gpu_case(name, B)
    no_forward(monkeypatch)
    got = E.run(kind, model, state, x, goal, fixed, extra_args={"cond_lambda": E.LAM}).cpu()
    got_pinned = E.run(kind, model, state, x, goal, fixed, extra_args={"cond_lambda": E.LAM, "pin": pin}).cpu()
    print(f"{name} {kind}: max |native - float64| {float((got.double() - want).abs().max()):.3e} guided, "
          f"{float((got_pinned.double() - want_pinned).abs().max()):.3e} guided and pinned")
    assert_close(got, want, what=f"{name} guided {kind}", **tol)
    assert_close(got_pinned, want_pinned, what=f"{name} guided {kind} with a pin", **tol)
    if kind in SELECTS_LAST:
        assert torch.equal(got_pinned[keep == 1], known[keep == 1])


# ---- d: candidates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("name", E.NAMES)
def test_candidates_with_a_pin_against_the_expanded_float64_loop(name, kind, monkeypatch):
    K = 5
    pin, keep, known, want, _ = pinned_reference(name, kind, B, repeat=K)
    model, state, goal, x, fixed = gpu_case(name, B, repeat=K)
    assert x.shape[0] == B * K and goal.shape[0] == B
    no_forward(monkeypatch)
    got = E.run(kind, model, state, x, goal, fixed, extra_args={"candidates": K, "pin": pin}).cpu()
    print(f"{name} {kind} K={K}: max |native - float64| {float((got.double() - want).abs().max()):.3e}")
    assert_close(got, want, what=f"{name} {kind} (B, K) = ({B}, {K})")
    assert torch.equal(got[keep == 1], known[keep == 1])
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == B  # one context per observation


# ---- e: denoise_vjp --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_denoise_vjp_against_float64_autograd(name):
    model, state, goal, x_T, _ = gpu_case(name, B)
    st, g, _, _, _ = E.chunk_case(name, B)
    ref = E.oracle_of(name)
    act = -E.loops(name, "ddim", B)[1].float()  # a chunk the model produced
    v = torch.from_numpy(synthetic.normal("vjp_probe", tuple(act.shape), 5))
    for sig in (80.0, 1.0, 0.01):
        sigma = torch.full((B,), sig) * torch.linspace(0.8, 1.25, B)
        x = act + sigma[:, None, None] * x_T.cpu() / E.SMAX
        den, jtv = model.denoise_vjp(state, x.cuda(), goal, sigma.cuda(), v.cuda())
        d64, j64 = ref.vjp(E.wide(st), x, g.double(), sigma, v)
        print(f"{name} sigma={sig}: max |D - float64| {float((den.cpu().double() - d64).abs().max()):.3e}, max |J^T v - float64| "
              f"{float((jtv.cpu().double() - j64).abs().max()):.3e} (|J^T v| max {float(j64.abs().max()):.3e})")
        assert_close(den.cpu(), d64, what=f"{name} denoised sigma={sig}")
        assert_close(jtv.cpu(), j64, rtol=2e-3, atol=2e-3 * float(j64.abs().max()), what=f"{name} vjp sigma={sig}")


# ---- f: the steer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_one_steered_evaluation_against_float64_autograd(name):
    model, state, goal, x_T, _ = gpu_case(name, B)
    st, g, _, _, _ = E.chunk_case(name, B)
    ref, steer = E.oracle_of(name), E.steer_of(name, B)
    act = -steer.known
    for sigma in dict.fromkeys((80.0, E.SD * (E.BETA - 1) ** 0.5, 1.0)):  # (the kink of s(sigma) is at 1 for these values)
        x = act + sigma * x_T.cpu() / E.SMAX
        with torch.no_grad():
            got = model(state, x.cuda(), goal, torch.tensor([sigma], device="cuda"), steer=steer).cpu().double()
        want, d64, j64 = ref.steered(E.wide(st), x.double(), g.double(), torch.full((B,), sigma, dtype=torch.float64), steer)
        s = steer.scale(sigma, E.SD)
        tol = (ATOL + RTOL * d64.abs()) + s * (2e-3 * float(j64.abs().max()) + 2e-3 * j64.abs())
        err = (got - want).abs()
        print(f"{name} sigma={sigma:g}: s={s:g} max |D' - float64| {float(err.max()):.3e}, largest err / bound "
              f"{float((err / tol).max()):.3f}, max|D| {float(d64.abs().max()):.3e}, max|J^T e| {float(j64.abs().max()):.3e}")
        assert bool((err <= tol).all()), f"{name} sigma={sigma}: {int((err > tol).sum())}/{err.numel()} outside tau_D + s tau_J"


@pytest.mark.parametrize("name", E.NAMES)
def test_steered_ddim_against_the_float64_loop(name, monkeypatch):
    want, unsteered = E.steered_ddim(name, B)
    steer = E.steer_of(name, B)
    assert E.werr(steer, want) < E.werr(steer, unsteered)
    assert float((want - unsteered).abs().max()) > 100 * (1 + E.BETA) * E.tol_of(want)
    model, state, goal, x, _ = gpu_case(name, B)
    sig = gs.get_sigmas_exponential(3, E.STEER_SMIN, E.SMAX)
    no_forward(monkeypatch)
    with torch.no_grad():
        got = gs.sample_ddim(model, state, x, goal, sig, extra_args={"steer": steer}).cpu()
        plain = gs.sample_ddim(model, state, x, goal, sig).cpu()
    print(f"{name}: max |native - float64| {float((got.double() - want).abs().max()):.3e} (|want| max {float(want.abs().max()):.3f}); "
          f"weighted error {E.werr(steer, plain):.4e} -> {E.werr(steer, got):.4e}")
    assert_close(got, want, rtol=(1 + E.BETA) * RTOL, atol=(1 + E.BETA) * ATOL, what=f"{name}: steered DDIM")
    assert E.werr(steer, got) < E.werr(steer, plain)


# ---- g: the log-likelihood -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.LL_NAMES)
def test_log_likelihood_against_the_float64_host_loop(name, monkeypatch):
    Bk, K = 2, 3
    want_ll, want_latent, want_delta, winfo = E.loglik_reference(name, monkeypatch, Bk, K)
    state, goal, rows, v = E.loglik_case(name, Bk, K)
    model = model_of(name)[0]
    ll, latent, delta, info = model.log_likelihood(cuda(state), rows.cuda(), goal.cuda(), v.cuda()[None], E.LL_SMIN, E.LL_SMAX,
                                                   candidates=K)
    print(f"{name}: fevals {info['fevals']} (float64 {winfo['fevals']}); ll {[round(float(t), 3) for t in ll]} against "
          f"{[round(float(t), 3) for t in want_ll]}; max |latent - float64| {float((latent.cpu().double() - want_latent).abs().max()):.3e}, "
          f"|delta - float64| {float((delta.cpu().double() - want_delta).abs().max()):.3e}")
    assert ll.shape == (Bk * K,)
    assert_close(latent.cpu(), want_latent, rtol=RTOL, atol=ATOL * E.LL_SMAX, what=f"{name}: latent")
    assert_close(delta.cpu(), want_delta, what=f"{name}: delta", **LL)
    assert_close(ll.cpu(), want_ll, what=f"{name}: log-likelihood", **LL)
    assert 0.3 * winfo["fevals"] <= info["fevals"] <= 3 * winfo["fevals"]
    check_info(info)
