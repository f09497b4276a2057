"""CPU-tier checks of ``ActionSteer`` (utils/action_steer.py) and of ``extra_args={"steer": ...}`` in the samplers: what the
constructor refuses, the overlap ramp against ``ActionPin.overlap``, the per-chunk / per-observation expansion, s(sigma) at its
ends and at its kink, the host loops over a foreign linear model against closed-form loops written here (the Jacobian of
D(x) = x @ M is M, so J^T e = e @ M^T), that steering lowers the weighted error, that an all-zero weight is no steer, which
combinations are refused by name, and which calls go to the native entry (a recorder stands in for the library)."""
import math
from contextlib import nullcontext

import pytest
import torch

from mdt_policy_amd import configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer

B, TA, A = 3, 10, 7


# ----------------------------------------------------------------------------------------------------------------
# the object
# ----------------------------------------------------------------------------------------------------------------
def test_validation_errors():
    known, w = torch.zeros(B, TA, A), torch.ones(TA)
    ActionSteer(known, w)
    for bad in (float("nan"), float("inf"), 0.0, -1.0):
        with pytest.raises(ValueError, match="beta"):
            ActionSteer(known, w, beta=bad)
    for bad in (torch.full((TA,), 1.5), torch.full((TA,), -0.1), torch.full((TA,), float("nan")), torch.zeros(0)):
        with pytest.raises(ValueError, match="weight must be finite and lie in"):
            ActionSteer(known, bad)
    with pytest.raises(ValueError, match="weight must be"):
        ActionSteer(known, torch.ones(1, B, TA, A))
    with pytest.raises(ValueError, match="known must be broadcastable"):
        ActionSteer(torch.zeros(1, B, TA, A), w)
    for bad in (float("nan"), float("inf")):
        k = known.clone()
        k[1, 2, 3] = bad
        with pytest.raises(ValueError, match="known must be finite"):
            ActionSteer(k, w)
    with pytest.raises(ValueError, match="do not fit"):
        ActionSteer(known, w).on("cpu", (B + 1, TA, A))
    with pytest.raises(ValueError, match="ActionSteer.overlap"):
        ActionSteer.overlap(torch.zeros(TA, A), 1, 2)
    assert ActionSteer(known, w).beta == 5.0 and ActionSteer(known, w).active
    assert not ActionSteer(known, torch.zeros(B, TA)).active


def test_the_accepted_weight_shapes_are_the_pins():
    known = torch.randn(B, TA, A)
    for w in (torch.rand(TA), torch.rand(B, TA), torch.rand(B, TA, 1), torch.rand(B, TA, A)):
        k1, w1 = ActionSteer(known, w).on("cpu", (B, TA, A))
        k2, w2 = ActionPin(known, w).on("cpu", (B, TA, A))
        assert torch.equal(k1, k2) and torch.equal(w1, w2) and w1.is_contiguous() and w1.dtype == torch.float32


@pytest.mark.parametrize("executed,hard,soft", [(0, 0, 0), (2, 3, 0), (2, 3, 4), (4, 2, 9), (12, 2, 2), (1, 0, 3)])
def test_overlap_has_the_pins_ramp(executed, hard, soft):
    prev = torch.randn(B, TA, A)
    s, p = ActionSteer.overlap(prev, executed, hard, soft, beta=3.0), ActionPin.overlap(prev, executed, hard, soft)
    assert torch.equal(s.weight, p.keep) and torch.equal(s.known, p.known) and s.beta == 3.0
    assert s.active == bool((p.keep != 0).any())


def test_on_expands_a_per_observation_steer_to_its_candidates():
    K = 4
    known, w = torch.randn(B, TA, A), torch.rand(B, TA)
    s = ActionSteer(known, w)
    k, wt = s.on("cpu", (B * K, TA, A), K)
    assert torch.equal(k, known.repeat_interleave(K, 0)) and torch.equal(wt, w[:, :, None].expand(B, TA, A).repeat_interleave(K, 0))
    per_chunk = ActionSteer(torch.randn(B * K, TA, A), torch.rand(TA))
    k, wt = per_chunk.on("cpu", (B * K, TA, A), K)
    assert torch.equal(k, per_chunk.known) and tuple(wt.shape) == (B * K, TA, A)
    with pytest.raises(ValueError, match="do not fit"):
        s.on("cpu", (B * K + 1, TA, A), K)


def test_scale_at_zero_at_the_kink_and_far_out():
    sd, beta = 0.5, 5.0
    s = ActionSteer(torch.zeros(1, TA, A), torch.ones(TA), beta)
    assert s.scale(0.0, sd) == 1.0
    kink = sd * math.sqrt(beta - 1)
    assert math.isclose(s.scale(kink, sd), beta, rel_tol=1e-15) and s.scale(kink, sd) <= beta
    assert math.isclose(s.scale(0.999 * kink, sd), 1 + (0.999 * kink / sd) ** 2, rel_tol=1e-15) and s.scale(0.999 * kink, sd) < beta
    assert s.scale(1.001 * kink, sd) == beta and s.scale(80.0, sd) == beta
    assert ActionSteer(torch.zeros(1, TA, A), torch.ones(TA), 1e9).scale(80.0, sd) == 1 + 80.0 ** 2 / sd ** 2


# ----------------------------------------------------------------------------------------------------------------
# the host loops over a foreign linear model, against closed forms
# ----------------------------------------------------------------------------------------------------------------
class Linear:
    """D(x; sigma) = x @ M on the action dimension: J^T e = e @ M^T.  sigma_data as _SteeredModel reads it.  M is 0.4 I plus a
    small perturbation: s M M^T stays below the identity up to s = beta = 5 (0.8), so D' moves the weighted tokens toward
    ``known`` without overshooting and the loops stay stable; at small sigma (s near 1) it still moves them by a sixth."""
    sigma_data = 0.5

    def __init__(self):
        g = torch.Generator().manual_seed(11)
        self.M = 0.4 * torch.eye(A, dtype=torch.float64) + 0.03 * torch.randn(A, A, dtype=torch.float64, generator=g)

    def __call__(self, state, x, goal, sigma):
        return x @ self.M


def _problem():
    g = torch.Generator().manual_seed(5)
    x = 80.0 * torch.randn(B, TA, A, dtype=torch.float64, generator=g)
    known = torch.randn(B, TA, A, dtype=torch.float64, generator=g).float().double()  # (a steer keeps fp32 values)
    steer = ActionSteer.overlap(known, 0, 3, 2)
    return x, known, steer, gs.get_sigmas_exponential(6, 0.01, 80.0)


def _steered(model, steer, x, sigma, known):
    """D' = D + s (W (y - D)) @ M^T, written out."""
    W = steer.weight.double()  # (1, Ta, 1)
    d = x @ model.M
    return d + steer.scale(sigma, model.sigma_data) * ((W * (known - d)) @ model.M.T)


def _closed_ddim(model, steer, x, known, sigmas):
    sig = sigmas.to(torch.float32)
    for i in range(len(sig) - 1):
        d = _steered(model, steer, x, float(sig[i]), known)
        t, tn = -sig[i].log(), -sig[i + 1].log()
        x = ((-tn).exp() / (-t).exp()).item() * x - (-(tn - t)).expm1().item() * d
    return x


def _closed_heun(model, steer, x, known, sigmas):
    sig = sigmas.to(torch.float32)
    for i in range(len(sig) - 1):
        s0, s1 = sig[i].item(), sig[i + 1].item()
        d = (x - _steered(model, steer, x, s0, known)) / s0
        dt = (sig[i + 1] - sig[i]).item()
        if s1 == 0:
            x = x + d * dt
        else:
            x2 = x + d * dt
            d2 = (x2 - _steered(model, steer, x2, s1, known)) / s1
            x = x + (d + d2) / 2 * dt
    return x


def _werr(steer, known, out):
    return float((steer.weight.double() * (known - out) ** 2).sum())


@pytest.mark.parametrize("name,closed", [("ddim", _closed_ddim), ("heun", _closed_heun)])
def test_host_loop_over_a_linear_model_equals_the_closed_form(name, closed):
    model = Linear()
    x, known, steer, sigmas = _problem()
    want = closed(model, steer, x, known, sigmas)
    got = getattr(gs, "sample_" + name)(model, {}, x, None, sigmas, extra_args={"steer": steer})
    assert got.dtype == torch.float64 and not got.requires_grad
    err = float((got - want).abs().max())
    scale = float(want.abs().max())
    assert err <= 1e-12 * max(scale, 1.0), (err, scale)  # float64 round-off of sums of O(80) terms
    # the closed form itself lowers the weighted error, and so does the sampler
    plain = getattr(gs, "sample_" + name)(model, {}, x, None, sigmas)
    zero = ActionSteer(known, torch.zeros(TA))
    want_plain = closed(model, zero, x, known, sigmas)
    assert _werr(steer, known, want) < _werr(steer, known, want_plain)
    assert _werr(steer, known, got) < _werr(steer, known, plain)


@pytest.mark.parametrize("name", ["ddim", "euler", "heun", "dpmpp_2m", "lms", "dpm_2", "dpmpp_2s"])
def test_an_all_zero_weight_returns_the_unsteered_bits(name):
    model = Linear()
    x, known, _, sigmas = _problem()
    zero = ActionSteer(known, torch.zeros(B, TA))
    fn = getattr(gs, "sample_" + name)
    torch.manual_seed(3)
    plain = fn(model, {}, x, None, sigmas)
    torch.manual_seed(3)
    got = fn(model, {}, x, None, sigmas, extra_args={"steer": zero})
    assert torch.equal(got, plain)


def test_every_sampler_takes_the_key():
    model = Linear()
    x, known, steer, sigmas = _problem()
    for name in ("ddim", "euler", "euler_ancestral", "heun", "dpm_2", "dpm_2_ancestral", "lms", "dpmpp_2m", "dpmpp_2_with_lms",
                 "dpmpp_2s", "dpmpp_2s_ancestral"):
        torch.manual_seed(1)
        a = getattr(gs, "sample_" + name)(model, {}, x, None, sigmas, extra_args={"steer": steer})
        torch.manual_seed(1)
        b = getattr(gs, "sample_" + name)(model, {}, x, None, sigmas)
        assert a.shape == x.shape and bool(torch.isfinite(a).all()) and not torch.equal(a, b), name
    ns = lambda s0, s1: torch.zeros_like(x)
    a = gs.sample_dpmpp_sde(model, {}, x, None, sigmas, extra_args={"steer": steer}, noise_sampler=ns)
    assert not torch.equal(a, gs.sample_dpmpp_sde(model, {}, x, None, sigmas, noise_sampler=ns))
    a = gs.sample_dpm_fast(model, {}, x, None, 0.01, 80.0, 6, extra_args={"steer": steer})
    assert not torch.equal(a, gs.sample_dpm_fast(model, {}, x, None, 0.01, 80.0, 6))
    a = gs.sample_dpm_adaptive(model, {}, x, None, 0.01, 80.0, extra_args={"steer": steer})
    assert not torch.equal(a, gs.sample_dpm_adaptive(model, {}, x, None, 0.01, 80.0))


def test_euler_without_churn_is_the_ddim_update():
    model = Linear()
    x, known, steer, sigmas = _problem()
    a = gs.sample_euler(model, {}, x, None, sigmas, extra_args={"steer": steer})
    b = gs.sample_ddim(model, {}, x, None, sigmas, extra_args={"steer": steer})
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())  # the schedule's fp32 coefficients, formed two ways


# ----------------------------------------------------------------------------------------------------------------
# refusals and routing with this package's denoiser (no device: the checks come first, a recorder stands in for the library)
# ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GCDenoiser(configs.mdtv_tiny(), 0.5).eval()


def _args():
    state = {"state_images": torch.randn(B, 3, 128), "modality": "lang"}
    return state, torch.randn(B, TA, A), torch.randn(B, 1, 512), gs.get_sigmas_exponential(4, 0.01, 80.0)


def _steer(weight=None):
    return ActionSteer(torch.randn(B, TA, A), torch.tensor([1.0, 1.0, 0.5] + [0.0] * (TA - 3)) if weight is None else weight)


@pytest.mark.parametrize("key,value", [("cond_lambda", 2.0), ("pin", ActionPin(torch.zeros(B, TA, A), torch.ones(TA)))])
def test_steer_with_guidance_or_a_pin_is_refused_by_name(model, key, value):
    state, x, goal, sig = _args()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match=key):
            model(state, x, goal, torch.tensor([1.0]), steer=_steer(), **{key: value})
    with pytest.raises(NotImplementedError, match=key):
        model.sample_ddim(state, x, goal, sig, steer=_steer(), **{key: value})
    for name in ("ddim", "euler", "heun", "dpmpp_2m"):
        with pytest.raises(NotImplementedError, match=key):
            getattr(gs, "sample_" + name)(model, state, x, goal, sig, extra_args={"steer": _steer(), key: value})
        with pytest.raises(NotImplementedError, match=key):
            getattr(gs, "sample_" + name)(Linear(), {}, x.double(), None, sig, extra_args={"steer": _steer(), key: value})
    with pytest.raises(NotImplementedError, match=key):
        gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args={"steer": _steer(), key: value})
    with pytest.raises(TypeError, match="ActionSteer"):
        gs.sample_ddim(model, state, x, goal, sig, extra_args={"steer": (torch.zeros(B, TA, A), torch.ones(TA))})


def test_cond_lambda_of_one_is_no_guidance(model, monkeypatch):
    seen = []
    monkeypatch.setattr(GCDenoiser, "_steered", lambda self, *a, **kw: seen.append(1) or a[1])
    state, x, goal, _ = _args()
    with torch.no_grad():
        model(state, x, goal, torch.tensor([1.0]), steer=_steer(), cond_lambda=1.0)
    assert seen == [1]


@pytest.fixture
def recorder(model, monkeypatch):
    calls = []

    def steered(self, state, action, goal, sigmas, steer, candidates=None, bounds=None):
        calls.append(("steer", candidates, bounds, tuple(action.shape)))
        return torch.zeros_like(action)

    def native(self, kind, state, action, goal, sigmas, noise=None, n_steps=None, **kw):
        calls.append(("native", kind, kw, tuple(action.shape)))
        return torch.zeros_like(action)

    def ddim(self, state, action, goal, sigmas, **kw):
        calls.append(("native", "ddim", kw, tuple(action.shape)))
        return torch.zeros_like(action)

    def forward(self, state, action, goal, sigma, **kw):
        calls.append(("forward", sorted(kw), None, tuple(action.shape)))
        return torch.zeros_like(action)

    monkeypatch.setattr(GCDenoiser, "sample_steered", steered)
    monkeypatch.setattr(GCDenoiser, "sample_native", native)
    monkeypatch.setattr(GCDenoiser, "sample_ddim", ddim)
    monkeypatch.setattr(GCDenoiser, "forward", forward)
    monkeypatch.setattr(GCDenoiser, "cached_context", lambda self, state, goal: nullcontext())
    monkeypatch.setattr(gs, "GraphedDDIM", None)  # a steered call never builds a graph
    monkeypatch.setattr(gs, "GraphedSampler", None)
    return calls


def test_ddim_and_churn_free_euler_go_to_the_native_call(model, recorder):
    state, x, goal, sig = _args()
    K = 2
    xk = torch.randn(B, K, TA, A)
    gs.sample_ddim(model, state, x, goal, sig, extra_args={"steer": _steer()})
    out = gs.sample_ddim(model, state, xk, goal, sig, extra_args={"steer": _steer(), "candidates": K})
    assert tuple(out.shape) == (B, K, TA, A)
    bounds = type("Bounds", (), {"clip_bounds": lambda self, device: (torch.zeros(A), torch.ones(A)),
                                 "clip_output": lambda self, a: a.clamp(0, 1)})()
    steer = _steer()
    state_before = torch.get_rng_state()
    gs.sample_euler(model, state, x, goal, sig, scaler=bounds, extra_args={"steer": steer})
    torch.set_rng_state(state_before)
    for _ in range(len(sig) - 1):
        torch.randn_like(x)  # the loop's draws
    after = torch.get_rng_state()
    torch.set_rng_state(state_before)
    gs.sample_euler(model, state, x, goal, sig, scaler=bounds, extra_args={"steer": steer})
    assert torch.equal(torch.get_rng_state(), after)
    assert [c[0] for c in recorder] == ["steer"] * 4
    assert recorder[0][1:3] == (1, None) and recorder[1][1] == K and recorder[1][3] == (B * K, TA, A)
    assert recorder[2][2] is bounds  # DDIM never clips; Euler's scaler rides in the call


def test_everything_else_keeps_the_host_loop_and_forward_gets_the_key(model, recorder):
    state, x, goal, sig = _args()
    steer = _steer()
    cases = [("ddim", dict(callback=lambda d: None)), ("ddim", dict(extra=dict(uncond=False))), ("euler", dict(s_churn=1.0)),
             ("euler", dict(scaler=type("Clip", (), {"clip_output": lambda self, a: a})())), ("heun", {}), ("dpmpp_2m", {}),
             ("lms", {}), ("dpm_2", {}), ("dpmpp_2s", {}), ("euler_ancestral", {}), ("dpm_2_ancestral", {}), ("dpmpp_2s_ancestral", {})]
    for name, kw in cases:
        del recorder[:]
        kw = dict(kw)
        ea = dict({"steer": steer}, **kw.pop("extra", {}))
        getattr(gs, "sample_" + name)(model, state, x, goal, sig, extra_args=ea, **kw)
        assert recorder and all(c[0] == "forward" and "steer" in c[1] for c in recorder), (name, recorder)
    del recorder[:]
    gs.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, 6, extra_args={"steer": steer})
    gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args={"steer": steer})
    gs.sample_dpmpp_sde(model, state, x, goal, sig, extra_args={"steer": steer}, noise_sampler=lambda a, b: torch.zeros_like(x))
    assert recorder and all(c[0] == "forward" and "steer" in c[1] for c in recorder)


def test_an_all_zero_weight_is_the_call_without_the_key(model, recorder):
    state, x, goal, sig = _args()
    zero = _steer(torch.zeros(TA))
    gs.sample_ddim(model, state, x, goal, sig, extra_args={"steer": zero})
    gs.sample_heun(model, state, x, goal, sig, extra_args={"steer": zero, "candidates": 1})
    assert [c[:2] for c in recorder] == [("native", "ddim"), ("native", "heun")]
    assert "steer" not in recorder[0][2] and "steer" not in recorder[1][2]
