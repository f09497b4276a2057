"""CPU-tier checks of where a steered sampler call goes (``extra_args = {"steer": ActionSteer}``, alone or with ``candidates``)
once the steer asks for the native plan call (``ActionSteer(..., plan_native=True)``; without the flag every one of these calls is
the host loop it was, which tests/test_action_steer.py pins and a test here repeats for every kind):
every fixed-step ``sample_<kind>`` on a GCDenoiser makes ONE call to ``GCDenoiser.sample_steered`` -- with its kind, its
parameters and as many noise rows as its unsteered native route draws -- and none to ``forward``, and leaves torch's generator
where the host loop (forced by a no-op ``callback``) leaves it; a callback, a scaler without bounds, a device schedule, ``pin`` /
``cond_lambda`` and sample_dpm_adaptive take the paths they took.  ``sample_steered`` and ``forward`` are recorders: no device."""
from contextlib import nullcontext

import pytest
import torch

from mdt_policy_amd import configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer

B, K, TA, A, N = 3, 2, 10, 7, 4
# name -> (the kind the native entry gets, the sampler's keyword arguments, the parameters that must arrive)
PLAN = {
    "euler churned": ("euler", dict(s_churn=1.0, s_noise=0.9), dict(s_churn=1.0, s_noise=0.9)),
    "heun": ("heun", {}, dict(s_churn=0.0)),
    "heun churned": ("heun", dict(s_churn=2.0, s_tmin=0.05, s_tmax=50.0), dict(s_churn=2.0, s_tmin=0.05, s_tmax=50.0)),
    "dpm_2": ("dpm_2", {}, dict(s_churn=0.0)),
    "lms": ("lms", {}, dict(order=4)),
    "lms order 1": ("lms", dict(order=1), dict(order=1)),
    "dpmpp_2m": ("dpmpp_2m", {}, {}),
    "dpmpp_2_with_lms": ("dpmpp_2m", {}, {}),
    "dpmpp_2s": ("dpmpp_2s", {}, {}),
    "euler_ancestral": ("euler_ancestral", {}, dict(eta=1.0)),
    "dpm_2_ancestral": ("dpm_2_ancestral", dict(eta=0.7), dict(eta=0.7)),
    "dpmpp_2s_ancestral": ("dpmpp_2s_ancestral", dict(s_noise=0.8), dict(eta=1.0, s_noise=0.8)),
    "dpmpp_sde": ("dpmpp_sde", {}, dict(eta=1.0, s_noise=1.0, r=0.5)),
    "dpmpp_sde sampled": ("dpmpp_sde", dict(noise_sampler="gauss"), dict(eta=1.0)),
    "dpm_fast": ("dpm_fast", {}, dict(eta=0.0)),
    "dpm_fast eta": ("dpm_fast", dict(eta=0.5), dict(eta=0.5)),
}


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GCDenoiser(configs.mdtv_tiny(), 0.5).eval()


@pytest.fixture
def recorder(model, monkeypatch):
    calls = []

    def steered(self, state, action, goal, sigmas, steer, candidates=None, bounds=None, kind=None, noise=None, n_steps=None,
                record=False, **params):
        calls.append(("steer", kind, dict(params, candidates=candidates, bounds=bounds, n_steps=n_steps), tuple(action.shape),
                      None if noise is None else tuple(noise.shape)))
        return torch.zeros_like(action)

    def native(self, kind, state, action, goal, sigmas, noise=None, n_steps=None, **kw):
        calls.append(("native", kind, kw, tuple(action.shape), None if noise is None else tuple(noise.shape)))
        return torch.zeros_like(action)

    def ddim(self, state, action, goal, sigmas, **kw):
        calls.append(("native", "ddim", kw, tuple(action.shape), None))
        return torch.zeros_like(action)

    def forward(self, state, action, goal, sigma, **kw):
        calls.append(("forward", None, kw, tuple(action.shape), None))
        return torch.zeros_like(action)

    monkeypatch.setattr(GCDenoiser, "sample_steered", steered)
    monkeypatch.setattr(GCDenoiser, "sample_native", native)
    monkeypatch.setattr(GCDenoiser, "sample_ddim", ddim)
    monkeypatch.setattr(GCDenoiser, "forward", forward)
    monkeypatch.setattr(GCDenoiser, "cached_context", lambda self, state, goal: nullcontext())
    monkeypatch.setattr(gs, "GraphedDDIM", None)  # a steered call never builds a graph
    monkeypatch.setattr(gs, "GraphedSampler", None)
    monkeypatch.setattr(gs, "_torchsde_available", lambda: False)  # the default noise of dpmpp_sde: the library's own tree
    return calls


def _inputs(shape=(B, TA, A)):
    g = torch.Generator().manual_seed(11)
    state = {"state_images": torch.randn(B, 3, 128, generator=g), "modality": "lang"}
    return state, torch.randn(*shape, generator=g), torch.randn(B, 1, 512, generator=g), gs.get_sigmas_exponential(N, 0.01, 80.0)


def _steer(plan_native=True):
    g = torch.Generator().manual_seed(12)
    return ActionSteer(torch.randn(B, TA, A, generator=g), torch.tensor([1.0, 1.0, 0.5] + [0.0] * (TA - 3)), plan_native=plan_native)


def _call(name, model, extra_args, shape=(B, TA, A), sigmas=None, **kw):
    kind, own, _ = PLAN.get(name, (name, {}, {}))
    kw = dict(own, **kw)
    if kw.get("noise_sampler") == "gauss":
        kw["noise_sampler"] = lambda s0, s1: torch.randn(*shape)
    state, x, goal, sig = _inputs(shape)
    sig = sig if sigmas is None else sigmas
    if kind == "dpm_fast":
        return gs.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, 6, extra_args=extra_args, **kw)
    if kind == "dpm_adaptive":
        return gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args=extra_args, **kw)
    fn = "dpmpp_2_with_lms" if name == "dpmpp_2_with_lms" else kind
    return getattr(gs, "sample_" + fn)(model, state, x, goal, sig, extra_args=extra_args, **kw)


@pytest.mark.parametrize("with_candidates", [False, True], ids=["alone", "candidates"])
@pytest.mark.parametrize("name", sorted(PLAN))
def test_a_steered_sampler_is_one_native_call_with_the_unsteered_routes_rows(name, with_candidates, model, recorder):
    kind, _, want = PLAN[name]
    shape = (B * K, TA, A) if with_candidates else (B, TA, A)
    ea = {"candidates": K} if with_candidates else {}
    # what the unsteered native route hands its entry, and where it leaves the generator
    torch.manual_seed(21)
    _call(name, model, dict(ea) or None, shape)
    plain, after_plain = list(recorder), torch.get_rng_state()
    assert [c[0] for c in plain] == ["native"] and plain[0][1] == kind, plain
    del recorder[:]
    # where the host loop leaves it under the steer (a no-op callback forces the loop)
    torch.manual_seed(21)
    _call(name, model, dict(ea, steer=_steer()), shape, callback=lambda d: None)
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder
    after_loop = torch.get_rng_state()
    del recorder[:]
    # the steered call
    torch.manual_seed(21)
    out = _call(name, model, dict(ea, steer=_steer()), shape)
    assert [c[0] for c in recorder] == ["steer"], recorder  # one call, none to forward
    _, got_kind, kw, got_shape, rows = recorder[0]
    assert got_kind == kind and got_shape == shape and tuple(out.shape) == shape
    assert kw["candidates"] == (K if with_candidates else 1)
    assert kw["n_steps"] == (6 if kind == "dpm_fast" else None)
    for key, value in want.items():
        assert kw[key] == value, (key, kw)
    if kind == "dpmpp_sde" and "sampled" not in name:  # the unsteered route walks its tree inside the call: its 2 (n - 1) rows
        assert plain[0][2].get("tree") is not None and rows == (2 * (N - 1),) + shape
    else:
        assert rows == plain[0][4], (rows, plain[0][4])  # as many noise rows, in the chunks' shape
    assert torch.equal(torch.get_rng_state(), after_loop)
    assert torch.equal(after_plain, after_loop)


@pytest.mark.parametrize("name", sorted(PLAN))
def test_without_the_flag_a_steered_sampler_keeps_its_host_loop(name, model, recorder):
    """The default: what these calls did before the native entry existed, alone and with ``candidates``."""
    assert not _steer(plan_native=False).plan_native and not ActionSteer(torch.zeros(B, TA, A), torch.ones(TA)).plan_native
    _call(name, model, {"steer": _steer(plan_native=False)})
    _call(name, model, {"steer": _steer(plan_native=False), "candidates": K}, (B * K, TA, A))
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder


def test_overlap_passes_the_flag_on():
    prev = torch.randn(B, TA, A)
    assert ActionSteer.overlap(prev, 2, 3, 2, plan_native=True).plan_native and not ActionSteer.overlap(prev, 2, 3, 2).plan_native


def test_the_tree_rows_are_the_host_loops(model, recorder, monkeypatch):
    """sample_dpmpp_sde without a noise_sampler: the rows come from the NativeBrownianTreeNoiseSampler the host loop constructs
    (one seed drawn from torch's generator), read at the loop's points."""
    seen = []
    monkeypatch.setattr(GCDenoiser, "sample_steered",
                        lambda self, state, action, goal, sigmas, steer, noise=None, **kw: seen.append(noise) or torch.zeros_like(action))
    torch.manual_seed(31)
    _call("dpmpp_sde", model, {"steer": _steer()})
    torch.manual_seed(31)
    state, x, goal, sig = _inputs()
    tree = gs.NativeBrownianTreeNoiseSampler(x, sig[sig > 0].min(), sig.max())
    want = []
    for i in range(N - 1):
        t, tn = -sig[i].log(), -sig[i + 1].log()
        s = t + (tn - t) * 0.5
        want += [tree((-t).exp(), (-s).exp()), tree((-t).exp(), (-tn).exp())]
    assert len(seen) == 1 and torch.equal(seen[0], torch.stack(want))


def test_ddim_and_churn_free_euler_keep_the_ddim_call(model, recorder):
    _call("ddim", model, {"steer": _steer()})
    _call("euler", model, {"steer": _steer(), "candidates": K}, (B, K, TA, A))
    assert [(c[0], c[1]) for c in recorder] == [("steer", None), ("steer", None)]
    assert recorder[1][2]["candidates"] == K and recorder[1][3] == (B * K, TA, A) and recorder[1][4] is None


def test_bounds_ride_where_the_loop_reads_its_scaler(model, recorder):
    bounds = type("Bounds", (), {"clip_bounds": lambda self, device: (torch.zeros(A), torch.ones(A)),
                                 "clip_output": lambda self, a: a.clamp(0, 1)})()
    for name in ("heun", "lms", "dpmpp_sde sampled", "euler_ancestral"):
        _call(name, model, {"steer": _steer()}, scaler=bounds)
        assert recorder[-1][0] == "steer" and recorder[-1][2]["bounds"] is bounds, name
    for name in ("dpmpp_2m", "dpm_fast"):  # accepted and never read, as in the loops
        _call(name, model, {"steer": _steer()}, scaler=bounds)
        assert recorder[-1][0] == "steer" and recorder[-1][2]["bounds"] is None, name


@pytest.mark.parametrize("name", sorted(PLAN) + ["ddim", "dpm_adaptive"])
def test_a_callback_keeps_the_host_loop(name, model, recorder):
    _call(name, model, {"steer": _steer()}, callback=lambda d: None)
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m", "lms", "euler_ancestral", "dpmpp_sde sampled"])
def test_a_scaler_without_bounds_and_a_further_key_keep_the_host_loop(name, model, recorder):
    clip = type("Clip", (), {"clip_output": lambda self, a: a})()
    _call(name, model, {"steer": _steer()}, scaler=clip)
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder
    del recorder[:]
    _call(name, model, {"steer": _steer(), "uncond": False})
    assert recorder and all(c[0] == "forward" and "steer" in c[2] and "uncond" in c[2] for c in recorder), recorder


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m", "dpm_2_ancestral"])
def test_a_device_schedule_keeps_the_host_loop(name, model, recorder, monkeypatch):
    class OnDevice(torch.Tensor):  # a schedule that says it lives on the GPU (there is none here): what the routes ask it
        @property
        def device(self):
            return torch.device("cuda", 0)

    sig = gs.get_sigmas_exponential(N, 0.01, 80.0)
    monkeypatch.setattr(gs, "_host", lambda s: torch.tensor([float(v) for v in s], dtype=torch.float32))
    _call(name, model, {"steer": _steer()}, sigmas=sig.as_subclass(OnDevice))
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder


def test_sample_dpm_adaptive_keeps_the_host_loop(model, recorder):
    _call("dpm_adaptive", model, {"steer": _steer()})
    assert recorder and all(c[0] == "forward" and "steer" in c[2] for c in recorder), recorder


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m", "dpm_fast", "dpmpp_sde sampled"])
def test_pin_and_guidance_are_still_refused(name, model, recorder):
    pin = ActionPin(torch.randn(B, TA, A), torch.tensor([1.0] + [0.0] * (TA - 1)))
    with pytest.raises(NotImplementedError, match="pin"):
        _call(name, model, {"steer": _steer(), "pin": pin})
    with pytest.raises(NotImplementedError, match="cond_lambda"):
        _call(name, model, {"steer": _steer(), "cond_lambda": 2.0})
    assert recorder == []


def test_an_all_zero_weight_is_the_unsteered_native_call(model, recorder):
    zero = ActionSteer(torch.randn(B, TA, A), torch.zeros(TA), plan_native=True)
    for name in ("heun", "dpmpp_2m", "dpm_fast"):
        _call(name, model, {"steer": zero})
    assert [(c[0], c[1]) for c in recorder] == [("native", "heun"), ("native", "dpmpp_2m"), ("native", "dpm_fast")]
    assert all("steer" not in c[2] for c in recorder)
