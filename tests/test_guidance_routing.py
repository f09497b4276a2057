"""CPU-tier checks of classifier-free guidance: which sampler calls take the guided native call (extra_args = {"cond_lambda": lam}
alone), which keep the host loop, that lambda = 1 is today's unguided call, the guided GCDenoiser.forward composition, and the
new C-ABI symbols with their ctypes prototypes."""
import ctypes as C
import os
import re
from contextlib import nullcontext

import pytest
import torch

from mdt_policy_amd import _lib, configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUIDED = ["mdt_sample_ddim_guided", "mdt_sample_ddim_dev_guided", "mdt_sample_guided", "mdt_sample_dev_guided",
          "mdt_sample_dpm_adaptive_guided"]
B, TA, A = 2, 10, 7


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GCDenoiser(configs.mdtv_default(), 0.5).eval()


@pytest.fixture
def recorder(model, monkeypatch):
    """Every native entry point and the per-step denoiser replaced by recorders (no device needed)."""
    calls = []

    def native(self, kind, state, action, goal, sigmas, noise=None, n_steps=None, **kw):
        calls.append(("native", kind, kw))
        return torch.zeros_like(action)

    def ddim(self, state, action, goal, sigmas, **kw):
        calls.append(("native", "ddim", kw))
        return torch.zeros_like(action)

    def adaptive(self, state, action, goal, sigma_min, sigma_max, **kw):
        calls.append(("native", "dpm_adaptive", kw))
        return torch.zeros_like(action), {}

    def forward(self, state, action, goal, sigma, **kw):
        calls.append(("forward", None, kw))
        return torch.zeros_like(action)

    monkeypatch.setattr(GCDenoiser, "sample_native", native)
    monkeypatch.setattr(GCDenoiser, "sample_ddim", ddim)
    monkeypatch.setattr(GCDenoiser, "sample_dpm_adaptive_native", adaptive)
    monkeypatch.setattr(GCDenoiser, "forward", forward)
    monkeypatch.setattr(GCDenoiser, "cached_context", lambda self, state, goal: nullcontext())
    return calls


def _args():
    state = {"state_images": torch.zeros(B, 3, 512), "modality": "lang"}
    return state, torch.randn(B, TA, A), torch.zeros(B, 1, 512), gs.get_sigmas_exponential(4, 0.01, 80.0)


FIXED = ["ddim", "euler", "euler_ancestral", "heun", "dpm_2", "dpm_2_ancestral", "lms", "dpmpp_2m", "dpmpp_2_with_lms", "dpmpp_2s",
         "dpmpp_2s_ancestral", "dpmpp_sde"]


def _call(name, model, extra_args):
    state, x, goal, sig = _args()
    if name == "dpm_fast":
        return gs.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, 6, extra_args=extra_args)
    if name == "dpm_adaptive":
        return gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args=extra_args)
    kw = {"noise_sampler": lambda s0, s1: torch.zeros(B, TA, A)} if name == "dpmpp_sde" else {}
    return getattr(gs, "sample_" + name)(model, state, x, goal, sig, extra_args=extra_args, **kw)


@pytest.mark.parametrize("name", FIXED + ["dpm_fast"])
def test_cond_lambda_alone_reaches_the_guided_native_call(name, model, recorder):
    _call(name, model, {"cond_lambda": 2.0})
    assert recorder and all(c[0] == "native" for c in recorder), recorder
    assert recorder[-1][2].get("cond_lambda") == 2.0, recorder


@pytest.mark.parametrize("name", FIXED + ["dpm_fast", "dpm_adaptive"])
def test_other_keys_keep_the_host_loop(name, model, recorder):
    _call(name, model, {"cond_lambda": 2.0, "s_churn": 0})
    assert recorder and all(c[0] == "forward" for c in recorder), recorder
    assert all(c[2] == {"cond_lambda": 2.0, "s_churn": 0} for c in recorder)


@pytest.mark.parametrize("name", FIXED + ["dpm_fast"])
def test_lambda_one_takes_the_unguided_native_call(name, model, recorder):
    _call(name, model, {"cond_lambda": 1.0})
    unguided = list(recorder)
    recorder.clear()
    _call(name, model, None)
    assert unguided == recorder and all("cond_lambda" not in c[2] for c in recorder), unguided


def test_forward_composes_the_guided_denoiser(model, monkeypatch):
    vals = {False: torch.full((B, TA, A), 3.0), True: torch.full((B, TA, A), 1.0)}
    seen = []

    def base(self, state, action, goal, sigma, cond_lambda=1.0, **kw):
        if float(cond_lambda) != 1.0:
            return orig(self, state, action, goal, sigma, cond_lambda=cond_lambda, **kw)
        seen.append(bool(kw.get("uncond", False)))
        return vals[bool(kw.get("uncond", False))]
    orig = GCDenoiser.forward
    monkeypatch.setattr(GCDenoiser, "forward", base)
    state, x, goal, _ = _args()
    out = model(state, x, goal, torch.ones(1), cond_lambda=2.5)
    assert torch.equal(out, torch.full((B, TA, A), 1.0 + 2.5 * 2.0))
    assert seen == [True, False]  # the unconditional evaluation first: latent_encoder_emb ends as the conditional context
    with pytest.raises(ValueError):
        model(state, x, goal, torch.ones(1), cond_lambda=2.0, uncond=True)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            model(state, x, goal, torch.ones(1), cond_lambda=bad)


def test_non_finite_lambda_is_refused_before_the_library(model, monkeypatch):
    monkeypatch.setattr(GCDenoiser, "cached_context", lambda self, state, goal: nullcontext())
    state, x, goal, sig = _args()
    with pytest.raises(ValueError):
        gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": float("nan")})


def test_guided_symbols_are_exported_with_matching_prototypes():
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip.h")).read(), flags=re.S)
    table = {n: argt for n, _, argt in _lib.SYMBOLS}
    for name in GUIDED:
        assert hasattr(lib, name), name
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/mdt_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        unguided = re.search(r"\b" + name.replace("_guided", "") + r"\s*\(([^)]*)\)\s*;", hdr).group(1)
        ua = [a.strip() for a in unguided.split(",")]
        # the unguided twin's arguments plus `float cond_lambda` (before the info pointer and the stream)
        assert [a for a in args if a != "float cond_lambda"] == ua, name
        assert "float cond_lambda" in args
        assert len(table[name]) == len(args)
        assert table[name][args.index("float cond_lambda")] is C.c_float, name
