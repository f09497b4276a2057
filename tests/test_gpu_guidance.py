"""Classifier-free guidance on the native samplers (pytest -m gpu): the guided sample_ddim against float64 composed from the
oracle's denoiser across configurations and the dispatcher's thresholds of the doubled batch, the other native kinds against
the guided host loop, lambda = 1 and goal-less models bit for bit, lambda = 0, batch independence and context, refusal, graph
replay keyed by the weight, and a plain C client.

D_lambda = D(x; sigma, 0) + lambda (D(x; sigma, g) - D(x; sigma, 0)); tolerance: rtol 1e-3, atol 1e-4 (|lambda| + |1 - lambda|)."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from oracle import mdt_oracle as O
from tests.envelope_configs import ENVELOPE
from tests.family import Family
from tests.helpers import assert_close, cuda  # noqa: F401 -- cuda: read as guid.cuda by other modules

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = dict(ENVELOPE)
CASES.update({
    "mdtv_default": dict(cfg=configs.mdtv_default(), arch="mdtv", proprio=False),
    "mdt_default": dict(cfg=configs.mdt_default(), arch="mdt", proprio=False),
    "rope": dict(cfg=configs.mdtv_default(use_rot_embed=True), arch="mdtv", proprio=False),
    "plain": dict(cfg=configs.mdtv_default(use_ada_conditioning=False), arch="mdtv", proprio=False),
    "noise_enc": dict(cfg=configs.mdtv_default(use_noise_encoder=True), arch="mdtv", proprio=False),
    "mlp_head": dict(cfg=configs.mdtv_default(linear_output=False), arch="mdtv", proprio=False),
    # no goal token: `uncond` changes nothing, a guided call is the unguided one
    "nogoal_proprio": dict(cfg=configs.mdtv_default(goal_conditioned=False), arch="mdtv", proprio=True),
    "mdt_nogoal": dict(cfg=configs.mdt_default(goal_conditioned=False, use_ada_conditioning=False), arch="mdt", proprio=False),
})
# Ta = 10 models: 2B samples cross 32 (B = 16 | 17), 64 (B = 39), 768 split rows (B = 39: 780) and 1401 rows (B = 72: 1440)
FULL = [1, 16, 17, 39, 72, 128]
BATCHES = {"mdtv_default": FULL, "mlp_head": [1, 17, 39, 72], "mdt_default": [1, 17, 39], "plain": [1, 17, 39],
           "h1_d64_min": [1, 17, 39, 800]}  # Ta = 1: 2B * 1 rows cross 1401 at B = 800
LAMBDAS = (0.0, 0.5, 3.0)


def tol(lam):
    return dict(rtol=1e-3, atol=1e-4 * (abs(lam) + abs(1 - lam)))


F = Family(None, CASES)   # (model, float32 state dict): 'rich' synthetic weights
model_of, inputs, _MODELS = F.model_of, F.inputs, F._models   # _MODELS: tests/test_sampler_envelope.py puts host weights in


def oracle_guided_ddim(name, B, seed, sig, lam):
    """The oracle's DDIM update around D_lambda, in float64."""
    e = CASES[name]
    _, P32 = model_of(name)
    P = O.to_dtype(P32, torch.float64)
    state, goal, noise = inputs(name, B, seed, torch.float64)
    x = noise * 80.0
    sig = sig.double()
    ones = x.new_ones([B])
    for i in range(len(sig) - 1):
        dg = O.denoise(P, e["cfg"], state, x, goal, sig[i] * ones, 0.5, e["arch"])
        du = O.denoise(P, e["cfg"], state, x, torch.zeros_like(goal), sig[i] * ones, 0.5, e["arch"])
        den = du + lam * (dg - du)
        t, t_next = sig[i].log().neg(), sig[i + 1].log().neg()
        x = (t_next.neg().exp() / t.neg().exp()) * x - (-(t_next - t)).expm1() * den
    return x


def _no_forward(monkeypatch):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    monkeypatch.setattr(GCDenoiser, "forward", boom)


GUIDED_NAMES = sorted(n for n in CASES if n not in ("nogoal_proprio", "mdt_nogoal"))


@pytest.mark.parametrize("name", GUIDED_NAMES)
def test_guided_ddim_against_float64(name, monkeypatch):
    """3-step guided sample_ddim at lambda 0 / 0.5 / 3 against float64 across the batches of BATCHES (default: 1 and 17)."""
    model, _ = model_of(name)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    _no_forward(monkeypatch)
    for j, B in enumerate(BATCHES.get(name, [1, 17])):
        lams = LAMBDAS if B <= 17 else (LAMBDAS[j % 3],)  # every weight at the small batches, one each above
        for lam in lams:
            state, goal, noise = inputs(name, B, 40 + B)
            want = oracle_guided_ddim(name, B, 40 + B, sig, lam)
            with torch.no_grad():
                got = gs.sample_ddim(model, cuda(state), noise.cuda() * 80.0, goal.cuda(), sig.cuda(),
                                       extra_args={"cond_lambda": lam}).cpu()
            assert_close(got, want, what=f"{name} B = {B} lambda = {lam}", **tol(lam))


@pytest.mark.parametrize("name", ["mdtv_default", "plain", "mlp_head", "mdt_default"])
def test_guided_ddim_graph_replay_is_keyed_by_lambda(name):
    """B = 1: calls 3 and 4 replay a graph; three calls with another weight capture their own graph, which stays correct."""
    model, _ = model_of(name)
    model.__dict__.pop("_graphed_samplers", None)
    model.__dict__.pop("_graph_seen", None)
    sig = gs.get_sigmas_exponential(10, 0.01, 80.0)
    seeds = (7, 8)
    for lam, calls in ((3.0, 4), (0.5, 3)):
        want = {s: oracle_guided_ddim(name, 1, s, sig, lam) for s in seeds}
        for i in range(calls):
            state, goal, noise = inputs(name, 1, seeds[i % 2])
            with torch.no_grad():
                got = gs.sample_ddim(model, cuda(state), noise.cuda() * 80.0, goal.cuda(), sig,
                                       extra_args={"cond_lambda": lam}).cpu()
            assert_close(got, want[seeds[i % 2]], what=f"{name} lambda {lam} call {i}", **tol(lam))
        assert any(g.cond_lambda == lam for g in model.__dict__.get("_graphed_samplers", [])), f"no graph for lambda {lam}"
    assert {g.cond_lambda for g in model._graphed_samplers} >= {3.0, 0.5}


OTHER_KINDS = [("euler", {}), ("heun", {}), ("dpm_2", {}), ("euler_ancestral", dict(eta=1.)), ("dpm_2_ancestral", dict(eta=1.)),
               ("dpmpp_2s_ancestral", dict(eta=1.)), ("lms", {}), ("dpmpp_2m", {}), ("dpmpp_2s", {}), ("dpmpp_sde", dict(eta=1.))]


@pytest.mark.parametrize("kind,kw", OTHER_KINDS)
@pytest.mark.parametrize("name", ["mdtv_default", "mlp_head"])
def test_other_kinds_guided_native_against_guided_host_loop(name, kind, kw, monkeypatch):
    model, _ = model_of(name)
    lam = 2.0
    B = 3
    state, goal, noise = inputs(name, B, 21)
    state = cuda(state)
    x, goal = noise.cuda() * 80.0, goal.cuda()
    sig = gs.get_sigmas_exponential(6, 0.01, 80.0)
    fn = getattr(gs, "sample_" + kind)
    kw = dict(kw)
    if kind == "dpmpp_sde":  # a seeded sampler: the native path draws its values up front in the loop's order
        kw["noise_sampler"] = lambda s0, s1: torch.randn(x.shape, device=x.device)
    with torch.no_grad():
        torch.manual_seed(3)
        loop = fn(model, state, x, goal, sig, extra_args={"cond_lambda": lam}, callback=lambda d: None, **kw).cpu()
        with monkeypatch.context() as mp:
            _no_forward(mp)
            torch.manual_seed(3)
            got = fn(model, state, x, goal, sig, extra_args={"cond_lambda": lam}, **kw).cpu()
    assert_close(got, loop, what=f"{name} {kind}", **tol(lam))


def test_dpm_fast_and_adaptive_guided_native_against_guided_host_loop(monkeypatch):
    model, _ = model_of("mdtv_default")
    lam = 2.0
    state, goal, noise = inputs("mdtv_default", 3, 22)
    state = cuda(state)
    x, goal = noise.cuda() * 80.0, goal.cuda()
    g = gs
    with torch.no_grad():
        for eta in (0.0, 1.0):
            kw = dict(eta=eta, noise_sampler=lambda s0, s1: torch.randn(x.shape, device=x.device))
            torch.manual_seed(4)
            loop = g.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, 10, extra_args={"cond_lambda": lam},
                                     callback=lambda d: None, **kw).cpu()
            with monkeypatch.context() as mp:
                _no_forward(mp)
                torch.manual_seed(4)
                got = g.sample_dpm_fast(model, state, x, goal, 0.01, 80.0, 10, extra_args={"cond_lambda": lam}, **kw).cpu()
            assert_close(got, loop, what=f"dpm_fast eta {eta}", **tol(lam))
        loop, li = g.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args={"cond_lambda": lam},
                                         callback=lambda d: None, return_info=True)
        with monkeypatch.context() as mp:
            _no_forward(mp)
            got, gi = g.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0, extra_args={"cond_lambda": lam}, return_info=True)
    assert gi["nfe"] == li["nfe"], (gi, li)
    assert_close(got.cpu(), loop.cpu(), what="dpm_adaptive", **tol(lam))


def _engine_call(model, state, x, goal, sig, lam):
    im = model.inner_model
    return model._engine(state=state).sample_ddim(state, x, im._goals(goal, False), sig, cond_lambda=lam)[0]


@pytest.mark.parametrize("name", ["mdtv_default", "mlp_head", "nogoal_proprio", "mdt_nogoal"])
def test_lambda_one_and_goal_less_models_give_the_unguided_bits(name):
    model, _ = model_of(name)
    state, goal, noise = inputs(name, 5, 23)
    state, x, goal = cuda(state), noise.cuda() * 80.0, goal.cuda()
    sig = gs.get_sigmas_exponential(5, 0.01, 80.0)
    with torch.no_grad():
        base = gs.sample_ddim(model, state, x, goal, sig)
        assert torch.equal(gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": 1.0}), base)
        assert torch.equal(_engine_call(model, state, x, goal, sig, 1.0), base)  # the C guided entry point at lambda = 1
        base_e = gs.sample_euler(model, state, x, goal, sig)
        assert torch.equal(gs.sample_euler(model, state, x, goal, sig, extra_args={"cond_lambda": 1.0}), base_e)
        if name in ("nogoal_proprio", "mdt_nogoal"):
            assert torch.equal(_engine_call(model, state, x, goal, sig, 2.0), base)
            assert torch.equal(gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": 2.0}), base)
            assert torch.equal(gs.sample_euler(model, state, x, goal, sig, extra_args={"cond_lambda": 2.0}), base_e)


@pytest.mark.parametrize("name", ["mdtv_default", "mdt_default"])
def test_lambda_zero_is_the_unconditional_model(name, monkeypatch):
    model, _ = model_of(name)
    state, goal, noise = inputs(name, 4, 24)
    state, x, goal = cuda(state), noise.cuda() * 80.0, goal.cuda()
    sig = gs.get_sigmas_exponential(5, 0.01, 80.0)
    with torch.no_grad():
        want = gs.sample_ddim(model, state, x, goal, sig, extra_args={"uncond": True}).cpu()
        with monkeypatch.context() as mp:
            _no_forward(mp)
            got = gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": 0.0}).cpu()
    assert_close(got, want, what=name)


@pytest.mark.parametrize("name", ["mdtv_default", "plain"])
def test_batch_independence_and_context(name):
    model, _ = model_of(name)
    lam = 2.5
    state, goal, noise = inputs(name, 3, 25)
    sig = gs.get_sigmas_exponential(4, 0.01, 80.0)
    im = model.inner_model
    with torch.no_grad():
        s3, x3, g3 = cuda(state), noise.cuda() * 80.0, goal.cuda()
        got = model.sample_ddim(s3, x3, g3, sig, cond_lambda=lam).cpu()
        ctx_g = im.latent_encoder_emb.clone()
        model.sample_ddim(s3, x3, g3, sig)
        ctx_u = im.latent_encoder_emb.clone()
        for b in range(3):
            sb = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in s3.items()}
            one = model.sample_ddim(sb, x3[b:b + 1], g3[b:b + 1], sig, cond_lambda=lam).cpu()
            assert_close(one, got[b:b + 1], what=f"{name} sample {b}", **tol(lam))
    assert ctx_g.shape == ctx_u.shape
    assert_close(ctx_g.cpu(), ctx_u.cpu(), rtol=1e-5, atol=1e-5, what=f"{name} context")


def test_non_finite_lambda_is_refused_and_the_handle_stays_usable():
    model, _ = model_of("mdtv_default")
    state, goal, noise = inputs("mdtv_default", 2, 26)
    state, x, goal = cuda(state), noise.cuda() * 80.0, goal.cuda()
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    tok = state["state_images"].contiguous()
    out = torch.empty_like(x)
    arr = (C.c_float * 4)(*[float(v) for v in sig])
    with torch.no_grad():
        eng = model._engine(state=state)
        lib = eng.lib
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError):
                gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": bad})
            with pytest.raises(ValueError):
                gs.sample_euler(model, state, x, goal, sig, extra_args={"cond_lambda": bad})
            with pytest.raises(ValueError):
                model(state, x, goal, sig[:1].cuda(), cond_lambda=bad)
            st = lib.mdt_sample_ddim_guided(eng.handle, tok.data_ptr(), None, goal.data_ptr(), _lib.MODALITY["lang"], x.data_ptr(),
                                            arr, 3, 2, out.data_ptr(), None, bad, eng._stream())
            assert st == 1, st  # MDT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            model(state, x, goal, sig[:1].cuda(), cond_lambda=2.0, uncond=True)
        want = oracle_guided_ddim("mdtv_default", 2, 26, sig, 2.0)
        got = gs.sample_ddim(model, state, x, goal, sig, extra_args={"cond_lambda": 2.0}).cpu()
    assert_close(got, want, what="after refusals", **tol(2.0))


def test_plain_c_client_matches_the_facade(tmp_path):
    exe = tmp_path / "guided_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "guided_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    B, n_steps, lam = 2, 5, 2.5
    state, goal, noise = inputs("mdtv_default", B, 27)
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    x_T = noise * 80.0
    blob = tmp_path / "blob.bin"
    allf = [n for n, _ in _lib.MDTConfig._fields_]
    names = allf[:allf.index("sigma_data")]
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        f.write(struct.pack(f"<{len(names)}i", *[getattr(cfg, n) for n in names]))
        f.write(struct.pack("<f", 0.5))
        sd = {"inner_model." + k: v for k, v in model.inner_model.state_dict().items()}
        wanted = list(model.inner_model.hip_engine(0.5).expected)
        f.write(struct.pack("<i", len(wanted)))
        for k in wanted:
            t = sd[k].detach().cpu().float().contiguous().numpy()
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", t.size) + t.tobytes())
        f.write(struct.pack("<ii", B, n_steps) + sig.numpy().astype(np.float32).tobytes())
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(struct.pack("<f", lam))
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape(tuple(x_T.shape))
    with torch.no_grad():
        want = gs.sample_ddim(model, cuda(state), x_T.cuda(), goal.cuda(), sig, extra_args={"cond_lambda": lam}).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    assert math.isfinite(float(np.abs(got).max()))
