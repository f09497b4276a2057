"""sample_dpmpp_sde's default noise -- the Brownian tree -- on the MI355X (pytest -m gpu): mdt_brownian_noise against the host
helper, the reference's call form without a noise sampler as one native call (tree walked inside, mdt_sample_sde_tree*) against
the host loop driven by a NativeBrownianTreeNoiseSampler of the same seed, the same rows passed as a noise buffer, the random
stream, stream capture, graph replay, guidance and per-sample seeds."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.helpers import assert_close, cfg_of, inputs_of, load_fixture, params_of

pytestmark = pytest.mark.gpu

_MODELS = {}


def build(meta):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    key = (meta["config"], str(meta.get("overrides")), meta["weight_seed"], meta["profile"])
    if key not in _MODELS:
        model = GCDenoiser(cfg_of(meta), sigma_data=0.5)
        model.load_state_dict(params_of(meta), strict=True)
        _MODELS[key] = model.cuda().eval()
    return _MODELS[key]


def gpu_inputs(meta, B, seed):
    state, goal, noise = inputs_of(dict(meta, B=B, input_seed=seed))
    state = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    return state, goal.cuda(), noise.cuda()


def _no_forward(monkeypatch):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    monkeypatch.setattr(GCDenoiser, "forward", boom)


def _model():
    meta, _ = load_fixture("g3_b256_lang.npz")
    return meta, build(meta)


def _seed_of(k):
    """The seed the default noise sampler draws after torch.manual_seed(k)."""
    torch.manual_seed(k)
    return torch.randint(0, 2 ** 63 - 1, []).item()


def _loop_sampler(x, sig, seed):
    return gs.NativeBrownianTreeNoiseSampler(x, sig[sig > 0].min(), sig.max(), seed=seed)


def test_device_noise_equals_the_host_helper():
    lib = _lib.load()
    pairs = [(80.0, 35.2), (80.0, 12.5), (0.0123, 0.0041), (2.0, 80.0), (0.5, 0.5000001)]
    for seeds, batch, per_row in (([12345], 64, 70), ([7, 8, 9, 2 ** 62 + 1, 0], 5, 70), ([3], 256, 70)):
        want = _lib.brownian_noise_host(seeds, 0.001, 80.0, 1e-6, pairs, batch, per_row)
        sd = torch.tensor(seeds, dtype=torch.int64, device="cuda")
        out = torch.empty((len(pairs), batch, per_row), device="cuda")
        pr = (C.c_double * (2 * len(pairs)))(*[v for p in pairs for v in p])
        _lib.check(lib.mdt_brownian_noise(sd.data_ptr(), len(seeds), 0.001, 80.0, 1e-6, pr, len(pairs), batch, per_row,
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        got = out.cpu().numpy()
        d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert int(d.max()) <= 1, f"{seeds}: {int(d.max())} ulp"


CASES = [("exp", dict()), ("karras", dict(eta=0.5, s_noise=1.3, r=0.3)), ("exp", dict(eta=1., s_noise=0.8, r=0.3)),
         ("karras", dict(eta=0.5, r=0.5))]


def _points(sig, r):
    """The (from, to) points of every noise row of a dpmpp_sde call with eta != 0, as the plan records them: sigma(t),
    sigma(t + h r), sigma(t_next) with ln / exp rounded once from double."""
    f32 = np.float32
    out = []
    for i in range(len(sig) - 2):
        t, tn = f32(-math.log(float(sig[i]))), f32(-math.log(float(sig[i + 1])))
        s = f32(t + f32(f32(tn - t) * f32(r)))
        q = [f32(math.exp(-float(v))) for v in (t, s, tn)]
        out += [(float(q[0]), float(q[1])), (float(q[0]), float(q[2]))]
    return out


@pytest.mark.parametrize("B", [1, 7, 256])
def test_default_noise_runs_natively_and_matches_the_host_loop(B, monkeypatch):
    meta, model = _model()
    state, goal, noise = gpu_inputs(meta, B, 900 + B)
    g = gs
    x = noise * 80.0
    for k, (sched, kw) in enumerate(CASES):
        sig = (g.get_sigmas_exponential if sched == "exp" else g.get_sigmas_karras)(6, 0.001, 80.0)
        seed = _seed_of(k)
        with torch.no_grad():
            loop = g.sample_dpmpp_sde(model, state, x, goal, sig, noise_sampler=_loop_sampler(x, sig, seed),
                                      callback=lambda d: None, **kw)
            ns = _loop_sampler(x, sig, seed)
            rows = torch.stack([ns(a, b) for a, b in _points(sig, kw.get("r", 0.5))])
            as_rows = model.sample_native("dpmpp_sde", state, x, goal, sig, noise=rows, **kw)
            with monkeypatch.context() as mp:
                _no_forward(mp)
                for schedule in (sig, sig.cuda()):
                    torch.manual_seed(k)
                    got = g.sample_dpmpp_sde(model, state, x, goal, schedule, scaler=None, disable=True, **kw)
                    assert_close(got.cpu(), loop.cpu(), what=f"B={B} {sched}{kw} sigmas on {schedule.device}")
                    assert torch.equal(got, as_rows), f"B={B} {sched}{kw}: tree inside the call != the same rows passed in"


def test_seeded_calls_repeat_and_the_next_call_differs(monkeypatch):
    meta, model = _model()
    state, goal, noise = gpu_inputs(meta, 16, 31)
    g = gs
    sig = g.get_sigmas_exponential(10, 0.001, 80.0).cuda()
    _no_forward(monkeypatch)
    with torch.no_grad():
        torch.manual_seed(123)
        a = g.sample_dpmpp_sde(model, state, noise * 80.0, goal, sig)
        b = g.sample_dpmpp_sde(model, state, noise * 80.0, goal, sig)
        torch.manual_seed(123)
        c = g.sample_dpmpp_sde(model, state, noise * 80.0, goal, sig)
    assert torch.equal(a, c)
    assert not torch.equal(a, b)


def test_device_schedule_tree_call_captures_on_a_stream():
    meta, model = _model()
    state, goal, noise = gpu_inputs(meta, 4, 41)
    sig = gs.get_sigmas_karras(8, 0.001, 80.0).cuda()
    seeds = torch.tensor([_seed_of(5)], dtype=torch.int64, device="cuda")
    x = noise * 80.0
    with torch.no_grad():
        eager = model.sample_native("dpmpp_sde", state, x, goal, sig, tree=(seeds, 1e-6))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.sample_native("dpmpp_sde", state, x, goal, sig, tree=(seeds, 1e-6))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model.sample_native("dpmpp_sde", state, x, goal, sig, tree=(seeds, 1e-6))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_rollout_sized_calls_replay_with_each_calls_seed(monkeypatch):
    meta, model = _model()
    state, goal, noise = gpu_inputs(meta, 1, 51)
    g = gs
    sig = g.get_sigmas_exponential(10, 0.001, 80.0)
    model.__dict__.pop("_graphed_native", None)
    model.__dict__.pop("_graph_seen", None)
    outs = []
    with torch.no_grad():
        with monkeypatch.context() as mp:
            _no_forward(mp)
            for i in range(5):
                torch.manual_seed(200 + i)
                outs.append(g.sample_dpmpp_sde(model, state, noise * 80.0, goal, sig))
        graphs = model.__dict__.get("_graphed_native") or []
        assert any(gr.tree is not None for gr in graphs), "the repeated tree call did not build a graph"
        for i, o in enumerate(outs):
            seeds = torch.tensor([_seed_of(200 + i)], dtype=torch.int64, device="cuda")
            eager = model.sample_native("dpmpp_sde", state, noise * 80.0, goal, sig, tree=(seeds, 1e-6))
            assert torch.equal(o, eager), f"call {i}: replay != eager call with its seed"
    assert not torch.equal(outs[3], outs[4])


def test_guided_default_noise_is_native_and_matches_the_guided_host_loop(monkeypatch):
    meta, model = _model()
    state, goal, noise = gpu_inputs(meta, 3, 61)
    g = gs
    sig = g.get_sigmas_exponential(6, 0.01, 80.0)
    x = noise * 80.0
    lam = 2.0
    with torch.no_grad():
        loop = g.sample_dpmpp_sde(model, state, x, goal, sig, extra_args={"cond_lambda": lam}, callback=lambda d: None,
                                  noise_sampler=_loop_sampler(x, sig, _seed_of(9)))
        with monkeypatch.context() as mp:
            _no_forward(mp)
            torch.manual_seed(9)
            got = g.sample_dpmpp_sde(model, state, x, goal, sig, extra_args={"cond_lambda": lam})
    assert_close(got.cpu(), loop.cpu(), rtol=1e-3, atol=1e-4 * (abs(lam) + abs(1 - lam)), what="guided dpmpp_sde, tree noise")


def test_per_sample_seeds_through_the_sampler(monkeypatch):
    meta, model = _model()
    B = 7
    state, goal, noise = gpu_inputs(meta, B, 71)
    g = gs
    sig = g.get_sigmas_karras(6, 0.001, 80.0)
    x = noise * 80.0
    seeds = [1000 + 17 * b for b in range(B)]
    _no_forward(monkeypatch)
    with torch.no_grad():
        full = g.sample_dpmpp_sde(model, state, x, goal, sig, noise_sampler=_loop_sampler(x, sig, seeds))
        for b in (0, 3, 6):
            st = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in state.items()}
            one = g.sample_dpmpp_sde(model, st, x[b:b + 1], goal[b:b + 1], sig, noise_sampler=_loop_sampler(x[b:b + 1], sig, [seeds[b]]))
            assert_close(one.cpu(), full[b:b + 1].cpu(), what=f"sample {b}")
