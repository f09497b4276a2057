"""The other samplers' native path on the MI355X (pytest -m gpu): GCDenoiser.sample_native / mdt_sample against the reference's
goldens with the per-step denoiser disabled, against the host loop (forced with a no-op callback) across conditioning variants,
batch sizes and host / device schedules, the random stream, and HIP-graph capture and replay."""
import pytest
import torch

from mdt_policy_amd import synthetic
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


def gpu_inputs(meta, B=None, seed=None):
    m = dict(meta) if B is None else dict(meta, B=B, input_seed=seed)
    state, goal, noise = inputs_of(m)
    state = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    return state, goal.cuda(), noise.cuda()


def _no_forward(monkeypatch):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    monkeypatch.setattr(GCDenoiser, "forward", boom)


def _host_loop(fn, *args, **kw):
    return fn(*args, callback=lambda d: None, **kw)


# every routed sampler with deterministic settings
DETERMINISTIC = [("euler", {}), ("heun", {}), ("dpm_2", {}), ("euler_ancestral", dict(eta=0.)), ("dpm_2_ancestral", dict(eta=0.)),
                 ("dpmpp_2m", {}), ("dpmpp_2_with_lms", {}), ("dpmpp_2s", {}), ("dpmpp_2s_ancestral", dict(eta=0.)),
                 ("lms", {}), ("lms", dict(order=2)), ("dpmpp_sde", dict(eta=0., noise_sampler=lambda s0, s1: None))]  # never called at eta 0


@pytest.mark.parametrize("sched", ["exp", "karras"])
@pytest.mark.parametrize("name", ["euler", "heun", "dpmpp_2m"])
def test_g7_goldens_on_the_native_path(name, sched, monkeypatch):
    meta, fx = load_fixture("g7_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    g = gs
    sig = (g.get_sigmas_exponential if sched == "exp" else g.get_sigmas_karras)(10, 0.001, 80.0)
    with torch.no_grad():
        out = getattr(g, "sample_" + name)(model, state, noise * 80.0, goal, sig)
    assert_close(out.cpu(), fx[f"{name}_{sched}"], what=f"{name}/{sched}")


@pytest.mark.parametrize("name,kw,key", [
    ("lms", {}, "lms"), ("dpm_2", {}, "dpm_2"), ("dpmpp_2_with_lms", {}, "dpmpp_2_with_lms"), ("dpmpp_2s", {}, "dpmpp_2s"),
    ("euler_ancestral", dict(eta=0.), "euler_ancestral_eta0"), ("dpm_2_ancestral", dict(eta=0.), "dpm_2_ancestral_eta0"),
    ("dpmpp_2s_ancestral", dict(eta=0.), "dpmpp_2s_ancestral_eta0")])
def test_g7b_goldens_on_the_native_path(name, kw, key, monkeypatch):
    meta, fx = load_fixture("g7b_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    g = gs
    with torch.no_grad():
        out = getattr(g, "sample_" + name)(model, state, noise * 80.0, goal, g.get_sigmas_exponential(10, 0.001, 80.0), **kw)
    assert_close(out.cpu(), fx[key], what=key)


def test_g7c_dpmpp_sde_goldens_on_the_native_path(monkeypatch):
    meta, fx = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    g = gs
    x0 = noise * 80.0
    fixed = torch.from_numpy(synthetic.normal("sde_noise", tuple(x0.shape), meta["noise_seed"])).cuda()
    sig = g.get_sigmas_exponential(10, 0.001, 80.0)
    with torch.no_grad():
        for eta, key in ((0., "dpmpp_sde_eta0"), (1., "dpmpp_sde_eta1_fixednoise")):
            out = g.sample_dpmpp_sde(model, state, x0.clone(), goal, sig, eta=eta, noise_sampler=lambda s0, s1: fixed)
            assert_close(out.cpu(), fx[key], what=key)


@pytest.mark.parametrize("variant", ["g8_no_ada", "g8_noise_block", "g8_mlp_head", "g8_mdt_no_ada", "g8_mdt_mlp_head",
                                     "g3_b8_mdt"])
def test_native_matches_the_host_loop_on_the_conditioning_variants(variant):
    meta, _ = load_fixture(f"{variant}.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    g = gs
    sig = g.get_sigmas_karras(5, 0.01, 80.0)
    im = model.inner_model
    with torch.no_grad():
        for name, kw in DETERMINISTIC:
            fn = getattr(g, "sample_" + name)
            want = _host_loop(fn, model, state, noise * 80.0, goal, sig, **kw)
            want_ctx = im.latent_encoder_emb.clone()
            got = fn(model, state, noise * 80.0, goal, sig, **kw)
            assert_close(got.cpu(), want.cpu(), what=f"{variant}/{name}{kw}")
            assert_close(im.latent_encoder_emb.cpu(), want_ctx.cpu(), what=f"{variant}/{name} ctx")


@pytest.mark.parametrize("B", [1, 16, 77, 300, 513])
def test_native_matches_the_host_loop_across_batch_sizes_and_schedule_placement(B):
    meta, _ = load_fixture("g3_b256_lang.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta, B=B, seed=300 + B)
    g = gs
    sig = g.get_sigmas_exponential(6, 0.001, 80.0)
    with torch.no_grad():
        for name, kw in DETERMINISTIC + [("euler_ancestral", dict(eta=1.)), ("heun", dict(s_churn=1.0))]:
            fn = getattr(g, "sample_" + name)
            torch.manual_seed(B)
            want = _host_loop(fn, model, state, noise * 80.0, goal, sig, **kw)
            for schedule in (sig, sig.cuda()):
                torch.manual_seed(B)
                got = fn(model, state, noise * 80.0, goal, schedule, **kw)
                assert_close(got.cpu(), want.cpu(), what=f"B={B} {name}{kw} sigmas on {schedule.device}")


@pytest.mark.parametrize("name,kw", [("euler_ancestral", dict(eta=1.)), ("dpm_2_ancestral", dict(eta=1.)),
                                     ("dpmpp_2s_ancestral", dict(eta=1.)), ("heun", dict(s_churn=2.0, s_noise=1.01)),
                                     ("euler", dict(s_churn=1.0))])
def test_seeded_native_call_follows_the_host_loops_random_stream(name, kw):
    meta, _ = load_fixture("g7b_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    g = gs
    fn = getattr(g, "sample_" + name)
    sig = g.get_sigmas_exponential(10, 0.001, 80.0)
    with torch.no_grad():
        torch.manual_seed(1234)
        want = _host_loop(fn, model, state, noise * 80.0, goal, sig, **kw)
        after_loop = torch.randn(5, device="cuda")
        torch.manual_seed(1234)
        got = fn(model, state, noise * 80.0, goal, sig, **kw)
        after_native = torch.randn(5, device="cuda")
    assert_close(got.cpu(), want.cpu(), what=name)
    assert torch.equal(after_native, after_loop), "the native call left the generator elsewhere than the host loop"


def test_device_schedule_call_captures_into_a_graph_and_replays_equal_to_eager():
    meta, _ = load_fixture("g7_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    g = gs
    sig = g.get_sigmas_karras(10, 0.001, 80.0).cuda()
    x = noise * 80.0
    with torch.no_grad():
        eager = model.sample_native("heun", state, x, goal, sig)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model.sample_native("heun", state, x, goal, sig)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model.sample_native("heun", state, x, goal, sig)
        sig.copy_(g.get_sigmas_exponential(10, 0.001, 80.0).cuda())  # read at replay time
        graph.replay()
        torch.cuda.synchronize()
        want = model.sample_native("heun", state, x, goal, sig)
    assert torch.equal(out, want)
    assert not torch.equal(out, eager)


@pytest.mark.parametrize("name,kw,deterministic", [("heun", {}, True), ("dpmpp_2m", {}, True), ("lms", {}, True),
                                                   ("euler_ancestral", dict(eta=1.), False)])
def test_rollout_sized_calls_go_through_the_graph_path(name, kw, deterministic):
    meta, _ = load_fixture("g7_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta, B=1, seed=41)
    g = gs
    fn = getattr(g, "sample_" + name)
    sig = g.get_sigmas_exponential(10, 0.001, 80.0)
    model.__dict__.pop("_graphed_native", None)
    model.__dict__.pop("_graph_seen", None)
    outs, nexts = [], []
    with torch.no_grad():
        for _ in range(4):
            torch.manual_seed(7)
            outs.append(fn(model, state, noise * 80.0, goal, sig, **kw))
            nexts.append(torch.randn(3, device="cuda"))
        torch.manual_seed(7)
        loop = _host_loop(fn, model, state, noise * 80.0, goal, sig, **kw)
    assert model.__dict__.get("_graphed_native"), "the third identical call did not build a graph"
    for o, nx in zip(outs[2:], nexts[2:]):
        if deterministic:
            assert torch.equal(o, outs[0]), "graph replay differs from the eager call"
        assert_close(o.cpu(), loop.cpu(), what=f"{name} graph vs host loop")
        assert torch.equal(nx, nexts[0])
