"""DPM-Solver-fast on the native path on the MI355X (pytest -m gpu): sample_dpm_fast -> GCDenoiser.sample_native('dpm_fast') ->
mdt_sample, checked with the per-step denoiser disabled, against the reference's goldens, against the host loop (forced with a
no-op callback) across conditioning variants, batch sizes, evaluation counts and eta (the random stream included), and through
the HIP-graph path of rollout-sized calls."""
import pytest
import torch

from tests.helpers import assert_close, load_fixture
from tests.test_gpu_native_samplers import _host_loop, _no_forward, build, gpu_inputs, gs

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 10, 11, 30]


def _close(got, want, n, what):
    """assert_close with the tolerances of test_gpu_native_samplers.py.  Only n <= 5 -- m = n // 3 + 1 <= 2 steps, each across
    half the range of t or more -- gets an absolute tolerance scaled by the result: steps that long multiply the denoiser's
    last-place differences (native head against the loop's forward) by up to sigma_max / sigma_node ~ 300 (order 1 and 2) or
    e^(2h/3) / (2h/3) ~ 11 (order 3), and the one-step results reach |x| ~ 250.  Measured on the MI355X: 3.4e-3 at
    max |x| 294 (n = 2), 3.1e-4 at 3.4 (n = 3), 6.3e-4 at 4.3 (n = 4)."""
    atol = 1e-4 * max(1.0, float(want.abs().max())) if n <= 5 else 1e-4
    assert_close(got.cpu(), want.cpu(), atol=atol, what=what)


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_dpm_fast_takes_the_native_route(eta, monkeypatch):
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    with torch.no_grad():
        torch.manual_seed(5)
        out = gs.sample_dpm_fast(model, state, noise * 80.0, goal, 0.001, 80.0, 10, eta=eta)
    assert out.shape == noise.shape and bool(torch.isfinite(out).all())


def test_g7c_dpm_fast_goldens_on_the_native_path(monkeypatch):
    meta, fx = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    with torch.no_grad():
        for nfe in (9, 10, 11):
            out = gs.sample_dpm_fast(model, state, noise * 80.0, goal, 0.001, 80.0, nfe, noise_sampler=lambda s0, s1: None)
            assert_close(out.cpu(), fx[f"dpm_fast_nfe{nfe}"], what=f"dpm_fast nfe={nfe}")


@pytest.mark.parametrize("variant", ["g7c_samplers", "g3_b8_mdt", "g8_no_ada", "g8_mlp_head", "g8_noise_block"])
def test_dpm_fast_native_matches_the_host_loop_on_the_conditioning_variants(variant):
    meta, _ = load_fixture(f"{variant}.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    g = gs
    im = model.inner_model
    with torch.no_grad():
        for n in NS:
            for smax, smin in ((80.0, 0.001), (0.01, 80.0)):
                want = _host_loop(g.sample_dpm_fast, model, state, noise * smax, goal, smin, smax, n)
                want_ctx = im.latent_encoder_emb.clone()
                got = g.sample_dpm_fast(model, state, noise * smax, goal, smin, smax, n)
                _close(got, want, n, what=f"{variant} n={n} sigma {smax}->{smin}")
                assert_close(im.latent_encoder_emb.cpu(), want_ctx.cpu(), what=f"{variant} n={n} ctx")


@pytest.mark.parametrize("B", [1, 7, 77, 256])
def test_dpm_fast_native_matches_the_host_loop_across_batch_sizes_and_eta(B):
    meta, _ = load_fixture("g3_b256_lang.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta, B=B, seed=500 + B)
    g = gs
    with torch.no_grad():
        for n in NS:
            for eta in (0.0, 0.5):
                torch.manual_seed(B + n)
                want = _host_loop(g.sample_dpm_fast, model, state, noise * 80.0, goal, 0.001, 80.0, n, eta=eta)
                after_loop = torch.randn(5, device="cuda")
                torch.manual_seed(B + n)
                got = g.sample_dpm_fast(model, state, noise * 80.0, goal, 0.001, 80.0, n, eta=eta)
                after_native = torch.randn(5, device="cuda")
                _close(got, want, n, what=f"B={B} n={n} eta={eta}")
                assert torch.equal(after_native, after_loop), f"B={B} n={n} eta={eta}: the generator moved differently"


def test_dpm_fast_host_and_device_levels_give_the_same_plan():
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    with torch.no_grad():
        for n in (4, 11, 128):
            host = model.sample_native("dpm_fast", state, noise * 80.0, goal, [80.0, 0.001], n_steps=n, eta=0.)
            dev = model.sample_native("dpm_fast", state, noise * 80.0, goal, torch.tensor([80.0, 0.001], device="cuda"),
                                      n_steps=n, eta=0.)
            assert torch.equal(host, dev), f"n={n}"


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_dpm_fast_rollout_sized_calls_replay_a_graph_equal_to_eager(eta):
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta, B=1, seed=43)
    g = gs
    model.__dict__.pop("_graphed_native", None)
    model.__dict__.pop("_graph_seen", None)
    outs, nexts = [], []
    with torch.no_grad():
        for _ in range(4):
            torch.manual_seed(9)
            outs.append(g.sample_dpm_fast(model, state, noise * 80.0, goal, 0.001, 80.0, 10, eta=eta))
            nexts.append(torch.randn(3, device="cuda"))
        torch.manual_seed(9)
        loop = _host_loop(g.sample_dpm_fast, model, state, noise * 80.0, goal, 0.001, 80.0, 10, eta=eta)
        cache = model.__dict__.get("_graphed_native")
        assert cache and cache[-1].kind == "dpm_fast" and cache[-1].n_steps == 10, "the third identical call built no graph"
        # another evaluation count is another graph key: eager again, not the n = 10 graph
        other = g.sample_dpm_fast(model, state, noise * 80.0, goal, 0.001, 80.0, 11)
        want_other = _host_loop(g.sample_dpm_fast, model, state, noise * 80.0, goal, 0.001, 80.0, 11)
    for o, nx in zip(outs[2:], nexts[2:]):
        if eta == 0:
            assert torch.equal(o, outs[0]), "graph replay differs from the eager call"
        assert_close(o.cpu(), outs[0].cpu(), what="dpm_fast graph replay vs eager")
        assert torch.equal(nx, nexts[0])
    assert_close(outs[-1].cpu(), loop.cpu(), what="dpm_fast graph vs host loop")
    assert_close(other.cpu(), want_other.cpu(), what="dpm_fast n=11 after an n=10 graph")


def test_dpm_fast_native_call_rejects_bad_levels():
    from mdt_policy_amd import _lib
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    with torch.no_grad():
        for levels, n in (([80.0, 0.0], 10), ([80.0, 0.001], 0), ([80.0, 0.001], 129)):
            with pytest.raises(_lib.MDTHipError):
                model.sample_native("dpm_fast", state, noise, goal, levels, n_steps=n, eta=0.)
