"""The adaptive DPM-Solver on the native path on the MI355X (pytest -m gpu): sample_dpm_adaptive (eta = 0) ->
GCDenoiser.sample_dpm_adaptive_native -> mdt_sample_dpm_adaptive, checked with the per-step denoiser disabled and against the
host loop (forced with a no-op callback) for orders 2 and 3, the defaults and a setting with rejected steps, both directions
and B in {1, 8, 256}: the same info dict, the same actions and the same latent_encoder_emb.  A NaN in x_T stops the call."""
import time

import pytest
import torch

from tests.helpers import assert_close as _assert_close, load_fixture
from tests.test_gpu_native_samplers import _host_loop, _no_forward, build, gpu_inputs, gs

pytestmark = pytest.mark.gpu


def assert_close(got, want, what):
    """The tolerance test_gpu_parity.py holds this solver to (HIP step against the oracle step): the ~27 evaluations of a call
    carry the head's last-place differences from the loop's forward through every accepted step (measured: 3.6e-4 at
    max |x| 2.3, B = 8, order 3)."""
    _assert_close(got, want, rtol=2e-3, atol=5e-4, what=what)


@pytest.mark.parametrize("order", [2, 3])
def test_dpm_adaptive_takes_the_native_route(order, monkeypatch):
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    _no_forward(monkeypatch)
    with torch.no_grad():
        out, info = gs.sample_dpm_adaptive(model, state, noise * 80.0, goal, 0.01, 80.0, order=order, return_info=True)
    assert out.shape == noise.shape and bool(torch.isfinite(out).all())
    assert info["nfe"] == order * info["steps"] and info["n_accept"] > 0


@pytest.mark.parametrize("B", [1, 8, 256])
def test_dpm_adaptive_native_matches_the_host_loop(B):
    meta, _ = load_fixture("g3_b256_lang.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta, B=B, seed=700 + B)
    g = gs
    im = model.inner_model
    saw_reject = False
    with torch.no_grad():
        for order in (2, 3):
            for kw in ({}, dict(h_init=2.0)):
                for smin, smax in ((0.01, 80.0), (80.0, 0.01)):
                    x = noise * smax  # x_T at the starting level
                    want, winfo = _host_loop(g.sample_dpm_adaptive, model, state, x, goal, smin, smax, order=order,
                                             return_info=True, **kw)
                    want_ctx = im.latent_encoder_emb.clone()
                    got, info = g.sample_dpm_adaptive(model, state, x, goal, smin, smax, order=order, return_info=True, **kw)
                    what = f"B={B} order={order} {kw} sigma {smax}->{smin}"
                    assert info == winfo, what
                    assert_close(got.cpu(), want.cpu(), what=what)
                    assert_close(im.latent_encoder_emb.cpu(), want_ctx.cpu(), what=what + " ctx")
                    if kw:
                        saw_reject |= winfo["n_reject"] > 0
    assert saw_reject, "the large-h_init setting rejected no step: it does not exercise the reject path"


def test_dpm_adaptive_native_on_a_conditioning_variant():
    meta, _ = load_fixture("g8_no_ada.npz")  # use_ada_conditioning=False: the encoder runs per evaluation
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    g = gs
    im = model.inner_model
    with torch.no_grad():
        want, winfo = _host_loop(g.sample_dpm_adaptive, model, state, noise * 80.0, goal, 0.01, 80.0, return_info=True)
        want_ctx = im.latent_encoder_emb.clone()
        got, info = g.sample_dpm_adaptive(model, state, noise * 80.0, goal, 0.01, 80.0, return_info=True)
    assert info == winfo
    assert_close(got.cpu(), want.cpu(), what="no_ada")
    assert_close(im.latent_encoder_emb.cpu(), want_ctx.cpu(), what="no_ada ctx")


def test_dpm_adaptive_native_stops_on_nan_instead_of_looping():
    from mdt_policy_amd import _lib
    meta, _ = load_fixture("g7c_samplers.npz")
    model = build(meta)
    state, goal, noise = gpu_inputs(meta)
    x = noise * 80.0
    x[0, 0, 0] = float("nan")
    t0 = time.perf_counter()
    with torch.no_grad(), pytest.raises(_lib.MDTHipError, match="stopped"):
        gs.sample_dpm_adaptive(model, state, x, goal, 0.01, 80.0)
    assert time.perf_counter() - t0 < 30.0
