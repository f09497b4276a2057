"""mdt_log_likelihood on the GPU (include/mdt_hip_train.h; gc_sampling.log_likelihood with this package's GCDenoiser): against the
g17 fixtures, against the host loop it replaces -- ``gs._dopri5`` over a flow made of ``model.denoise_vjp`` on observations
expanded with repeat_interleave, both untouched by the native call -- across candidates, probes and the conditioning variants,
plus what the call promises about itself: shared context = same context, the tape survives a backward, reproducible bits, no
capture.  Tolerances are tests/test_log_likelihood.py's: rtol=2e-3, atol=0.05 on ll and delta, fevals within 0.3x .. 3x;
``latent`` uses assert_close's defaults scaled by sigma_max (the latent is sigma_max-sized noise)."""
import functools
import warnings

import pytest
import torch

from mdt_policy_amd import _lib, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, inputs_of, load_fixture
from tests.test_log_likelihood import CASES, case, gpu_model, to_cuda

pytestmark = pytest.mark.gpu
LL = dict(rtol=2e-3, atol=0.05)


def take(state, n):
    return {k: (v[:n] if torch.is_tensor(v) else v) for k, v in state.items()}


def expand(state, K):
    return {k: (v.repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}


def chunks_of(action, K, seed=31):
    """(B*K, Ta, A): chunk 0 of every observation is its action, the others are perturbed by 0.3 N(0, 1)."""
    B = action.shape[0]
    rows = action.repeat_interleave(K, 0).clone()
    noise = torch.from_numpy(synthetic.normal("ll_chunks", tuple(rows.shape), seed))
    keep = (torch.arange(B * K) % K == 0)[:, None, None]
    return torch.where(keep, rows, rows + 0.3 * noise)


def signs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def parent_path(model, state, goal, rows, v, K, sigma_min, sigma_max, rtol=1e-4, atol=1e-4):
    """What log_likelihood ran before the native call: _dopri5 on the host over denoise_vjp, observations expanded K times.
    Returns (ll, latent, delta, fevals)."""
    st, g = expand(state, K), goal.repeat_interleave(K, 0)
    P, fevals = v.shape[0], [0]

    def flow(sigma, y):
        x = y[0]
        fevals[0] += 1
        sg = torch.full((x.shape[0],), sigma, device=x.device, dtype=x.dtype)
        div = 0
        for p in range(P):
            den, jtv = model.denoise_vjp(st, x, g, sg, v[p])
            div = div + (v[p] * ((v[p] - jtv) / sigma)).flatten(1).sum(1)
        return gs.to_d(x, sigma, den), div / P

    with torch.no_grad():
        latent, delta = gs._dopri5(flow, (rows, rows.new_zeros([rows.shape[0]])), float(sigma_min), float(sigma_max), rtol, atol)
        ll = torch.distributions.Normal(0, sigma_max).log_prob(latent).flatten(1).sum(1) + delta
    return ll.cpu(), latent.cpu(), delta.cpu(), fevals[0]


@functools.lru_cache(maxsize=None)
def tiny():
    meta, fx, cfg, state, goal, action = case("mdtv_tiny")
    return meta, fx, gpu_model(meta, cfg), to_cuda(state), goal.cuda(), action


def check_info(info):
    assert info["fevals"] == 2 + 6 * info["steps"] and info["steps"] == info["n_accept"] + info["n_reject"], info


@pytest.mark.parametrize("name", CASES)
def test_native_call_matches_the_reference_fixtures(name):
    """K = 1, P = 1, the fixture's own probe passed as a tensor: the reference's log_likelihood values."""
    meta, fx, cfg, state, goal, action = case(name)
    model = gpu_model(meta, cfg)
    v = torch.from_numpy(fx["v"]).cuda()[None]
    ll, info = gs.log_likelihood(model, to_cuda(state), action.cuda(), goal.cuda(), meta["sigma_min"], meta["sigma_max"],
                                 extra_args={"probes": v})
    assert ll.shape == (meta["B"],)
    assert_close(ll.cpu(), fx["ll"], what="log-likelihood", **LL)
    assert 0.3 * meta["fevals"] <= info["fevals"] <= 3 * meta["fevals"]
    check_info(info)


@pytest.mark.parametrize("B,K", [(1, 1), (3, 5), (2, 40)])
def test_native_call_matches_the_host_loop_it_replaces(B, K):
    """R = 1 is the single-row edge; R = 15 fills no workgroup evenly (the right-hand side runs 4 rows per workgroup, the norms
    256 elements: 15 * 70 + 15 = 1065 of them, 5 workgroups with a ragged last one); R = 80 is 80 * 70 + 80 = 5680 entries,
    23 workgroups of the error kernel's partials."""
    meta, fx, model, state, goal, action = tiny()
    st, g = take(state, B), goal[:B]
    rows = chunks_of(action[:B], K).cuda()
    v = signs((1, B * K) + tuple(rows.shape[1:]), 5)
    v[0, ::K] = torch.from_numpy(fx["v"][:B])  # chunk 0 of every observation under the fixture's probe
    v = v.cuda()
    want_ll, want_latent, want_delta, want_fe = parent_path(model, st, g, rows, v, K, meta["sigma_min"], meta["sigma_max"])
    ll, latent, delta, info = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"], candidates=K)
    print(f"B={B} K={K}: fevals {info['fevals']} (host loop {want_fe}); max |ll - host| {float((ll.cpu() - want_ll).abs().max()):.3e}, "
          f"|latent - host| {float((latent.cpu() - want_latent).abs().max()):.3e}, "
          f"|delta - host| {float((delta.cpu() - want_delta).abs().max()):.3e}")
    assert_close(latent.cpu(), want_latent, rtol=RTOL, atol=ATOL * meta["sigma_max"], what="latent")
    assert_close(delta.cpu(), want_delta, what="delta", **LL)
    assert_close(ll.cpu(), want_ll, what="log-likelihood", **LL)
    assert 0.3 * want_fe <= info["fevals"] <= 3 * want_fe
    check_info(info)
    # ... and through the facade: the (B, K, Ta, A) shape goes in, (B, K) comes out, the same bits
    ll2, info2 = gs.log_likelihood(model, st, rows.reshape((B, K) + tuple(rows.shape[1:])), g, meta["sigma_min"], meta["sigma_max"],
                                   extra_args={"candidates": K, "probes": v})
    assert ll2.shape == (B, K) and torch.equal(ll2.reshape(-1), ll) and info2 == info
    if K == 5:  # chunk 0 of every observation is the fixture's action: its value stays the fixture's under the shared step size
        assert_close(ll.cpu()[::K], fx["ll"][:B], what="chunk 0 against the fixture", **LL)
        with pytest.raises(ValueError, match=r"14.*15|15.*14"):
            gs.log_likelihood(model, st, rows[:14], g, meta["sigma_min"], meta["sigma_max"], extra_args={"candidates": K})


def test_shared_context_is_the_same_context():
    """candidates = K on B observations against candidates = 1 on the observations repeated K times: the encoder and the K|V rows
    are computed per observation either way, so the bits agree."""
    meta, fx, model, state, goal, action = tiny()
    B, K = 3, 5
    rows = chunks_of(action[:B], K).cuda()
    v = signs((1, B * K) + tuple(rows.shape[1:]), 6).cuda()
    a = model.log_likelihood(take(state, B), rows, goal[:B], v, meta["sigma_min"], meta["sigma_max"], candidates=K)
    b = model.log_likelihood(expand(take(state, B), K), rows, goal[:B].repeat_interleave(K, 0), v, meta["sigma_min"],
                             meta["sigma_max"], candidates=1)
    assert a[3] == b[3]
    for x, y, what in zip(a[:3], b[:3], ("ll", "latent", "delta")):
        assert torch.equal(x, y), f"{what}: max diff {float((x - y).abs().max()):.3e}"


def test_the_tape_survives_a_backward():
    """P = 2 with the same probe twice is P = 1 bit for bit ((a + a) / 2 == a): the second backward found the tape as the first
    did.  With two distinct probes delta is the mean of the single-probe deltas -- at the tolerance, the step sequences differ."""
    meta, fx, model, state, goal, action = tiny()
    B, K = 2, 3
    st, g = take(state, B), goal[:B]
    rows = chunks_of(action[:B], K).cuda()
    v0, v1 = (signs((1, B * K) + tuple(rows.shape[1:]), s).cuda() for s in (7, 8))
    run = lambda v: model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"], candidates=K)
    one, other = run(v0), run(v1)
    twice = run(torch.cat([v0, v0]))
    assert twice[3] == one[3]
    for x, y, what in zip(twice[:3], one[:3], ("ll", "latent", "delta")):
        assert torch.equal(x, y), f"{what}: max diff {float((x - y).abs().max()):.3e}"
    both = run(torch.cat([v0, v1]))
    assert_close(both[2].cpu(), ((one[2] + other[2]) / 2).cpu(), rtol=0.0, atol=0.05, what="delta of two probes")
    check_info(both[3])
    # the facade's int draws P * numel signs in one call, probe-major: the first draw of that call is not _probe_signs(rows)'s
    torch.manual_seed(11)
    ll3, info3 = gs.log_likelihood(model, st, rows, g, meta["sigma_min"], meta["sigma_max"], extra_args={"candidates": K, "probes": 3})
    torch.manual_seed(11)
    v3 = gs._probe_signs(rows.new_empty((3,) + tuple(rows.shape)))
    assert torch.equal(ll3, run(v3)[0])


def variant(name):
    if name == "proprio":
        from tests.test_proprio import case as pcase
        meta, fx, cfg, state, goal, noise, li = pcase("tiny")
        return meta, cfg, state, goal, li["actions"]
    meta, _ = load_fixture(f"g11_grads_{name}.npz")
    cfg = cfg_of(meta)
    state, goal, _ = inputs_of(meta)
    return meta, cfg, state, goal, torch.from_numpy(synthetic.loss_inputs(meta["B"], cfg, meta["loss_seed"])["actions"])


@pytest.mark.parametrize("name", ["mdtv_noise_block", "mdtv_no_ada", "mdtv_rope", "mdtv_mlp_head", "proprio"])
def test_conditioning_variants_match_the_host_loop(name):
    """NoiseBlock, the sigma token (the context is then per evaluation: hoisting it would fail here), RoPE, the MLP head and the
    proprio token, each at (B, K) = (2, 3)."""
    meta, cfg, state, goal, action = variant(name)
    model = gpu_model(meta, cfg)
    B, K, smin, smax = 2, 3, 0.001, 80.0
    st, g = take(to_cuda(state), B), goal[:B].cuda()
    rows = chunks_of(action[:B], K).cuda()
    v = signs((1, B * K) + tuple(rows.shape[1:]), 9).cuda()
    want_ll, want_latent, want_delta, want_fe = parent_path(model, st, g, rows, v, K, smin, smax)
    ll, latent, delta, info = model.log_likelihood(st, rows, g, v, smin, smax, candidates=K)
    print(f"{name}: fevals {info['fevals']} (host loop {want_fe}); max |ll - host| {float((ll.cpu() - want_ll).abs().max()):.3e}")
    assert_close(latent.cpu(), want_latent, rtol=RTOL, atol=ATOL * smax, what="latent")
    assert_close(delta.cpu(), want_delta, what="delta", **LL)
    assert_close(ll.cpu(), want_ll, what="log-likelihood", **LL)
    assert 0.3 * want_fe <= info["fevals"] <= 3 * want_fe
    check_info(info)


def test_two_identical_calls_give_identical_bits():
    meta, fx, model, state, goal, action = tiny()
    B, K = 3, 5
    rows = chunks_of(action[:B], K).cuda()
    v = signs((2, B * K) + tuple(rows.shape[1:]), 10).cuda()
    a = model.log_likelihood(take(state, B), rows, goal[:B], v, meta["sigma_min"], meta["sigma_max"], candidates=K)
    b = model.log_likelihood(take(state, B), rows, goal[:B], v, meta["sigma_min"], meta["sigma_max"], candidates=K)
    assert a[3] == b[3]
    for x, y, what in zip(a[:3], b[:3], ("ll", "latent", "delta")):
        assert torch.equal(x, y), what


def test_a_capturing_stream_is_refused_and_nothing_is_enqueued():
    meta, fx, model, state, goal, action = tiny()
    B = 2
    st, g, rows = take(state, B), goal[:B], action[:B].cuda()
    v = signs((1, B) + tuple(rows.shape[1:]), 12).cuda()
    before = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])  # (parameters uploaded, buffers grown)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        with torch.cuda.graph(graph):
            with pytest.raises(_lib.MDTHipError) as err:
                model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    assert err.value.status == 5 and "mdt_log_likelihood" in str(err.value) and "captured" in str(err.value)  # MDT_ERR_STATE
    assert any("Graph is empty" in str(w.message) for w in seen), [str(w.message) for w in seen]
    torch.cuda.synchronize()
    after = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])  # the handle is as it was
    assert after[3] == before[3] and all(torch.equal(x, y) for x, y in zip(after[:3], before[:3]))


def test_numeric_stop_and_argument_refusals_leave_the_handle_usable():
    """max_steps exhausted is MDT_ERR_NUMERIC with the tapes released: sixteen such calls would otherwise use the pool up."""
    meta, fx, model, state, goal, action = tiny()
    st, g, rows = take(state, 1), goal[:1], action[:1].cuda()
    v = signs((1, 1) + tuple(rows.shape[1:]), 13).cuda()
    for _ in range(18):
        with pytest.raises(_lib.MDTHipError) as err:
            model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"], max_steps=2)
        assert err.value.status == 6 and "step budget" in str(err.value)
    with pytest.raises(_lib.MDTHipError) as err:
        model.log_likelihood(st, rows, g, v, meta["sigma_max"], meta["sigma_min"])
    assert err.value.status == 1 and "sigma_max" in str(err.value)
    with pytest.raises(ValueError):
        model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"], candidates=0)
    ll, _, _, info = model.log_likelihood(st, rows, g, v, meta["sigma_min"], meta["sigma_max"])
    assert bool(torch.isfinite(ll).all())
    check_info(info)


def test_best_candidates_on_the_device():
    B, K = 3, 4
    chunks = torch.randn(B * K, 10, 7, device="cuda")
    scores = torch.tensor([[0.1, 0.7, 0.7, -1.0], [5.0, 5.0, 5.0, 5.0], [-9.0, -3.0, -2.0, -2.5]], device="cuda")
    best, index = gs.best_candidates(chunks, scores.reshape(-1), K)
    assert best.is_cuda and index.is_cuda and best.shape == (B, 10, 7) and index.tolist() == [1, 0, 2]
    assert torch.equal(best, chunks.reshape(B, K, 10, 7)[torch.arange(B), index.cpu()])
    best2, index2 = gs.best_candidates(chunks.reshape(B, K, 10, 7), scores, K)
    assert torch.equal(best2, best) and torch.equal(index2, index)


def test_the_call_is_refused_between_the_stages_of_a_staged_loss_backward():
    """The P backwards write the scratch that carries a staged loss backward from stage to stage: in between the call is
    MDT_ERR_STATE (nothing enqueued, no tape taken), and it runs once the staged backward has finished."""
    from tests.test_gpu_denoise_grad import facade, load_case
    meta, cfg, state, goal, li = load_case("mdtv_tiny")
    model = facade(meta, cfg)
    st = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    eng = model._engine(allow_grad=True, state=st)
    tok, tok2, gg, B, _, _ = model._train_inputs(eng, st, goal.cuda(), True)
    a, nz = eng._in(li["actions"].cuda(), (B, eng.Ta, eng.A)), eng._in(li["noise_train"].cuda(), (B, eng.Ta, eng.A))
    sg = eng._in(li["sigma"].cuda(), (B,))
    v = signs((1,) + tuple(a.shape), 14).cuda()
    _, _, _, loss_tape = eng.train_loss_fwd(st, tok, tok2, gg, a, nz, sg, None)
    buf = eng.train_loss_bwd_begin(torch.ones((), device="cuda"), None, tok, tok2, gg, (False, False, False))
    eng.train_loss_bwd_stage(loss_tape, 0, *buf)
    with pytest.raises(_lib.MDTHipError) as err:
        eng.log_likelihood(st, a, gg, v, 0.001, 80.0)
    assert err.value.status == 5 and "mdt_log_likelihood" in str(err.value) and "staged loss backward" in str(err.value)
    for k in range(1, eng._n_stages):
        eng.train_loss_bwd_stage(loss_tape, k, *buf)
    eng.tape_release(loss_tape)
    ll, _, _, info = eng.log_likelihood(st, a, gg, v, 0.001, 80.0)
    assert bool(torch.isfinite(ll).all())
    check_info(info)
