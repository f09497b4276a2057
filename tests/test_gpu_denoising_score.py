"""mdt_denoising_score on the MI355X (pytest -m gpu): the native call through gc_sampling.denoising_score against the float64
oracle in the residual form (tests/score_oracle.py).

Tolerance, per case: E32 = the largest |float32 oracle - float64 oracle| over the case's chunks -- the same precision in another
summation order -- and every chunk must lie within 3 * E32 + 8 * eps32 * sum|terms| of the float64 score: 2 for the different
order of sums times the 1.5 the project accepts for the pair-split launches against fp32 launches; sum|terms| = -score, every
term w_s / M q^2 being >= 0.  Each case prints its largest error beside its bound.

Shapes: B = 3 observations (2 at d = 384), each with its own tokens and goal; (K, S, M) = (1, 1, 1), (3, 3, 2) = 54 decoder
samples and (1, 5, 1), below the split launches; (3, 5, 2) = 90 with the pair-split launches on; (4, 6, 2) = 144 on the wide row
tiles.  Levels are log-uniform from sigma_max = 80 down to sigma_min = 0.001, both included (one level: sigma_min, where the D
form would cancel)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.envelope_configs import ENVELOPE
from tests.guarded import GuardedSet, same_bits
from tests.helpers import assert_close, cfg_of, cuda, load_fixture, observation, params_of, rich_model
from tests.long_chunk_configs import LONG_ENVELOPE
from tests.long_context_configs import CTX_ENVELOPE
from tests.score_oracle import residual_score
from tests.wide_action_configs import WIDE_ENVELOPE

pytestmark = pytest.mark.gpu

SMIN, SMAX = 0.001, 80.0
EPS32 = float(np.finfo(np.float32).eps)
_MODELS, _REFS = {}, {}


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


def levels_of(S):
    return [SMIN] if S == 1 else [math.exp(v) for v in np.linspace(math.log(SMAX), math.log(SMIN), S)]


def entry(name):
    """(cfg, arch, proprio, float32 state dict or None for 'rich' synthetic weights)"""
    if name in ("mdtv_tiny", "mdt_tiny"):
        return configs.NAMED[name](), name[:-5], False, None
    if name.startswith("g11_"):  # the training fixtures' decoder variants, with their own weights
        meta, _ = load_fixture(f"g11_grads_{name[4:]}.npz")
        return cfg_of(meta), meta["arch"], False, params_of(meta)
    if name.startswith("g16_proprio_"):  # the proprioceptive fixtures, with their own weights and state_obs
        meta, _ = load_fixture(name + ".npz")
        return cfg_of(meta), meta["arch"], True, params_of(meta)
    if name == "mdtv_default_no_ada":  # sigma as a context token at the shipped width
        return configs.mdtv_default(use_ada_conditioning=False), "mdtv", False, None
    for env in (ENVELOPE, LONG_ENVELOPE, WIDE_ENVELOPE, CTX_ENVELOPE):
        if name in env:
            return env[name]["cfg"], env[name]["arch"], env[name]["proprio"], None
    raise KeyError(name)


def model_of(name):
    """(GCDenoiser on cuda:0 in eval mode, its float32 state dict)"""
    if name not in _MODELS:
        cfg, _, _, P = entry(name)
        if P is None:
            m, P = rich_model(cfg)
        else:   # a fixture's own weights
            from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
            torch.manual_seed(0)
            m = GCDenoiser(cfg, 0.5)
            m.load_state_dict(P, strict=False)
        _MODELS[name] = (m.cuda().eval(), P)
    return _MODELS[name]


def case(name, B, K, S, M, seed=None):
    """Host inputs: state and goal per observation, x0 (B*K, Ta, A), levels, noise (S, M, Ta, A)."""
    cfg, arch, proprio, _ = entry(name)
    seed = 2000 + 31 * B + 7 * K + 3 * S + M if seed is None else seed
    state, goal, _ = observation(cfg, arch, proprio, B, seed)
    x0 = torch.from_numpy(synthetic.loss_inputs(B * K, cfg, seed + 1)["actions"])
    noise = torch.from_numpy(synthetic.normal("score_noise", (S, M) + tuple(x0.shape[1:]), seed + 2))
    return state, goal, x0, levels_of(S), noise


def reference(name, B, K, S, M):
    """(float64 score, bound) per chunk, computed once per case and left unchanged."""
    key = (name, B, K, S, M)
    if key not in _REFS:
        _, arch, _, _ = entry(name)
        cfg = entry(name)[0]
        _, P = model_of(name)
        state, goal, x0, levels, noise = case(name, B, K, S, M)
        want, terms = residual_score(P, cfg, arch, state, goal, x0, levels, noise, K=K, dtype=torch.float64)
        f32, _ = residual_score(P, cfg, arch, state, goal, x0, levels, noise, K=K, dtype=torch.float32)
        e32 = float((f32.double() - want).abs().max())
        _REFS[key] = (want, 3 * e32 + 8 * EPS32 * terms)
    return _REFS[key]


def native(name, B, K, S, M, weights=None, layout4=False):
    model, _ = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    x = x0.reshape((B, K) + tuple(x0.shape[1:])) if layout4 else x0
    return gs.denoising_score(model, cuda(state), x.cuda(), goal.cuda(), levels, extra_args={"candidates": K}, noise=noise.cuda(),
                                weights=weights)


def check(name, B, K, S, M):
    want, bound = reference(name, B, K, S, M)
    got = native(name, B, K, S, M).cpu().double()
    assert tuple(got.shape) == (B * K,)
    err = (got - want).abs()
    i = int((err / bound).argmax())
    print(f"{name} B={B} (K, S, M)=({K}, {S}, {M}): |got - float64| {float(err[i]):.3e} / bound {float(bound[i]):.3e} "
          f"at score {float(want[i]):.6g}")
    assert bool((err <= bound).all()), (name, B, K, S, M, err.tolist(), bound.tolist())


@pytest.mark.parametrize("K,S,M", [(1, 1, 1), (3, 3, 2), (1, 5, 1)])
@pytest.mark.parametrize("name", ["mdtv_tiny", "mdt_tiny"])
def test_the_score_matches_float64_below_the_split_launches(name, K, S, M):
    check(name, 3, K, S, M)


@pytest.mark.parametrize("K,S,M", [(3, 5, 2), (4, 6, 2)])
def test_the_score_matches_float64_on_the_split_launches_and_the_wide_row_tiles(K, S, M):
    check("mdtv_tiny", 3, K, S, M)


@pytest.mark.parametrize("name", ["g11_mdtv_noise_block", "g11_mdtv_no_ada"])
def test_the_score_matches_float64_on_the_other_decoders(name):
    """NoiseBlock ([c | ones] rows per sample) and sigma as a context token (the encoder on B * S contexts, K * M samples each)."""
    check(name, 3, 3, 3, 2)


@pytest.mark.parametrize("name", ["ta17_hd48", "a17", "ctx17_hd48"])
def test_the_score_matches_float64_past_16_steps_16_elements_and_16_tokens(name):
    check(name, 2, 3, 3, 2)


def test_the_same_call_twice_gives_the_same_bits_in_both_layouts():
    a, b = native("mdtv_tiny", 3, 3, 3, 2), native("mdtv_tiny", 3, 3, 3, 2)
    assert same_bits(a, b)
    grid = native("mdtv_tiny", 3, 3, 3, 2, layout4=True)
    assert tuple(grid.shape) == (3, 3) and same_bits(grid.reshape(-1), a)


def test_a_chunk_alone_scores_like_the_same_chunk_among_three():
    name, B, K, S, M = "mdtv_tiny", 3, 3, 3, 2
    model, _ = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    among = native(name, B, K, S, M).cpu().double().reshape(B, K)
    _, bound = reference(name, B, K, S, M)
    for k in range(K):
        alone = gs.denoising_score(model, cuda(state), x0[k::K].cuda(), goal.cuda(), levels, noise=noise.cuda()).cpu().double()
        err = (alone - among[:, k]).abs()
        print(f"chunk {k} alone against among {K}: {float(err.max()):.3e} / bound {float(bound.reshape(B, K)[:, k].min()):.3e}")
        assert bool((err <= bound.reshape(B, K)[:, k]).all())


def test_all_zero_weights_give_zero():
    got = native("mdtv_tiny", 3, 3, 3, 2, weights=[0.0, 0.0, 0.0])
    assert bool((got == 0).all())


def test_the_context_is_the_encoders():
    name = "mdtv_tiny"
    model, _ = model_of(name)
    state, goal, _, _, _ = case(name, 3, 3, 3, 2)
    native(name, 3, 3, 3, 2)
    ctx = model.inner_model.latent_encoder_emb.clone()
    eng = model._engine(state=cuda(state))
    want = eng.encode(cuda(state), goal.cuda(), honour_modality=True)
    assert tuple(ctx.shape) == (3, eng.Te, eng.D)
    assert_close(ctx.cpu(), want.cpu(), what="ctx_out against mdt_encode")


def test_best_candidates_takes_the_score_as_it_is():
    name, B, K = "mdtv_tiny", 3, 3
    _, _, x0, _, _ = case(name, B, K, 3, 2)
    score = native(name, B, K, 3, 2)
    best, index = gs.best_candidates(x0.cuda(), score, K)
    want = score.reshape(B, K).argmax(1)
    assert torch.equal(index, want)
    assert torch.equal(best.cpu(), x0.reshape((B, K) + tuple(x0.shape[1:]))[torch.arange(B), want.cpu()])


def test_a_captured_call_replays_the_eager_bits():
    name, B, K, S, M = "mdtv_tiny", 1, 3, 3, 2
    model, _ = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    gstate, ggoal, gnoise = cuda(state), goal.cuda(), noise.cuda()
    chunks = [x0.cuda(), case(name, B, K, S, M, seed=91)[2].cuda(), case(name, B, K, S, M, seed=92)[2].cuda()]
    run = lambda x: model.denoising_score(gstate, x, ggoal, levels, gnoise, candidates=K)
    eager = [run(x).clone() for x in chunks]   # the first call also sizes the workspace
    assert not same_bits(eager[1], eager[2])
    static = chunks[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static)
    for i in (1, 2):
        static.copy_(chunks[i])
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[i]), f"replay {i}"


def test_the_call_stays_inside_its_buffers():
    """The C call with every device operand between guard bands: the inputs keep their bits, nothing is written outside score."""
    name, B, K, S, M = "mdtv_tiny", 3, 3, 3, 2
    model, _ = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    want = native(name, B, K, S, M)
    eng = model._engine(state=cuda(state))
    eng.sync_params()
    gset = GuardedSet()
    tok = gset.inp("tokens", state["state_images"].reshape(B, -1))
    g = gset.inp("goal", goal.reshape(B, -1))
    x = gset.inp("x0", x0.reshape(B * K, -1))
    nz = gset.inp("noise", noise.reshape(S * M, -1))
    score = gset.out("score", 1, B * K)
    ctx = gset.out("ctx_out", B * eng.Te, eng.D)
    sig = (C.c_float * S)(*levels)
    _lib.call(eng.lib.mdt_denoising_score, eng.handle, tok.ptr, None, g.ptr, _lib.MODALITY["lang"], x.ptr, sig, None, S, nz.ptr, M, B, K,
              score.ptr, ctx.ptr, eng._stream())
    torch.cuda.synchronize()
    gset.check("mdt_denoising_score")
    score.check("score", written=True)
    ctx.check("ctx_out", written=True)
    assert same_bits(score.region.reshape(-1), want)
