"""mdt_denoising_score across the configurations mdt_create accepts (pytest -m gpu): the native call through
gc_sampling.denoising_score against the float64 oracle in the residual form (tests/score_oracle.py), with the helpers and the
per-case bound of tests/test_gpu_denoising_score.py unchanged -- every chunk within 3 * E32 + 8 * eps32 * sum|terms| of float64,
E32 the float32 oracle's own distance from it.  Each case prints its largest error beside its bound (DESIGN.md 4.3k has the table).

What tests/test_gpu_denoising_score.py never ran: the nine configurations of tests/envelope_configs.py and the long-chunk,
wide-action and long-context tables; sigma as a context token WITH tokens2 (MDT's gripper tokens; a use_proprio handle's state_obs),
at depth (the pair-split launches from 768 decoder rows, the wide row tiles from 1401), its ctx_out (value, guard bands, capture);
S and M at 64; the library's own trapezoid weights over ascending levels.  The oracle stays at seconds: R <= 6 chunks and
S M <= 12 passes at d >= 384 (the two deep cases: 9 x 10 and 12 x 12)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from oracle import mdt_oracle as O
from tests.envelope_configs import ENVELOPE
from tests.guarded import GuardedSet, same_bits
from tests.helpers import assert_close
from tests.score_oracle import residual_score, trapezoid
from tests.test_gpu_denoising_score import EPS32, _inference, case, check, cuda, entry, gs, model_of, native  # noqa: F401

pytestmark = pytest.mark.gpu

TABLES = ["ta64_hd48", "ta48_plain", "ta32_noise", "mdt_ta40_hd64", "ta20_mlp_head_proprio", "a64", "a48_plain", "mdt_a20_d512",
          "a64_ta24_rope_hd64", "ctx64_hd48", "ctx32_plain", "ctx40_ta48", "ctx34_proprio_mlp_head", "ctx40_no_goal", "ctx18_a64"]


@pytest.mark.parametrize("name", sorted(ENVELOPE) + TABLES)
def test_the_score_matches_float64_across_the_envelope(name):
    check(name, 2, 3, 3, 2)


def test_the_tables_hold_what_they_are_here_for():
    cfgs = {n: entry(n) for n in sorted(ENVELOPE) + TABLES}
    assert len(ENVELOPE) == 9
    assert any(not c.get("linear_output", True) for c, _, _, _ in cfgs.values()), "no MLP head"
    assert not cfgs["ctx40_no_goal"][0].get("goal_conditioned", True)
    assert any(p for _, _, p, _ in cfgs.values()) and any(a == "mdt" for _, a, _, _ in cfgs.values())
    assert any(c.get("use_rot_embed") for c, _, _, _ in cfgs.values()) and any(c.get("use_noise_encoder") for c, _, _, _ in cfgs.values())
    for n in ("g11_mdt_no_ada", "g16_proprio_tiny_no_ada", "mdtv_default_no_ada"):
        assert not entry(n)[0]["use_ada_conditioning"]
    assert entry("g11_mdt_no_ada")[1] == "mdt" and entry("g16_proprio_tiny_no_ada")[2]


@pytest.mark.parametrize("name", ["g11_mdt_no_ada", "g16_proprio_tiny_no_ada"])
def test_sigma_as_a_context_token_with_tokens2(name):
    """k_score_repeat's tokens2 branch and the encoder on the staged tokens2: MDT's gripper tokens (w2 = obs_dim) and a use_proprio
    handle's state_obs (w2 = proprio_dim), each staged S times."""
    check(name, 3, 3, 3, 2)


@pytest.mark.parametrize("K,S,M", [(3, 5, 2), (4, 6, 2)])
def test_a_sigma_token_model_at_depth(K, S, M):
    """B = 3 at the shipped width: 900 decoder rows (the pair-split launches) and 1440 (the wide row tiles), B * S = 15 / 18
    contexts, K * M samples reading each."""
    assert 768 <= 3 * K * S * M * 10 and (3 * K * S * M * 10 > 1400) == (K == 4)
    check("mdtv_default_no_ada", 3, K, S, M)


@pytest.mark.parametrize("name", ["g11_mdtv_no_ada", "g11_mdt_no_ada"])
def test_the_context_of_a_sigma_token_model_is_the_last_levels(name):
    B, K, S, M = 3, 3, 3, 2
    cfg, arch, _, _ = entry(name)
    model, P = model_of(name)
    state, goal, _, levels, _ = case(name, B, K, S, M)
    native(name, B, K, S, M)
    ctx = model.inner_model.latent_encoder_emb.clone().cpu()
    P64 = O.to_dtype(P, torch.float64)
    st = {k: (v.double() if torch.is_tensor(v) else v) for k, v in state.items()}
    at = lambda sg: O.encode(P64, cfg, st, goal.double(), arch, "forward", sigma=torch.full((B,), float(sg), dtype=torch.float64))
    last, first = at(levels[-1]), at(levels[0])
    assert tuple(ctx.shape) == tuple(last.shape)
    print(f"{name}: ctx_out against float64 at the last level {float((ctx.double() - last).abs().max()):.3e}, "
          f"at the first {float((ctx.double() - first).abs().max()):.3e}")
    assert_close(ctx, last, what="ctx_out against the oracle's encoder at the last level")
    with pytest.raises(AssertionError):
        assert_close(ctx, first, what="ctx_out against the first level")
    assert len({ctx[b].numpy().tobytes() for b in range(B)}) == B   # each observation its own


def guarded_call(name, B, K, S, M, levels=None, weights=None, with_ctx=True):
    """The C call with every device operand between guard bands: (score bits as a tensor, ctx_out region or None)."""
    model, _ = model_of(name)
    _, arch, proprio, _ = entry(name)
    state, goal, x0, lv, noise = case(name, B, K, S, M)
    levels = lv if levels is None else levels
    eng = model._engine(state=cuda(state))
    eng.sync_params()
    gset = GuardedSet()
    if arch == "mdtv":
        tok = gset.inp("tokens", state["state_images"].reshape(B, -1))
        tok2 = gset.inp("tokens2", state["state_obs"].reshape(B, -1)) if proprio else None
    else:
        tok, tok2 = gset.inp("tokens", state["static"].reshape(B, -1)), gset.inp("tokens2", state["gripper"].reshape(B, -1))
    g = gset.inp("goal", goal.reshape(B, -1))
    x = gset.inp("x0", x0.reshape(B * K, -1))
    nz = gset.inp("noise", noise.reshape(S * M, -1))
    score = gset.out("score", 1, B * K)
    ctx = gset.out("ctx_out", B * eng.Te, eng.D) if with_ctx else None
    sig = (C.c_float * S)(*levels)
    w = None if weights is None else (C.c_float * S)(*weights)
    _lib.call(eng.lib.mdt_denoising_score, eng.handle, tok.ptr, tok2.ptr if tok2 else None, g.ptr, _lib.MODALITY["lang"], x.ptr, sig, w, S,
              nz.ptr, M, B, K, score.ptr, ctx.ptr if ctx else None, eng._stream())
    torch.cuda.synchronize()
    gset.check(f"mdt_denoising_score {name}")
    score.check("score", written=True)
    if ctx:
        ctx.check("ctx_out", written=True)
    return score.region.reshape(-1).clone(), (ctx.region.reshape(B, eng.Te, eng.D).clone() if ctx else None)


@pytest.mark.parametrize("name", ["g11_mdtv_no_ada", "mdt_tiny", "g11_mdt_no_ada"])
def test_the_call_stays_inside_its_buffers(name):
    """score and ctx_out written, every input's bits kept, nothing outside: the strided copy of the last level's contexts
    (g11_mdtv_no_ada), tokens2 between bands (mdt_tiny), both (g11_mdt_no_ada)."""
    B, K, S, M = 3, 3, 3, 2
    want = native(name, B, K, S, M)
    model, _ = model_of(name)
    want_ctx = model.inner_model.latent_encoder_emb.clone()
    score, ctx = guarded_call(name, B, K, S, M)
    assert same_bits(score, want) and same_bits(ctx, want_ctx)


def test_a_captured_call_of_a_sigma_token_model_replays_the_eager_bits():
    name, B, K, S, M = "g11_mdtv_no_ada", 1, 3, 3, 2
    model, _ = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    gstate, ggoal, gnoise = cuda(state), goal.cuda(), noise.cuda()
    chunks = [x0.cuda(), case(name, B, K, S, M, seed=91)[2].cuda(), case(name, B, K, S, M, seed=92)[2].cuda()]

    def run(x):
        score = model.denoising_score(gstate, x, ggoal, levels, gnoise, candidates=K)
        return score, model.inner_model.latent_encoder_emb
    eager = [tuple(t.clone() for t in run(x)) for x in chunks]   # the first call also sizes the workspace
    assert not same_bits(eager[1][0], eager[2][0])
    static = chunks[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, ctx = run(static)
    for i in (1, 2):
        static.copy_(chunks[i])
        ctx.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(out, eager[i][0]), f"replay {i}: score"
        assert same_bits(ctx, eager[i][1]), f"replay {i}: ctx_out"


@pytest.mark.parametrize("S,M", [(64, 2), (2, 64)])
def test_levels_and_draws_at_the_limit(S, M):
    check("mdtv_tiny", 1, 1, S, M)


def test_the_librarys_own_weights_over_ascending_levels():
    """weights_host == NULL with S = 5 ascending levels: the oracle's trapezoid, and the bits of the same call given those weights
    rounded to float32."""
    name, B, K, S, M = "mdtv_tiny", 3, 3, 5, 2
    cfg, arch, _, _ = entry(name)
    _, P = model_of(name)
    state, goal, x0, levels, noise = case(name, B, K, S, M)
    up = levels[::-1]
    assert all(b > a for a, b in zip(up, up[1:]))
    own, _ = guarded_call(name, B, K, S, M, levels=up, with_ctx=False)
    f32 = [float(np.float32(v)) for v in up]   # the levels as the call reads them
    given, _ = guarded_call(name, B, K, S, M, levels=up, weights=[float(np.float32(w)) for w in trapezoid(f32)], with_ctx=False)
    assert same_bits(own, given), "the library's trapezoid weights are not the oracle's, rounded to float32"
    want, terms = residual_score(P, cfg, arch, state, goal, x0, up, noise, weights=trapezoid(up), K=K, dtype=torch.float64)
    f, _ = residual_score(P, cfg, arch, state, goal, x0, up, noise, weights=trapezoid(up), K=K, dtype=torch.float32)
    bound = 3 * float((f.double() - want).abs().max()) + 8 * EPS32 * terms
    err = (own.cpu().double() - want).abs()
    i = int((err / bound).argmax())
    print(f"{name} ascending levels, the library's weights: |got - float64| {float(err[i]):.3e} / bound {float(bound[i]):.3e}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
