"""Sample, score and select as one native call on the MI355X (pytest -m gpu): GCDenoiser.sample_select -> mdt_sample_ddim_select /
mdt_sample_select against the three calls it replaces -- the ``*_multi`` sampler, mdt_denoising_score, gc_sampling.best_candidates
-- on the same inputs and noise.

Unguided, chunks, scores, index and best must have the three calls' bits: the sampler's launches are the ``*_multi`` entry's, the
score phase makes mdt_denoising_score's launches but for the encoder, whose output it reads where the sampler's prefix left it
(sigma as a context token: it encodes what the stand-alone call encodes).  Guided, the chunks have the guided ``*_multi`` call's
bits and the scores are held to the float64 oracle (tests/score_oracle.py) within the bound of tests/test_gpu_denoising_score.py
-- 3 E32 + 8 eps32 sum|terms|, E32 the float32 oracle's own distance from the float64 one -- because the sampler's encoder ran 2B
contexts where the stand-alone scorer's runs B.

Cases (B, K, S, M): (1, 1, 1, 1); (3, 5, 3, 2); (2, 40, 2, 2) = 320 score rows; and (1, 8, 16, 2) at the shipped MDT-V width with
the library's synthetic weights: 8 sampler rows in the small-batch regime, 256 score samples = 2560 rows on the pair-split
launches.  The schedule has four steps."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.guarded import same_bits
from tests.helpers import cfg_of, cuda, load_fixture, observation, params_of, rich_model
from tests.score_oracle import residual_score
from tests.test_gpu_denoising_score import levels_of

pytestmark = pytest.mark.gpu

SMIN, SMAX = 0.001, 80.0
EPS32 = float(np.finfo(np.float32).eps)
N_STEPS = 4
_MODELS = {}
CASES = [(1, 1, 1, 1), (3, 5, 3, 2), (2, 40, 2, 2)]
SHIPPED = (1, 8, 16, 2)


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


def entry(name):
    """(cfg, arch, float32 state dict or None for 'rich' synthetic weights)"""
    if name in ("mdtv_tiny", "mdt_tiny"):
        return configs.NAMED[name](), name[:-5], None
    if name == "mdtv_default":
        return configs.mdtv_default(), "mdtv", None
    meta, _ = load_fixture(f"g11_grads_{name[4:]}.npz")
    return cfg_of(meta), meta["arch"], params_of(meta)


def model_of(name):
    if name not in _MODELS:
        cfg, _, P = entry(name)
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
    """Device inputs: state and goal per observation, x_T (B*K, Ta, A), the score's levels and noise rows (S, M, Ta, A), the
    sampler's noise rows (N_STEPS, B*K, Ta, A), a pin per chunk; and the host copies of state and goal for the oracle."""
    cfg, arch, _ = entry(name)
    seed = 3000 + 31 * B + 7 * K + 3 * S + M if seed is None else seed
    state, goal, _ = observation(cfg, arch, False, B, seed)
    shape = tuple(torch.from_numpy(synthetic.loss_inputs(1, cfg, seed)["actions"]).shape[1:])
    x_T = SMAX * torch.from_numpy(synthetic.normal("x_T", (B * K,) + shape, seed + 1))
    snoise = torch.from_numpy(synthetic.normal("score_noise", (S, M) + shape, seed + 2))
    rows = torch.from_numpy(synthetic.normal("sampler_noise", (N_STEPS, B * K) + shape, seed + 3))
    known = torch.from_numpy(synthetic.normal("pin_known", (B * K,) + shape, seed + 4))
    keep = torch.zeros((B * K,) + shape)
    keep[:, :2] = 1.0
    keep[:, 2] = 0.5
    return dict(state=cuda(state), goal=goal.cuda(), x_T=x_T.cuda(), levels=levels_of(S), snoise=snoise.cuda(), rows=rows.cuda(),
                pin=(known.cuda(), keep.cuda()), host_state=state, host_goal=goal,
                sig=gs.get_sigmas_exponential(N_STEPS, SMIN, SMAX))


def three_calls(model, c, K, kind, pin=None, lam=None):
    kw = {} if lam is None else {"cond_lambda": lam}
    if kind == "ddim":
        chunks = model.sample_ddim(c["state"], c["x_T"], c["goal"], c["sig"], candidates=K, pin=pin, **kw)
    else:
        chunks = model.sample_native(kind, c["state"], c["x_T"], c["goal"], c["sig"], candidates=K, pin=pin,
                                     noise=c["rows"] if kind == "euler_ancestral" else None, **kw)
    ctx = model.inner_model.latent_encoder_emb.clone()
    scores = model.denoising_score(c["state"], chunks, c["goal"], c["levels"], c["snoise"], candidates=K)
    best, index = gs.best_candidates(chunks, scores, K)
    return best, index, scores, chunks, ctx


def one_call(model, c, K, kind, pin=None, lam=None):
    kw = {} if lam is None else {"cond_lambda": lam}
    out = model.sample_select(c["state"], c["x_T"], c["goal"], c["sig"], c["levels"], K, kind=None if kind == "ddim" else kind,
                              noise=c["rows"] if kind == "euler_ancestral" else None, pin=pin, score_noise=c["snoise"], **kw)
    return out + (model.inner_model.latent_encoder_emb.clone(),)


def check_equal(name, B, K, S, M, kind, pinned):
    model, _ = model_of(name)
    c = case(name, B, K, S, M)
    pin = c["pin"] if pinned else None
    held = {k: c[k].clone() for k in ("x_T", "snoise", "rows", "goal")}
    held_pin = tuple(t.clone() for t in c["pin"])
    want = three_calls(model, c, K, kind, pin)
    got = one_call(model, c, K, kind, pin)
    torch.cuda.synchronize()
    for what, g, w in zip(("best", "index", "scores", "chunks", "ctx_out"), got, want):
        if what == "index":
            assert g.dtype == torch.int64 and torch.equal(g, w), (name, kind, what, g.tolist(), w.tolist())
        else:
            assert same_bits(g, w), (name, (B, K, S, M), kind, pinned, what, float((g - w).abs().max()))
    assert tuple(got[0].shape) == (B,) + tuple(c["x_T"].shape[1:]) and tuple(got[2].shape) == (B * K,)
    assert bool(torch.isfinite(got[2]).all())
    for k, v in held.items():
        assert same_bits(c[k], v), f"{k} was written"
    assert all(same_bits(a, b) for a, b in zip(c["pin"], held_pin)), "the pin was written"


@pytest.mark.parametrize("pinned", [False, True], ids=["plain", "pin"])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m", "euler_ancestral"])
@pytest.mark.parametrize("B,K,S,M", CASES)
def test_the_one_call_has_the_bits_of_the_three(B, K, S, M, kind, pinned):
    check_equal("mdtv_tiny", B, K, S, M, kind, pinned)


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m", "euler_ancestral"])
def test_the_one_call_has_the_bits_of_the_three_at_the_shipped_width(kind):
    check_equal("mdtv_default", *SHIPPED, kind, kind == "ddim")


@pytest.mark.parametrize("kind", ["ddim", "euler_ancestral"])
@pytest.mark.parametrize("name", ["mdt_tiny", "g11_mdtv_noise_block", "g11_mdtv_no_ada"])
def test_the_one_call_has_the_bits_of_the_three_on_the_other_models(name, kind):
    """MDT (two camera tokens), the NoiseBlock decoder, and sigma as a context token, whose score phase shares nothing: it stages
    and encodes the B * S contexts the stand-alone call encodes."""
    check_equal(name, 3, 5, 3, 2, kind, kind == "ddim")


@pytest.mark.parametrize("name,B,K,S,M", [("mdtv_tiny", 3, 5, 3, 2), ("mdtv_default",) + SHIPPED])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_a_guided_call_scores_the_conditional_model(name, B, K, S, M, kind):
    model, P = model_of(name)
    cfg, arch, _ = entry(name)
    c = case(name, B, K, S, M)
    want = three_calls(model, c, K, kind, lam=2.0)
    best, index, scores, chunks, ctx = one_call(model, c, K, kind, lam=2.0)
    torch.cuda.synchronize()
    assert same_bits(chunks, want[3]), "chunks against the guided *_multi call"
    assert same_bits(ctx, want[4]), "ctx_out against the guided *_multi call"
    ref, terms = residual_score(P, cfg, arch, c["host_state"], c["host_goal"], chunks.cpu(), c["levels"], c["snoise"].cpu(), K=K,
                                dtype=torch.float64)
    f32, _ = residual_score(P, cfg, arch, c["host_state"], c["host_goal"], chunks.cpu(), c["levels"], c["snoise"].cpu(), K=K,
                            dtype=torch.float32)
    bound = 3 * float((f32.double() - ref).abs().max()) + 8 * EPS32 * terms
    err = (scores.cpu().double() - ref).abs()
    i = int((err / bound).argmax())
    print(f"{name} {kind} guided (B, K, S, M)=({B}, {K}, {S}, {M}): |score - float64| {float(err[i]):.3e} / bound {float(bound[i]):.3e}; "
          f"bits equal to the stand-alone scorer: {same_bits(scores, want[2])}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    want_best, want_index = gs.best_candidates(chunks, scores, K)
    assert torch.equal(index, want_index) and same_bits(best, want_best)
    assert same_bits(best, chunks.reshape(B, K, *chunks.shape[1:])[torch.arange(B), index])


@pytest.mark.parametrize("kind", ["ddim", "dpmpp_2m"])
def test_one_candidate_gives_the_opt_calls_chunk(kind):
    name, B = "mdtv_tiny", 3
    model, _ = model_of(name)
    c = case(name, B, 1, 3, 2)
    if kind == "ddim":
        want = model.sample_ddim(c["state"], c["x_T"], c["goal"], c["sig"], pin=c["pin"])
    else:
        want = model.sample_native(kind, c["state"], c["x_T"], c["goal"], c["sig"], pin=c["pin"])
    best, index, scores, chunks, _ = one_call(model, c, 1, kind, pin=c["pin"])
    assert same_bits(best, want) and same_bits(chunks, want) and index.tolist() == [0] * B and tuple(scores.shape) == (B,)


def test_the_layout_of_action_is_the_layout_of_the_results():
    name, B, K, S, M = "mdtv_tiny", 3, 5, 3, 2
    model, _ = model_of(name)
    c = case(name, B, K, S, M)
    flat = gs.sample_select(model, c["state"], c["x_T"], c["goal"], c["sig"], c["levels"], noise=c["snoise"],
                              extra_args={"candidates": K})
    x4 = c["x_T"].reshape(B, K, *c["x_T"].shape[1:])
    grid = gs.sample_select(model, c["state"], x4, c["goal"], c["sig"], c["levels"], noise=c["snoise"], extra_args={"candidates": K})
    assert tuple(flat[2].shape) == (B * K,) and tuple(grid[2].shape) == (B, K) and grid[3].shape == x4.shape
    assert tuple(grid[0].shape) == (B,) + tuple(c["x_T"].shape[1:]) and grid[1].dtype == torch.int64
    for a, b in zip(flat, grid):
        assert same_bits(a.reshape(-1).float(), b.reshape(-1).float())


def test_a_captured_call_replays_the_eager_bits_and_the_workspace_stays():
    name, B, K, S, M = "mdtv_tiny", 1, 8, 3, 2
    model, _ = model_of(name)
    cs = [case(name, B, K, S, M, seed=s) for s in (None, 71, 72, 73)]
    c = cs[0]
    eng = model._engine(state=c["state"])
    run = lambda x, rows, snoise, pin: model.sample_select(c["state"], x, c["goal"], c["sig"], c["levels"], K, kind="euler_ancestral",
                                                           noise=rows, pin=pin, score_noise=snoise)
    eager = [tuple(t.clone() for t in run(d["x_T"], d["rows"], d["snoise"], d["pin"])) for d in cs]  # the first sizes the workspace
    assert not same_bits(eager[1][0], eager[2][0])
    gen = int(eng.lib.mdt_ws_generation(eng.handle))
    static = [c["x_T"].clone(), c["rows"].clone(), c["snoise"].clone(), c["pin"][0].clone(), c["pin"][1].clone()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(static[0], static[1], static[2], (static[3], static[4]))
    for i in (1, 2, 3):
        d = cs[i]
        for dst, src in zip(static, (d["x_T"], d["rows"], d["snoise"], d["pin"][0], d["pin"][1])):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for what, g, w in zip(("best", "index", "scores", "chunks"), out, eager[i]):
            assert same_bits(g.float(), w.float()), f"replay {i}: {what}"
        assert int(eng.lib.mdt_ws_generation(eng.handle)) == gen, "the workspace moved"


def test_the_facade_replays_the_third_identical_call(monkeypatch):
    name, B, K, S, M = "mdtv_tiny", 1, 8, 3, 2
    model, _ = model_of(name)
    g = gs
    monkeypatch.setattr(g, "_GRAPH_MODE", "auto")
    monkeypatch.setattr(g, "_GRAPH_SAMPLER", False)
    for k in ("_graphed_select", "_graph_seen", "_graph_failed"):
        model.__dict__.pop(k, None)
    cs = [case(name, B, K, S, M, seed=s) for s in (81, 82, 83, 84)]
    call = lambda d: g.sample_select(model, d["state"], d["x_T"], d["goal"], d["sig"], d["levels"], sampler="euler_ancestral",
                                     noise=d["snoise"], extra_args={"candidates": K})
    outs = []
    for d in cs:
        torch.manual_seed(5)  # the sampler's noise rows are drawn inside: the same for the eager twin below
        outs.append(tuple(t.clone() for t in call(d)))
    assert len(model.__dict__.get("_graphed_select", [])) == 1, "the third call did not build a graph"
    monkeypatch.setattr(g, "_GRAPH_MODE", "0")
    for d, got in zip(cs, outs):
        torch.manual_seed(5)
        want = call(d)
        for what, a, b in zip(("best", "index", "scores", "chunks"), got, want):
            assert a.dtype == b.dtype and same_bits(a.float(), b.float()), what
    assert len(model.__dict__["_graphed_select"]) == 1
    assert outs[2][0].data_ptr() != outs[3][0].data_ptr()
    model.__dict__.pop("_graphed_select", None)
