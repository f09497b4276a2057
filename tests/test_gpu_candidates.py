"""K action chunks per observation from one shared context on the MI355X (pytest -m gpu): mdt_sample*_multi and
``candidates=`` through GCDenoiser and gc_sampling.

Yardsticks: the float64 oracle (oracle/mdt_oracle.py) on inputs replicated with ``repeat_interleave``, and the plain native call
at batch B*K on the same replicated inputs, both at the sampler gate of tests/helpers (rtol 1e-3, atol 1e-4).  Bits cannot be
asked between a (B, K) call and the replicated one -- the encoder runs at B in one and at B*K in the other, which may be other
dispatcher regimes -- and are asked where the launches are the same: candidates = 1 against the ``_opt`` entries, the context
against the plain call at batch B, a graph replay against the eager call, a (B, K, Ta, A) action against its (B*K, Ta, A) form,
a per-observation pin against its hand-expanded per-chunk one.

10 steps of the exponential 80 -> 0.001 schedule.  Every observation has its own tokens and goal (independent normal draws) and
B is no power of two wherever B > 1, so an index that is ``s``, ``s % B`` or ``s / K`` of another K reads another
observation's context or rows nobody wrote.  euler_ancestral and dpmpp_sde have no float64 oracle loop: they are held against
the replicated native call alone (the same noise rows: drawn from one seed, or from the same B*K tree seeds)."""
import ctypes as C

import pytest
import torch

from mdt_policy_amd import _lib, configs, synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from oracle import mdt_oracle as O
from tests.family import Family
from tests.helpers import assert_close, cuda, observation, to

pytestmark = pytest.mark.gpu

N, SMIN, SMAX = 10, 0.001, 80.0
CONFIGS = {
    "mdtv_tiny": dict(cfg=configs.mdtv_tiny(), arch="mdtv", proprio=False),          # d = 128, hd = 16: every fused form
    "mdtv_default": dict(cfg=configs.mdtv_default(), arch="mdtv", proprio=False),    # d = 384, hd = 48: k_attn_xattn
    # the explicit cross-attention (k_attn reads the K|V rows): RoPE, NoiseBlock, the proprio token (Te = 5), sigma as a context
    # token (the encoder runs per step, at B), MDT
    # (RoPE rotates 32 dims of a head: 4 heads of 32 at d = 128, the tiny rotary configuration of tests/golden/make_golden.py)
    "rope": dict(cfg=configs.mdtv_tiny(use_rot_embed=True, n_heads=4), arch="mdtv", proprio=False),
    "noise_block": dict(cfg=configs.mdtv_tiny(use_noise_encoder=True), arch="mdtv", proprio=False),
    "state_obs": dict(cfg=configs.mdtv_tiny(), arch="mdtv", proprio=True),
    "sigma_token": dict(cfg=configs.mdtv_tiny(use_ada_conditioning=False), arch="mdtv", proprio=False),
    "mdt_tiny": dict(cfg=configs.mdt_tiny(), arch="mdt", proprio=False),
}
_REFS = {}
model_of = Family(None, CONFIGS).model_of   # (model, float32 state dict): 'rich' synthetic weights


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():  # every call here is inference: the facade refuses to run under autograd
        yield


def sched():
    return gs.get_sigmas_exponential(N, SMIN, SMAX)


def case(name, B, K, seed=None):
    """Host inputs of a (B, K) call: state and goal per observation, x_T per chunk, and the two replicated with repeat_interleave."""
    e = CONFIGS[name]
    seed = 1000 + 17 * B + K if seed is None else seed
    state, goal, _ = observation(e["cfg"], e["arch"], e["proprio"], B, seed)
    x = torch.from_numpy(synthetic.sampler_inputs(B * K, e["cfg"], seed + 1, e["arch"])["noise"]) * SMAX
    return state, goal, x, to(state, lambda v: v.repeat_interleave(K, 0)), goal.repeat_interleave(K, 0)


def no_forward(mp):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    mp.setattr(GCDenoiser, "forward", boom)


def oracle(name, sampler, wide, x, wide_goal):
    e = CONFIGS[name]
    _, P = model_of(name)
    st = {k: (v.double() if torch.is_tensor(v) else v) for k, v in wide.items()}
    return sampler(O.to_dtype(P, torch.float64), e["cfg"], st, x.double(), wide_goal.double(), sched().double(), arch=e["arch"],
                   hoist=True)


def check_ddim(name, B, K, monkeypatch):
    model, _ = model_of(name)
    state, goal, x, wide, wide_goal = case(name, B, K)
    want = oracle(name, O.sample_ddim, wide, x, wide_goal)
    no_forward(monkeypatch)
    with torch.no_grad():
        got = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sched(), extra_args={"candidates": K})
        ctx = model.inner_model.latent_encoder_emb
        plain = gs.sample_ddim(model, cuda(wide), x.cuda(), wide_goal.cuda(), sched())
    e = model._engine(state=cuda(state))
    assert tuple(got.shape) == (B * K, e.Ta, e.A) and tuple(ctx.shape) == (B, e.Te, e.D)
    assert_close(got.cpu(), want, what=f"{name} ({B}, {K}) against float64")
    assert_close(got.cpu(), plain.cpu(), what=f"{name} ({B}, {K}) against the replicated native call")


# ---- 1: one decoder batch per cross-attention form (DDIM) ------------------------------------------------------------------------
# (1, 2): 2 chunks, the cross-attention inside c_fc (XATTN_FC_MAX_BATCH); (3, 2): 6, k_attn_proj + the stand-alone k_xattn_apply;
# (7, 5): 35, above ATTN_PROJ_MAX_BATCH -- at d = 384 k_attn_xattn takes it (350 rows >= 200); (65, 8): 520, above
# ATTN_XATTN_MAX_BATCH: the stand-alone apply again
@pytest.mark.parametrize("B,K", [(1, 2), (3, 2), (7, 5), (65, 8)])
def test_ddim_on_each_collapsed_cross_attention_route(B, K, monkeypatch):
    check_ddim("mdtv_tiny", B, K, monkeypatch)


def test_ddim_through_k_attn_xattn_at_d384(monkeypatch):
    check_ddim("mdtv_default", 7, 5, monkeypatch)


# ---- 2: the explicit k_attn cross path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(3, 2), (7, 5)])
@pytest.mark.parametrize("name", ["rope", "noise_block", "state_obs", "sigma_token", "mdt_tiny"])
def test_ddim_on_the_explicit_cross_attention(name, B, K, monkeypatch):
    check_ddim(name, B, K, monkeypatch)


# ---- 3: plan kinds at (3, 2) -----------------------------------------------------------------------------------------------------
def run_kind(kind, model, state, x, goal, extra_args=None, **kw):
    torch.manual_seed(23)  # the noise rows of the ancestral kinds: one draw per step in the action's shape, so per chunk
    with torch.no_grad():
        return getattr(gs, "sample_" + kind)(model, state, x, goal, sched(), extra_args=extra_args, **kw)


@pytest.mark.parametrize("kind", ["heun", "euler_ancestral", "dpmpp_2m", "dpmpp_sde"])
def test_plan_kinds(kind, monkeypatch):
    B, K = 3, 2
    model, _ = model_of("mdtv_tiny")
    state, goal, x, wide, wide_goal = case("mdtv_tiny", B, K)
    no_forward(monkeypatch)
    kw = {}
    if kind == "dpmpp_sde":  # tree noise, one tree per chunk: B*K seeds
        sig = sched()
        kw["noise_sampler"] = gs.NativeBrownianTreeNoiseSampler(x.cuda(), sig[sig > 0].min(), sig.max(),
                                                                 seed=[101 + i for i in range(B * K)])
    got = run_kind(kind, model, cuda(state), x.cuda(), goal.cuda(), {"candidates": K}, **kw)
    plain = run_kind(kind, model, cuda(wide), x.cuda(), wide_goal.cuda(), None, **kw)
    assert tuple(model.inner_model.latent_encoder_emb.shape)[0] == B * K  # (the replicated call's)
    assert_close(got.cpu(), plain.cpu(), what=f"{kind} against the replicated native call")
    if kind in ("heun", "dpmpp_2m"):
        want = oracle("mdtv_tiny", getattr(O, "sample_" + kind), wide, x, wide_goal)
        assert_close(got.cpu(), want, what=f"{kind} against float64")
    if kind in ("euler_ancestral", "dpmpp_sde"):  # the chunks of one observation got different noise rows
        assert float((got[0] - got[1]).abs().max()) > 1e-3


# ---- 4: options together, heun (3, 2) --------------------------------------------------------------------------------------------
def heun_case():
    if "heun" not in _REFS:
        model, _ = model_of("mdtv_tiny")
        state, goal, x, wide, wide_goal = case("mdtv_tiny", 3, 2)
        _REFS["heun"] = (model, cuda(state), goal.cuda(), x.cuda(), cuda(wide), wide_goal.cuda())
    return _REFS["heun"]


def hard_pin(x, seed):
    """A per-observation pin (3 observations): the first two tokens hard, a ``known`` of the chunks' own scale."""
    known = torch.from_numpy(synthetic.normal("known", (3,) + tuple(x.shape[1:]), seed)).cuda()
    keep = torch.zeros(x.shape[1])
    keep[:2] = 1.0
    return ActionPin(known, keep.cuda())


def test_guidance_alone(monkeypatch):
    model, state, goal, x, wide, wide_goal = heun_case()
    no_forward(monkeypatch)
    got = run_kind("heun", model, state, x, goal, {"candidates": 2, "cond_lambda": 3.0})
    ctx = model.inner_model.latent_encoder_emb
    plain = run_kind("heun", model, wide, x, wide_goal, {"cond_lambda": 3.0})
    free = run_kind("heun", model, state, x, goal, {"candidates": 2})
    assert float((got - free).abs().max()) > 1e-2  # the weight did something
    assert ctx.shape[0] == 3
    assert_close(got.cpu(), plain.cpu(), what="guided heun against the replicated guided call")


def test_bounds_pin_and_record_together():
    model, state, goal, x, wide, wide_goal = heun_case()
    K = 2
    pin = hard_pin(x, 77)
    chunk_pin = ActionPin(pin.known.repeat_interleave(K, 0), pin.keep)  # the hand-expanded per-chunk pin
    with torch.no_grad():
        free = model.sample_native("heun", state, x, goal, sched(), pin=pin, candidates=K)
        rows = free.reshape(-1, free.shape[-1]).float().cpu()
        lo, hi = torch.quantile(rows, 0.3, dim=0), torch.quantile(rows, 0.7, dim=0)
        got, rec = model.sample_native("heun", state, x, goal, sched(), bounds=(lo, hi), record=True, pin=pin, candidates=K)
        same = model.sample_native("heun", state, x, goal, sched(), bounds=(lo, hi), pin=chunk_pin, candidates=K)
        want, wrec = model.sample_native("heun", wide, x, wide_goal, sched(), bounds=(lo, hi), record=True, pin=chunk_pin)
    assert float((got - free).abs().max()) > 1e-2  # the bounds clipped
    assert torch.equal(got, same), "a per-observation pin is not its hand-expanded per-chunk pin"
    assert_close(got.cpu(), want.cpu(), what="heun with bounds and a pin against the replicated call")
    assert tuple(rec["x"].shape) == (N, 6) + tuple(x.shape[1:])
    for k in ("x", "denoised"):
        assert_close(rec[k].cpu(), wrec[k].cpu(), what=f"record {k}")
    known, keep = chunk_pin.on(x.device, x.shape)
    for i in range(N):
        assert torch.equal(rec["denoised"][i][keep == 1], known[keep == 1]), "the recorded denoised is not D'"
    # keep == 1 elements arrive at known (clamped like everything else: the bounds come after the pin)
    arrive = torch.clamp(known, lo.cuda(), hi.cuda())
    assert_close(got[:, :2].cpu(), arrive[:, :2].cpu(), what="the hard tokens")


def test_guidance_with_a_pin(monkeypatch):
    model, state, goal, x, wide, wide_goal = heun_case()
    K = 2
    pin = hard_pin(x, 78)
    chunk_pin = ActionPin(pin.known.repeat_interleave(K, 0), pin.keep)
    no_forward(monkeypatch)
    got = run_kind("heun", model, state, x, goal, {"candidates": K, "cond_lambda": 3.0, "pin": pin})
    same = run_kind("heun", model, state, x, goal, {"candidates": K, "cond_lambda": 3.0, "pin": chunk_pin})
    plain = run_kind("heun", model, wide, x, wide_goal, {"cond_lambda": 3.0, "pin": chunk_pin})
    assert torch.equal(got, same), "a per-observation pin is not its hand-expanded per-chunk pin"
    assert_close(got.cpu(), plain.cpu(), what="guided pinned heun against the replicated call")
    assert_close(got[:, :2].cpu(), chunk_pin.known[:, :2].cpu(), what="the hard tokens arrive at known")


# ---- 5: bitwise checks -----------------------------------------------------------------------------------------------------------
def entry(name, model, state, x_T, goal, K=None, lam=1.0, kind=None):
    """``out`` and ``ctx_out`` of one sampler entry called as a C client calls it: an ``_opt`` entry (K None) or its ``_multi``
    twin with ``candidates`` = K; ``kind`` for the plan family; the schedule goes to the device for a ``_dev`` entry."""
    eng = model._engine(state=state)
    eng.sync_params()
    tok, tok2, B = eng._tokens(state)
    g = eng._goal(model.inner_model._goals(goal, False), B)
    x = eng._in(x_T)  # (a refused call reads none of it: its chunk count need not fit)
    out = torch.empty_like(x)
    ctx = torch.empty((B, eng.Te, eng.D), device=x.device, dtype=torch.float32)
    vals = [float(v) for v in sched()]
    if "_dev" in name:
        sig = torch.tensor(vals, device=x.device, dtype=torch.float32)
        sig_arg = sig.data_ptr()
    else:
        sig = sig_arg = (C.c_float * len(vals))(*vals)
    opts = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), lam, None, None, None, None, None, None)
    mid = (sig_arg, N) if kind is None else (_lib.SAMPLER_KIND[kind], C.byref(_lib.sampler_params()), sig_arg, N, None, 0)
    count = (B,) if K is None else (B, K)
    eng.ctx_generation += 1
    st = getattr(_lib.load(), name)(eng.handle, tok.data_ptr(), None if tok2 is None else tok2.data_ptr(), g.data_ptr(),
                                    eng._modality(state), x.data_ptr(), *mid, *count, out.data_ptr(), ctx.data_ptr(),
                                    C.byref(opts), eng._stream())
    if st != 0:
        raise _lib.MDTHipError(st, _lib.load().mdt_last_error().decode("utf-8", "replace"))
    torch.cuda.synchronize()
    return out, ctx


@pytest.mark.parametrize("lam", [1.0, 3.0])
@pytest.mark.parametrize("B", [2, 35])
def test_one_candidate_is_the_opt_entry_bit_for_bit(B, lam):
    model, _ = model_of("mdtv_tiny")
    state, goal, x, _, _ = case("mdtv_tiny", B, 1)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    for multi, opt, kind in (("mdt_sample_ddim_multi", "mdt_sample_ddim_opt", None),
                             ("mdt_sample_ddim_dev_multi", "mdt_sample_ddim_dev_opt", None),
                             ("mdt_sample_multi", "mdt_sample_opt", "heun"),
                             ("mdt_sample_dev_multi", "mdt_sample_dev_opt", "heun")):
        want, wctx = entry(opt, model, state, x, goal, lam=lam, kind=kind)
        got, gctx = entry(multi, model, state, x, goal, K=1, lam=lam, kind=kind)
        assert torch.equal(got, want) and torch.equal(gctx, wctx), f"{multi} with candidates = 1 is not {opt}"


@pytest.mark.parametrize("lam", [None, 3.0])
@pytest.mark.parametrize("name,B,K", [("mdtv_tiny", 3, 2), ("mdtv_tiny", 7, 5), ("mdtv_default", 7, 5), ("state_obs", 3, 2)])
def test_the_context_is_the_plain_calls_at_batch_b(name, B, K, lam):
    """The same encoder launches: ctx_out of a (B, K) call is ctx_out of the plain call on the B observations; guided, the
    conditional half."""
    model, _ = model_of(name)
    state, goal, x, _, _ = case(name, B, K)
    kw = {} if lam is None else {"cond_lambda": lam}
    with torch.no_grad():
        model.sample_ddim(cuda(state), x.cuda(), goal.cuda(), sched(), candidates=K, **kw)
        got = model.inner_model.latent_encoder_emb.clone()
        model.sample_ddim(cuda(state), x[::K].contiguous().cuda(), goal.cuda(), sched(), **kw)
        want = model.inner_model.latent_encoder_emb
    assert tuple(got.shape) == tuple(want.shape) and got.shape[0] == B
    assert torch.equal(got, want)


def test_repeats_replay_a_graph_with_the_eager_bits(monkeypatch):
    model, _ = model_of("mdtv_tiny")
    g = gs
    monkeypatch.setattr(g, "_GRAPH_MODE", "auto")  # the rollout rule: chunks <= 8, from the third identical call on
    monkeypatch.setattr(g, "_GRAPH_SAMPLER", False)
    model.__dict__.pop("_graphed_samplers", None)
    model.__dict__.pop("_graph_seen", None)
    state, goal, x, _, _ = case("mdtv_tiny", 1, 4)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    with torch.no_grad():
        eager = model.sample_ddim(state, x, goal, sched(), candidates=4)
        ectx = model.inner_model.latent_encoder_emb.clone()
        outs = [g.sample_ddim(model, state, x, goal, sched(), extra_args={"candidates": 4}) for _ in range(4)]
    graphs = model.__dict__.get("_graphed_samplers")
    assert graphs and len(graphs) == 1 and graphs[0].candidates == 4, "the replay path was not taken"
    assert all(torch.equal(o, eager) for o in outs)
    assert torch.equal(model.inner_model.latent_encoder_emb, ectx) and ectx.shape[0] == 1
    # another K: another graph (the shapes of the call below differ in nothing but the meaning of the 4 rows)
    state2, goal2, x2, _, _ = case("mdtv_tiny", 2, 2)
    state2, goal2, x2 = cuda(state2), goal2.cuda(), x2.cuda()
    with torch.no_grad():
        eager2 = model.sample_ddim(state2, x2, goal2, sched(), candidates=2)
        outs2 = [g.sample_ddim(model, state2, x2, goal2, sched(), extra_args={"candidates": 2}) for _ in range(4)]
    assert len(model._graphed_samplers) == 2 and sorted(gr.candidates for gr in model._graphed_samplers) == [2, 4]
    assert all(torch.equal(o, eager2) for o in outs2)
    with torch.no_grad():  # and the first graph still serves its call
        assert torch.equal(g.sample_ddim(model, state, x, goal, sched(), extra_args={"candidates": 4}), eager)
    assert len(model._graphed_samplers) == 2


def test_a_four_dimensional_action_gives_the_same_bits_in_its_shape():
    model, _ = model_of("mdtv_tiny")
    B, K = 3, 2
    state, goal, x, _, _ = case("mdtv_tiny", B, K)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    x4 = x.reshape(B, K, *x.shape[1:])
    with torch.no_grad():
        flat = model.sample_ddim(state, x, goal, sched(), candidates=K)
        four = model.sample_ddim(state, x4, goal, sched(), candidates=K)
        torch.manual_seed(4)
        flat_e = gs.sample_euler_ancestral(model, state, x, goal, sched(), extra_args={"candidates": K})
        torch.manual_seed(4)
        four_e = gs.sample_euler_ancestral(model, state, x4, goal, sched(), extra_args={"candidates": K})
    assert tuple(four.shape) == tuple(x4.shape) and torch.equal(four.reshape(flat.shape), flat)
    assert tuple(four_e.shape) == tuple(x4.shape) and torch.equal(four_e.reshape(flat_e.shape), flat_e)


# ---- refusals that need a handle -------------------------------------------------------------------------------------------------
def test_a_chunk_count_beyond_the_decoders_rows_is_refused_by_name():
    """batch * candidates beyond what the decoder's int row counts hold (2^24 / max(Te, Ta) samples), the doubled count when
    guided: MDT_ERR_INVALID_ARG before anything is enqueued, and the handle stays usable."""
    model, _ = model_of("mdtv_tiny")
    state, goal, x, _, _ = case("mdtv_tiny", 3, 2)
    state, goal, x = cuda(state), goal.cuda(), x.cuda()
    limit = (1 << 24) // 10
    for name, kind in (("mdt_sample_ddim_multi", None), ("mdt_sample_dev_multi", "heun")):
        for K, lam in ((limit // 3 + 1, 1.0), (limit // 6 + 1, 3.0)):
            with pytest.raises(_lib.MDTHipError) as err:
                entry(name, model, state, x, goal, K=K, lam=lam, kind=kind)
            assert err.value.status == 1 and name in str(err.value) and "candidates" in str(err.value), err.value
            assert ("doubled" in str(err.value)) == (lam != 1.0)
        with pytest.raises(_lib.MDTHipError) as err:
            entry(name, model, state, x, goal, K=0, kind=kind)
        assert err.value.status == 1 and name in str(err.value) and "candidates" in str(err.value)
    with torch.no_grad():
        a = model.sample_ddim(state, x, goal, sched(), candidates=2)
        b = entry("mdt_sample_ddim_multi", model, state, x, goal, K=2)[0]
    assert torch.equal(a, b)
    with pytest.raises(ValueError) as err:
        model.sample_ddim(state, x[:5], goal, sched(), candidates=2)
    assert "5" in str(err.value) and "6" in str(err.value)
