"""Train mode (dropout on) against float64 oracles that replay the library's masks (pytest -m gpu).

The masks of a train-mode forward are counter based: one seed per forward (HipScoreNetwork.train_dropout draws it from torch's
CPU generator), one site per (block, place), the element's own flat index.  tests/dropout_masks.py restates them in numpy, the
oracle (oracle/mdt_oracle.py, ``masks=``) multiplies with them at the reference's dropout places, and torch autograd in float64
gives what the HIP step has to compute: loss, model output, context, EVERY parameter gradient and the input gradients.

Tolerances are the eval-mode tests' own (test_train_grads.py, test_c3_step.py): loss 1e-3 relative, outputs and context rtol 1e-3 /
atol 1e-4, gradients rtol 2e-3 and atol 2e-3 * max |ref| + 1e-7 per tensor.  Dropout changes no arithmetic -- it zeroes and
rescales operands -- so they carry over; every check prints its largest error as a fraction of its tolerance."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests import dropout_masks as DM
from tests.helpers import assert_close, cfg_of, inputs_of, load_fixture, params_of

pytestmark = pytest.mark.gpu

G11 = ["mdtv_tiny", "mdt_tiny", "mdtv_default", "mdtv_rope", "mdt_rope", "mdtv_noise_block", "mdtv_no_ada", "mdt_no_ada",
       "mdtv_mlp_head", "mdtv_no_goal_cond", "mdt_no_goal_cond"]


class CachedMasks(DM.Masks):
    """The oracle asks for a block's masks twice when a test runs loss and encode: keep what was generated."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._memo = {}

    def _t(self, site, shape, p):
        key = (site, tuple(shape), p)
        if key not in self._memo:
            self._memo[key] = super()._t(site, shape, p)
        return self._memo[key].clone()


def load_case(name, B=None, overrides=None):
    if name.startswith("proprio_"):
        meta, _ = load_fixture(f"g16_{name}.npz")
    else:
        meta, _ = load_fixture(f"g11_grads_{name}.npz")
    cfg = dict(cfg_of(meta), **(overrides or {}))
    B = B or meta["B"]
    state, goal, _ = inputs_of(meta, batch=B)
    if name.startswith("proprio_"):
        state["state_obs"] = torch.from_numpy(synthetic.normal("state_obs", (B, 1, cfg["proprio_dim"]), meta["obs_seed"]))
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, meta["loss_seed"]).items()}
    return meta, cfg, state, goal, li


def facade(meta, cfg):
    """The model in train() mode and the list its dropout seeds are appended to, in call order."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model = GCDenoiser(cfg, 0.5)
    model.load_state_dict(params_of(meta))
    model = model.cuda().train()
    return model, spy_seeds(model.inner_model)


def spy_seeds(im):
    seeds, orig = [], im.train_dropout

    def train_dropout():
        d = orig()
        seeds.append(int(d.seed))
        return d

    im.train_dropout = train_dropout
    return seeds


def replayed_goal_keep(cfg, goal, torch_seed):
    """mask_cond's Bernoulli draw of the forward that ran under torch.manual_seed(torch_seed) (the first draw on the device's
    generator), as test_goal_masking_draws_the_reference_bernoulli_stream replays it; None without goal masking."""
    p = float(cfg.get("goal_drop", 0) or 0)
    if p <= 0:
        return None
    shape = goal.shape if goal.dim() == 3 else (goal.shape[0], 1, goal.shape[1])
    torch.manual_seed(torch_seed)
    return (1.0 - torch.bernoulli(torch.ones(shape, device="cuda") * p)).cpu().double()


def on_device(fn):
    """The float64 oracle on the GPU's fp64 units, on the host where one of its ops has no device kernel."""
    try:
        return fn("cuda")
    except (RuntimeError, NotImplementedError):
        return fn("cpu")


def oracle_leaves(meta, state, goal, dev):
    P = {k: v.double().to(dev).requires_grad_(v.dtype.is_floating_point) for k, v in params_of(meta).items()}
    st = {k: (v.double().to(dev).requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    return P, st, goal.double().to(dev).requires_grad_()


def goal_in(g64, keep):
    if keep is None:
        return g64
    return (g64 if g64.dim() == 3 else g64[:, None, :]) * keep.to(g64.device)


def grads_of(P, st, g64):
    out = {k: (v.grad.cpu() if v.grad is not None else None) for k, v in P.items()}
    out.update({"d_" + k: v.grad.cpu() for k, v in st.items() if torch.is_tensor(v) and v.grad is not None})
    out["d_goal"] = g64.grad.cpu() if g64.grad is not None else None
    return out


def oracle_loss_step(meta, cfg, state, goal, li, seed, keep=None, ctx_coef=0.1):
    """loss + ctx_coef * <ctx, w> / numel through the masked float64 oracle -> (loss, model_output, ctx, {name: gradient})."""
    def run(dev):
        P, st, g64 = oracle_leaves(meta, state, goal, dev)
        l = {k: v.double().to(dev) for k, v in li.items()}
        masks = CachedMasks.of(seed, cfg)
        g = goal_in(g64, keep)
        lo, mo = O.loss(P, cfg, st, l["actions"], g, l["noise_train"], l["sigma"], arch=meta["arch"], masks=masks)
        ctx = O.encode(P, cfg, st, g, meta["arch"], "forward", sigma=l["sigma"], masks=masks)
        w = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), meta["ctx_seed"])).double().to(dev)
        (lo + ctx_coef * (ctx * w).sum() / ctx.numel()).backward()
        return lo.item(), mo.detach().cpu(), ctx.detach().cpu(), grads_of(P, st, g64)
    return on_device(run)


def hip_loss_step(model, meta, state, goal, li, torch_seed, ctx_coef=0.1):
    gstate = {k: (v.cuda().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    ggoal = goal.cuda().requires_grad_()
    model.zero_grad(set_to_none=True)
    torch.manual_seed(torch_seed)
    loss, mo = model.loss(gstate, li["actions"].cuda(), ggoal, li["noise_train"].cuda(), li["sigma"].cuda())
    ctx = model.inner_model.latent_encoder_emb
    w = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), meta["ctx_seed"])).cuda()
    (loss + ctx_coef * (ctx * w).sum() / ctx.numel()).backward()
    torch.cuda.synchronize()
    return loss.item(), mo.detach().cpu(), ctx.detach().cpu(), hip_grads(model, gstate, ggoal)


def hip_grads(model, gstate, ggoal):
    got = {"inner_model." + k: (p.grad.cpu() if p.grad is not None else None) for k, p in model.inner_model.named_parameters()}
    got.update({"d_" + k: v.grad.cpu() for k, v in gstate.items() if torch.is_tensor(v) and v.grad is not None})
    got["d_goal"] = ggoal.grad.cpu() if ggoal.grad is not None else None
    return got


def worst(got, want, rtol, atol):
    err = (got.double() - want.double()).abs()
    return float((err / (atol + rtol * want.double().abs())).max())


def check_gradients(got, ref, what, at_least, zero_is_none=False):
    """zero_is_none: the context-only backward hands every parameter of the handle a gradient, exact zeros for the decoder's."""
    n, top = 0, (0.0, "")
    for k, g in got.items():
        r = ref.get(k)
        if r is None:   # a parameter this forward never reads (or an unused goal): no gradient on either side
            assert g is None or ((zero_is_none or k == "d_goal") and float(g.abs().max()) == 0.0), \
                f"{what} {k}: a gradient where the oracle has none"
            continue
        assert g is not None, f"{what} {k}: no gradient"
        atol = 2e-3 * float(r.abs().max()) + 1e-7
        top = max(top, (worst(g, r, 2e-3, atol), k))
        assert_close(g, r, rtol=2e-3, atol=atol, what=f"{what} {k}")
        n += 1
    assert set(k for k, v in ref.items() if v is not None) <= set(got), what
    print(f"{what}: {n} gradients, largest error {top[0]:.3f} of its tolerance ({top[1]})")
    assert n >= at_least, (what, n)


def check_step(hip, ref, what, at_least):
    (lh, moh, ch, gh), (lo, moo, co, go) = hip, ref
    print(f"{what}: loss {lh:.7g} / oracle {lo:.7g} ({abs(lh - lo) / abs(lo):.2e} relative); model_output "
          f"{worst(moh, moo, 1e-3, 1e-4):.3f}, context {worst(ch, co, 1e-3, 1e-4):.3f} of their tolerances")
    assert abs(lh - lo) <= 1e-3 * abs(lo), (what, lh, lo)
    assert_close(moh, moo, what=what + " model_output")
    assert_close(ch, co, what=what + " latent_encoder_emb")
    check_gradients(gh, go, what, at_least)


# (name, overrides): the g11 configurations at the shipped probabilities (0.3 / 0.1 / 0.05); embed_pdrob = 0.1 where the
# context's embedding dropout exists (MDT: every embedded token; MDT-V without goal conditioning: the appended goal token) --
# shipped 0, so k_dropout_rows and embed_drop_from run nowhere else; goal_drop on one case for the Bernoulli replay; g16: the
# proprioceptive token
MODEL_CASES = [(n, {}) for n in G11] + [("mdt_tiny", dict(embed_pdrob=0.1)), ("mdtv_no_goal_cond", dict(embed_pdrob=0.1)),
                                        ("mdt_no_ada", dict(embed_pdrob=0.1)), ("mdtv_tiny", dict(goal_drop=0.2, embed_pdrob=0.1)),
                                        ("proprio_default", {})]


@pytest.mark.parametrize("name,overrides", MODEL_CASES, ids=[n + "".join(f"-{k}" for k in o) for n, o in MODEL_CASES])
def test_train_mode_step_matches_the_masked_float64_oracle(name, overrides):
    meta, cfg, state, goal, li = load_case(name, overrides=overrides)
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    keep = replayed_goal_keep(cfg, goal, 31)
    ref = oracle_loss_step(meta, cfg, state, goal, li, seeds[0], keep)
    check_step(hip, ref, name, at_least=30)
    # the masks matter: the eval-mode oracle's output is outside the tolerance the masked one's is held to
    with torch.no_grad():
        ev = O.loss(params_of(meta), cfg, state, li["actions"], goal, li["noise_train"], li["sigma"], arch=meta["arch"])[1]
    with pytest.raises(AssertionError):
        assert_close(hip[1], ev, what="eval-mode output")


_ORACLE_AT = {}


def oracle_at(B, seed_of):
    """mdtv_default at batch B: the masked oracle's step, computed once per (B, seed) (the split switches below replay it)."""
    meta, cfg, state, goal, li = load_case("mdtv_default", B=B)
    key = (B, seed_of)
    if key not in _ORACLE_AT:
        _ORACLE_AT.clear()
        _ORACLE_AT[key] = oracle_loss_step(meta, cfg, state, goal, li, seed_of)
    return _ORACLE_AT[key]


@pytest.mark.parametrize("B", [37, 256, 1024])
def test_train_mode_step_at_training_batches(B):
    """mdtv_default at B = 37, 256 and 1024 (the benchmark's step: side stream, two-half decoder blocks, bf16-split products,
    split-K weight gradients): forward and backward regenerate the restated masks on every element."""
    meta, cfg, state, goal, li = load_case("mdtv_default", B=B)
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=47)
    check_step(hip, oracle_at(B, seeds[0]), f"B={B}", at_least=100)


@pytest.mark.parametrize("switch", ["mdt_op_set_mlp_split", "mdt_op_set_ws_split", "mdt_op_set_tn_split"])
def test_train_mode_step_at_b1024_with_a_split_form_off(switch):
    from mdt_policy_amd import _lib
    B = 1024
    meta, cfg, state, goal, li = load_case("mdtv_default", B=B)
    setter = getattr(_lib.load(), switch)
    setter(0)
    try:
        model, seeds = facade(meta, cfg)
        hip = hip_loss_step(model, meta, state, goal, li, torch_seed=47)
    finally:
        setter(-1)
    check_step(hip, oracle_at(B, seeds[0]), f"B={B} {switch}(0)", at_least=100)


def _context_only(model, meta, cfg, state, goal, li, torch_seed):
    gstate = {k: (v.cuda().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    ggoal = goal.cuda().requires_grad_()
    torch.manual_seed(torch_seed)
    ctx = model.forward_context_only(gstate, li["actions"].cuda(), ggoal, li["sigma"].cuda())
    return gstate, ggoal, ctx


@pytest.mark.parametrize("name,overrides", [("mdtv_tiny", {}), ("mdtv_no_ada", {}), ("mdt_tiny", dict(embed_pdrob=0.1))])
def test_train_mode_context_only_forward_and_backward(name, overrides):
    """forward_context_only in train mode (mdt_train_encode_fwd / _bwd): context and every encoder-side gradient."""
    meta, cfg, state, goal, li = load_case(name, overrides=overrides)
    model, seeds = facade(meta, cfg)
    gstate, ggoal, ctx = _context_only(model, meta, cfg, state, goal, li, 5)
    w = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), 7))
    (ctx * w.cuda()).mean().backward()
    torch.cuda.synchronize()
    assert len(seeds) == 1
    P, st, g64 = oracle_leaves(meta, state, goal, "cpu")
    c64 = O.forward_context_only(P, cfg, st, g64, meta["arch"], sigma=li["sigma"].double(), masks=CachedMasks.of(seeds[0], cfg))
    (c64 * w.double()).mean().backward()
    assert_close(ctx.detach().cpu(), c64.detach(), what=name + " context")
    check_gradients(hip_grads(model, gstate, ggoal), grads_of(P, st, g64), name + " context only", at_least=10, zero_is_none=True)


@pytest.mark.parametrize("name", ["mdtv_tiny", "mdt_tiny"])
def test_train_mode_two_tapes_then_one_backward(name):
    """The agent's step: loss and forward_context_only alive at once, each with its own seed, then ONE backward."""
    meta, cfg, state, goal, li = load_case(name)
    model, seeds = facade(meta, cfg)
    gstate = {k: (v.cuda().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    ggoal = goal.cuda().requires_grad_()
    torch.manual_seed(9)
    loss, mo = model.loss(gstate, li["actions"].cuda(), ggoal, li["noise_train"].cuda(), li["sigma"].cuda())
    ctx = model.forward_context_only(gstate, li["actions"].cuda(), ggoal, li["sigma"].cuda())
    w = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), 7))
    (loss + (ctx * w.cuda()).mean()).backward()
    torch.cuda.synchronize()
    assert len(seeds) == 2 and seeds[0] != seeds[1]
    P, st, g64 = oracle_leaves(meta, state, goal, "cpu")
    l64, mo64 = O.loss(P, cfg, st, li["actions"].double(), g64, li["noise_train"].double(), li["sigma"].double(), arch=meta["arch"],
                       masks=CachedMasks.of(seeds[0], cfg))
    c64 = O.forward_context_only(P, cfg, st, g64, meta["arch"], sigma=li["sigma"].double(), masks=CachedMasks.of(seeds[1], cfg))
    (l64 + (c64 * w.double()).mean()).backward()
    assert abs(loss.item() - l64.item()) <= 1e-3 * abs(l64.item())
    assert_close(mo.detach().cpu(), mo64.detach(), what=name + " model_output")
    assert_close(ctx.detach().cpu(), c64.detach(), what=name + " second context")
    check_gradients(hip_grads(model, gstate, ggoal), grads_of(P, st, g64), name + " two tapes", at_least=30)


@pytest.mark.parametrize("name", ["mdtv_default", "mdt_tiny"])
def test_train_mode_staged_backward_equals_the_one_call_backward(name, monkeypatch):
    """The per-stage backward regenerates the masks the one-call backward regenerates: the same bits everywhere."""
    meta, cfg, state, goal, li = load_case(name, overrides=dict(embed_pdrob=0.1))
    res = {}
    for staged in ("0", "1"):
        monkeypatch.setenv("MDT_HIP_BWD_STAGES", staged)
        model, seeds = facade(meta, cfg)
        res[staged] = hip_loss_step(model, meta, state, goal, li, torch_seed=13) + (seeds[0],)
    a, b = res["0"], res["1"]
    assert a[4] == b[4] and a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert set(a[3]) == set(b[3])
    for k, g in a[3].items():
        assert (g is None and b[3][k] is None) or torch.equal(g, b[3][k]), f"{k}: staged and one-call gradients differ"
