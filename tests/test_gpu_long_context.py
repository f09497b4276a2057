"""Every configuration of tests/long_context_configs.py (contexts of 17 .. 64 tokens) on the MI355X (pytest -m gpu): sampling
against the reference's recording and against the float64 oracle across the dispatcher's batch regimes, graph replay, forward and
loss at per-sample sigmas, a training step's loss and every gradient (eval mode, and train mode against the replayed dropout
masks), denoise_grad with what the decoder can and cannot see of a context, and two resamplers of 16 latents feeding one call.

Tolerances are those the same checks have at contexts <= 16 tokens: the forward tolerance rtol 1e-3 / atol 1e-4 (tests/helpers.py,
test_gpu_parity.py), the loss to 1e-3 relative and every gradient to rtol 2e-3, atol 2e-3 * max |ref| + 1e-7 per tensor
(test_train_grads.py, test_gpu_train_dropout.py, test_gpu_denoise_grad.py)."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.family import Family
from tests.helpers import assert_close, load_fixture, params_of, to
from tests.long_context_configs import CTX_ENVELOPE, CTX_GOLDEN, CTX_SHAPES, CTX_SPEC

pytestmark = pytest.mark.gpu

NAMES = sorted(CTX_ENVELOPE)
SEEDS = dict(weight_seed=211, input_seed=212, loss_seed=213, ctx_seed=214, obs_seed=215)   # the recorder's
assert all(e["arch"] == "mdtv" for e in CTX_ENVELOPE.values())   # every state here is state_images
F = Family(CTX_SPEC, CTX_ENVELOPE, SEEDS)
meta_of, model_of, inputs, oracle_sample, hip_sample = F.meta_of, F.model_of, F.inputs, F.oracle_sample, F.hip_sample


@pytest.mark.parametrize("name", CTX_GOLDEN)
def test_sample_ddim_matches_the_reference_recording(name):
    """The recorded 3-step sample_ddim at B = 2, and the context it left."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    meta, fx = load_fixture(f"g21_ctx_{name}.npz")
    model, _ = model_of(name)
    state, goal, noise = inputs(name, meta["B"], meta["input_seed"])
    with torch.no_grad():
        got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), torch.from_numpy(fx["sigmas"])).cpu()
    assert_close(got, fx["actions"], what=f"{name} recorded actions")
    assert_close(model.inner_model.latent_encoder_emb.cpu(), fx["ctx"], what=f"{name} recorded context")


@pytest.mark.parametrize("name", NAMES)
def test_sample_ddim_at_b1_and_b8_and_graph_replay(name):
    """3-step sample_ddim against the float64 oracle at B = 8 and B = 1; at B = 1 four calls, the last two replayed as a HIP graph
    and bit-identical to the eager calls."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    model, _ = model_of(name)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    assert_close(hip_sample(name, 8, 48, sig), oracle_sample(name, 8, 48, sig), what=f"{name} B = 8")
    seeds = (7, 8)
    want = {s: oracle_sample(name, 1, s, sig) for s in seeds}
    outs = []
    for i in range(4):
        outs.append(hip_sample(name, 1, seeds[i % 2], sig))
        assert_close(outs[-1], want[seeds[i % 2]], what=f"{name} B = 1, call {i}")
    assert getattr(model, "_graphed_samplers", None), "the replay path was not taken"
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), f"{name}: the replayed call differs from the eager one"


@pytest.mark.parametrize("B", [16, 80])
def test_sample_ddim_where_the_encoder_and_the_decoder_take_different_launches(B):
    """ctx64_hd48 (Te = 64, Ta = 10): at B = 16 the encoder has 1024 rows -- the fp16 pair launches, from 768 rows on -- and the
    decoder 160, on the fp32 ones; at B = 80 both are past 768."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    name = "ctx64_hd48"
    Ta, Te, _ = CTX_SHAPES[name]
    assert B * Te >= 768 and (B * Ta >= 768) == (B == 80)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    assert_close(hip_sample(name, B, 40 + B, sig), oracle_sample(name, B, 40 + B, sig), what=f"{name} B = {B}")


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_loss_at_per_sample_sigmas(name):
    """B = 33: GCDenoiser.forward and .loss against the float64 oracle."""
    e = CTX_ENVELOPE[name]
    cfg, arch, B = e["cfg"], e["arch"], 33
    model, meta = model_of(name)
    state, goal, _ = inputs(name, B, 51)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 52).items()}
    assert len(set(li["sigma"].tolist())) > 16
    x = li["actions"] + li["noise_train"] * li["sigma"][:, None, None]
    P = params_of(meta, torch.float64)
    st64 = to(state, torch.Tensor.double)
    with torch.no_grad():
        den = model(to(state, torch.Tensor.cuda), x.cuda(), goal.cuda(), li["sigma"].cuda()).cpu()
        loss, mo = model.loss(to(state, torch.Tensor.cuda), li["actions"].cuda(), goal.cuda(), li["noise_train"].cuda(), li["sigma"].cuda())
        want_den = O.denoise(P, cfg, st64, x.double(), goal.double(), li["sigma"].double(), 0.5, arch)
        lo, want_mo = O.loss(P, cfg, st64, li["actions"].double(), goal.double(), li["noise_train"].double(), li["sigma"].double(), arch=arch)
    assert_close(den, want_den, what=f"{name} forward")
    assert_close(mo.cpu(), want_mo, what=f"{name} model_output")
    assert abs(loss.item() - lo.item()) <= 1e-3 * abs(lo.item()), f"{name}: loss {loss.item()} vs {lo.item()}"


def hip_step(model, state, goal, li):
    model.zero_grad(set_to_none=True)
    gstate = to(state, lambda v: v.cuda().requires_grad_())
    ggoal = goal.cuda().requires_grad_()
    loss, _ = model.loss(gstate, li["actions"].cuda(), ggoal, li["noise_train"].cuda(), li["sigma"].cuda())
    ctx = model.inner_model.latent_encoder_emb
    wctx = synthetic.normal("ctx_weight", tuple(ctx.shape), 63)
    (loss + 0.1 * (ctx * torch.from_numpy(wctx).cuda()).sum() / ctx.numel()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.inner_model.named_parameters() if p.grad is not None}
    grads.update({"d_" + k: v.grad.clone() for k, v in gstate.items() if torch.is_tensor(v)})
    grads["d_goal"] = ggoal.grad.clone()
    return loss, wctx, grads


@pytest.mark.parametrize("name", NAMES)
def test_training_step_gradients_and_their_repeatability(name):
    """One training step at B = 16 (eval mode: no dropout): the loss to 1e-3 relative, every parameter gradient and the input
    gradients against float64 autograd through the oracle, each to 2e-3 of its own largest value; a second run of the same step
    gives the same bits in every gradient (no atomics: every output element has one owner)."""
    e = CTX_ENVELOPE[name]
    cfg, arch, B = e["cfg"], e["arch"], 16
    model, meta = model_of(name)
    state, goal, _ = inputs(name, B, 61)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 62).items()}
    loss, wctx, got = hip_step(model, state, goal, li)
    loss2, _, again = hip_step(model, state, goal, li)
    assert loss.item() == loss2.item() and set(got) == set(again)
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{name} {k}: two runs differ in bits"

    P = {k: v.requires_grad_(v.dtype.is_floating_point) for k, v in params_of(meta, torch.float64).items()}
    st64 = to(state, lambda v: v.double().requires_grad_())
    g64 = goal.double().requires_grad_()
    lo, _ = O.loss(P, cfg, st64, li["actions"].double(), g64, li["noise_train"].double(), li["sigma"].double(), arch=arch)
    c = O.encode(P, cfg, st64, g64, arch, "forward", sigma=li["sigma"].double())
    (lo + 0.1 * (c * torch.from_numpy(wctx).double()).sum() / c.numel()).backward()
    assert abs(loss.item() - lo.item()) <= 1e-3 * abs(lo.item()), f"{name}: loss {loss.item()} vs {lo.item()}"
    n = 0
    for k, p in model.inner_model.named_parameters():
        if not p.requires_grad:  # the rotary frequency buffers
            continue
        ref = P["inner_model." + k].grad
        if ref is None:
            assert k not in got, k
            continue
        assert_close(got[k].cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what=f"{name} {k}")
        n += 1
    assert n > 20
    for k, v in st64.items():
        if torch.is_tensor(v):
            assert_close(got["d_" + k].cpu(), v.grad, rtol=2e-3, atol=2e-3 * float(v.grad.abs().max()) + 1e-9, what=f"{name} d_{k}")
    assert_close(got["d_goal"].cpu(), g64.grad, rtol=2e-3, atol=2e-3 * float(g64.grad.abs().max()) + 1e-9, what=f"{name} d_goal")


@pytest.mark.parametrize("name,embed_p", [("ctx17_hd48", 0.1), ("ctx33_rope_hd64", 0), ("ctx40_ta48", 0)])
def test_train_mode_step_matches_the_masked_float64_oracle(name, embed_p):
    """Train mode at the shipped dropout probabilities against the oracle that replays the library's masks
    (tests/dropout_masks.py; the cross-attention's site is (B, H, Ta, Te)), as tests/test_gpu_train_dropout.py does at contexts
    <= 16 tokens, with its checks; ctx17_hd48 also with the embedding dropout (17 context rows per sample) the shipped
    configurations leave at 0."""
    from tests.test_gpu_train_dropout import check_step, facade, hip_loss_step, oracle_loss_step
    cfg, B = dict(CTX_ENVELOPE[name]["cfg"], embed_pdrob=embed_p), 4
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    meta = meta_of(name)
    state, goal, _ = inputs(name, B, 71)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 72).items()}
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    ref = oracle_loss_step(meta, cfg, state, goal, li, seeds[0], None)
    check_step(hip, ref, name, at_least=30)


def test_train_mode_staged_backward_equals_the_one_call_backward(monkeypatch):
    """ctx17_hd48 with every dropout on: the per-stage backward regenerates the masks the one-call backward regenerates -- the same
    bits everywhere (tests/test_gpu_train_dropout.py's check at <= 16 tokens)."""
    from tests.test_gpu_train_dropout import facade, hip_loss_step
    name, B = "ctx17_hd48", 4
    cfg, meta = dict(CTX_ENVELOPE[name]["cfg"], embed_pdrob=0.1), meta_of(name)
    state, goal, _ = inputs(name, B, 73)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 74).items()}
    res = {}
    for staged in ("0", "1"):
        monkeypatch.setenv("MDT_HIP_BWD_STAGES", staged)
        model, seeds = facade(meta, cfg)
        res[staged] = hip_loss_step(model, meta, state, goal, li, torch_seed=13) + (seeds[0],)
    a, b = res["0"], res["1"]
    assert a[4] == b[4] and a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert set(a[3]) == set(b[3]) and len(a[3]) > 30
    for k, g in a[3].items():
        assert (g is None and b[3][k] is None) or torch.equal(g, b[3][k]), f"{k}: staged and one-call gradients differ"


def test_ten_fused_adamw_steps_lower_the_loss_at_40_tokens():
    """FusedAdamW on ctx40_no_goal at B = 8: the library writes the parameters in place and the next forward reads them -- the loss
    falls as tests/test_gpu_optim.py asks of the tiny model."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.optim import FusedAdamW
    name, B = "ctx40_no_goal", 8
    cfg = CTX_ENVELOPE[name]["cfg"]
    torch.manual_seed(0)
    model = GCDenoiser(cfg, 0.5).cuda().eval()
    state, goal, _ = inputs(name, B, 75)
    state, goal = to(state, torch.Tensor.cuda), goal.cuda()
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, 76).items()}
    opt = FusedAdamW(model.parameters(), lr=2e-3, weight_decay=0.05)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss, _ = model.loss(state, li["actions"], goal, li["noise_train"], li["sigma"])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.8 * losses[0], losses


def test_denoise_grad_at_31_tokens():
    """GCDenoiser.denoise_grad on ctx31_h3_d144 at B = 3: L = (D . w).sum() -- the value, then the gradient of every parameter and
    input, with tests/test_gpu_denoise_grad.py's checks."""
    from tests.test_gpu_denoise_grad import all_grads, check_grads, leaves, oracle_run, upstream
    name, B = "ctx31_h3_d144", 3
    cfg = CTX_ENVELOPE[name]["cfg"]
    model, meta = model_of(name)
    state, goal, _ = inputs(name, B, 81)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 82).items()}
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    w = upstream(x.shape)
    model.zero_grad(set_to_none=True)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    vals = {}

    def objective(denoise, x64, s64, dev):
        vals["den"] = denoise(x64, s64)
        return (vals["den"] * w.double().to(dev)).sum()

    _, ref = oracle_run(meta, cfg, state, goal, li, objective)
    assert_close(den.detach().cpu(), vals["den"].detach().cpu(), rtol=1e-3, atol=1e-4, what=name + " denoised")
    got = all_grads(model, gstate, ggoal, x, sigma)
    check_grads(got, ref, name, at_least=30)
    model.zero_grad(set_to_none=True)


@pytest.mark.parametrize("name", ["ctx17_hd48", "ctx40_no_goal", "ctx64_rope_hd32"])
def test_the_decoder_sees_the_first_ta_rows_of_a_given_context(name):
    """denoise_grad(None, x, None, sigma, context=ctx) at B = 3 with an objective on the denoised chunk alone: rows >= Tv =
    min(Ta, Te) of d_ctx are exactly zero (the causal mask of the Ta x Te cross-attention is top-left aligned: no query sees
    them), rows < Tv are not; a context whose rows >= Ta differ wildly gives the same bits in the chunk and in every gradient."""
    from tests.test_gpu_denoise_grad import leaves, upstream
    B = 3
    Ta, Te, _ = CTX_SHAPES[name]
    Tv = min(Ta, Te)
    cfg = CTX_ENVELOPE[name]["cfg"]
    model, _ = model_of(name)
    state, goal, _ = inputs(name, B, 91)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 92).items()}
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    w = upstream(x.shape).cuda()
    with torch.no_grad():
        ctx = model.forward_context_only(gstate, None, ggoal, sigma.detach())
    assert tuple(ctx.shape) == (B, Te, cfg["embed_dim"])
    other = ctx.clone()
    other[:, Ta:] = 1e3 * torch.from_numpy(synthetic.normal("ctx_noise", (B, Te - Ta, cfg["embed_dim"]), 93)).cuda()
    runs = []
    for c in (ctx, other):
        model.zero_grad(set_to_none=True)
        c = c.clone().requires_grad_()
        xx = x.detach().clone().requires_grad_()
        den = model.denoise_grad(None, xx, None, sigma.detach(), context=c)
        (den * w).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in model.inner_model.named_parameters() if p.grad is not None}
        runs.append(dict(den=den.detach().clone(), d_x=xx.grad.clone(), d_ctx=c.grad.clone(), **grads))
    model.zero_grad(set_to_none=True)
    a, b = runs
    assert bool((a["d_ctx"][:, Tv:] == 0).all()), f"{name}: d_ctx rows >= {Tv} are not zero"
    assert bool((a["d_ctx"][:, :Tv].abs().amax(dim=(0, 2)) > 0).all()), f"{name}: a visible row of d_ctx is zero"
    assert set(a) == set(b) and len(a) > 20
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{name} {k}: context rows >= Ta reached the result"


def test_two_resamplers_of_16_latents_feed_one_sampler_call():
    """Two cameras x PerceiverResampler(num_latents=16) -> state_images (B, 32, 384) -> ctx34_proprio_mlp_head's sample_ddim at
    B = 3, against the float64 oracles of both (oracle/perceiver_oracle.py, oracle/mdt_oracle.py)."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    from oracle import perceiver_oracle as PO
    from tests.helpers import envelope_params
    name, B, heads = "ctx34_proprio_mlp_head", 3, 2
    model, _ = model_of(name)
    kw = dict(dim=384, depth=1, dim_head=64, heads=heads, num_latents=16, num_time_embeds=1, ff_mult=1)
    latents, latents64 = [], []
    for cam in range(2):
        r = PerceiverResampler(**kw)
        P = envelope_params([(k, tuple(v.shape)) for k, v in r.state_dict().items()], 221 + cam)
        r.load_state_dict(P, strict=True)
        media = torch.from_numpy(synthetic.normal("media", (B, 1, 20, 384), 223 + cam))
        with torch.no_grad():
            latents.append(r.cuda().eval()(media.cuda(), None).reshape(B, 16, 384))
        latents64.append(PO.perceiver_resampler({k: v.double() for k, v in P.items()}, media.double(), heads, None).reshape(B, 16, 384))
    state, goal, noise = inputs(name, B, 95)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    gstate = dict(to(state, torch.Tensor.cuda), state_images=torch.cat(latents, 1))
    with torch.no_grad():
        got = gs.sample_ddim(model, gstate, noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
    assert tuple(model.inner_model.latent_encoder_emb.shape) == (B, 34, 384)
    st64 = dict(to(state, torch.Tensor.double), state_images=torch.cat(latents64, 1))
    assert_close(torch.cat(latents, 1).cpu(), st64["state_images"], what="resampler latents")
    assert_close(got, oracle_sample(name, B, 95, sig, state=st64), what="two resamplers into sample_ddim")
