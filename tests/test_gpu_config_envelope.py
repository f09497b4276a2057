"""Every configuration of tests/envelope_configs.py (the edges of what mdt_create accepts) on the MI355X (pytest -m gpu):
sampling across the dispatcher's batch and row thresholds, one native sampler call, and a training step's loss and
gradients -- each against float64 through the oracle."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.envelope_configs import ENVELOPE
from tests.family import Family
from tests.helpers import assert_close, to

pytestmark = pytest.mark.gpu

NAMES = sorted(ENVELOPE)
F = Family(None, ENVELOPE)   # (model, float32 state dict): 'rich' synthetic weights
model_of, inputs = F.model_of, F.inputs
oracle_sample = lambda name, sampler, B, seed, sig: F.oracle_sample(name, B, seed, sig, sampler)  # noqa: E731


def batches(cfg):
    """B = 1; up to 32 samples (ATTN_PROJ_MAX_BATCH); 33..63; >= 64 (k_attn's head split); >= 768 decoder rows (split forms)
    and >= 1401 rows (wide attention prologue, fused MLP).  With one action row per sample the row thresholds need more
    samples; that model (d = 64) keeps the oracle cheap at any of them."""
    ta = cfg["action_seq_len"]
    if ta == 1:
        return [1, 24, 48, 80, 800, 1500]
    if ta == 16:
        return [1, 20, 40, 70, 96]  # rows 16 / 320 / 640 / 1120 / 1536
    return [1, 24, 48, 80, 150]  # Ta = 10: rows 10 / 240 / 480 / 800 / 1500


@pytest.mark.parametrize("name", NAMES)
def test_sample_ddim_across_the_batch_thresholds(name):
    """3-step sample_ddim against the float64 oracle at every batch of batches(); at B = 1 four calls, the last two
    replayed as a HIP graph."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    model, _ = model_of(name)
    cfg = ENVELOPE[name]["cfg"]
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    for B in batches(cfg):
        state, goal, noise = inputs(name, B, 40 + B)
        want = oracle_sample(name, O.sample_ddim, B, 40 + B, sig)
        with torch.no_grad():
            got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
        assert_close(got, want, what=f"{name} B = {B}")
    # rollout calls: the third and fourth call with the same shapes replay a captured graph
    seeds = (7, 8)
    want = {s: oracle_sample(name, O.sample_ddim, 1, s, sig) for s in seeds}
    with torch.no_grad():
        for i in range(4):
            state, goal, noise = inputs(name, 1, seeds[i % 2])
            got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
            assert_close(got, want[seeds[i % 2]], what=f"{name} B = 1, call {i}")
    assert getattr(model, "_graphed_samplers", None), "the replay path was not taken"


@pytest.mark.parametrize("name", NAMES)
def test_native_euler_sampler(name, monkeypatch):
    """One native sampler call (sample_euler -> mdt_sample, the per-step denoiser disabled) at B = 1 and B = 40."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model, _ = model_of(name)

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    monkeypatch.setattr(GCDenoiser, "forward", boom)
    sig = gs.get_sigmas_exponential(4, 0.01, 80.0)
    for B in (1, 40):
        state, goal, noise = inputs(name, B, 90 + B)
        want = oracle_sample(name, O.sample_euler, B, 90 + B, sig)
        with torch.no_grad():
            got = gs.sample_euler(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
        assert_close(got, want, what=f"{name} euler B = {B}")


@pytest.mark.parametrize("name", NAMES)
def test_training_step_gradients(name):
    """One training step at B = 12 (eval mode: no dropout): the loss, every parameter gradient and the input gradients
    against float64 autograd through the oracle, each gradient to 2e-3 of its own largest value."""
    e = ENVELOPE[name]
    cfg, arch = e["cfg"], e["arch"]
    model, P32 = model_of(name)
    B = 12
    state, goal, _ = inputs(name, B, 61)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 62).items()}
    model.zero_grad(set_to_none=True)
    gstate = to(state, lambda v: v.cuda().requires_grad_())
    ggoal = goal.cuda().requires_grad_()
    loss, _ = model.loss(gstate, li["actions"].cuda(), ggoal, li["noise_train"].cuda(), li["sigma"].cuda())
    ctx = model.inner_model.latent_encoder_emb
    wctx = synthetic.normal("ctx_weight", tuple(ctx.shape), 63)
    (loss + 0.1 * (ctx * torch.from_numpy(wctx).cuda()).sum() / ctx.numel()).backward()
    torch.cuda.synchronize()

    P = {k: v.double().requires_grad_(v.dtype.is_floating_point) for k, v in P32.items()}
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
            assert p.grad is None, k
            continue
        scale = float(ref.abs().max())
        assert_close(p.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * scale + 1e-7, what=f"{name} {k}")
        n += 1
    assert n > 20
    for k, v in gstate.items():
        if torch.is_tensor(v):
            ref = st64[k].grad
            assert_close(v.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-9, what=f"{name} d_{k}")
    assert_close(ggoal.grad.cpu(), g64.grad, rtol=2e-3, atol=2e-3 * float(g64.grad.abs().max()) + 1e-9, what=f"{name} d_goal")
