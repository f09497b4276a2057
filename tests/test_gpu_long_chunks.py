"""Every configuration of tests/long_chunk_configs.py (action chunks of 17 .. 64 steps) on the MI355X (pytest -m gpu), as
tests/test_gpu_config_envelope.py runs the 16-step envelope: sampling across the dispatcher's batch and row thresholds, one
native sampler call, and a training step's loss and gradients -- each against float64 through the oracle."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.family import Family
from tests.helpers import assert_close, to
from tests.long_chunk_configs import LONG_ENVELOPE

pytestmark = pytest.mark.gpu

NAMES = sorted(LONG_ENVELOPE)
F = Family(None, LONG_ENVELOPE)   # (model, float32 state dict): 'rich' synthetic weights
model_of, inputs = F.model_of, F.inputs
oracle_sample = lambda name, sampler, B, seed, sig: F.oracle_sample(name, B, seed, sig, sampler)  # noqa: E731


def batches(cfg):
    """B = 1; the smallest batches that reach 200, 768 and 1401 decoder rows (one workgroup per sample from 200 rows on where it
    applies, the split forms, the fused MLP launch) as long as they stay below 64 samples; one batch of at most 32 samples and one
    of 33 .. 63 in any case.  The d = 128 model also runs 70 samples (the oracle stays cheap there)."""
    ta = cfg["action_seq_len"]
    bs = {1} | {b for b in (-(-rows // ta) for rows in (200, 768, 1401)) if b <= 63}
    if not any(2 <= b <= 32 for b in bs):
        bs.add(20)
    if not any(33 <= b <= 63 for b in bs):
        bs.add(40)
    if cfg["embed_dim"] == 128:
        bs.add(70)
    return sorted(bs)


def test_the_batches_reach_every_dispatcher_regime():
    """Over the ten cases: B = 1, a batch of at most 32 and one of 33 .. 63 everywhere; 200 and 768 rows everywhere; 1401 rows
    wherever 63 samples reach them; 64 samples or more on the d = 128 model only."""
    for name in NAMES:
        cfg = LONG_ENVELOPE[name]["cfg"]
        bs, ta = batches(cfg), cfg["action_seq_len"]
        assert bs[0] == 1 and any(2 <= b <= 32 for b in bs) and any(33 <= b <= 63 for b in bs), (name, bs)
        assert any(b * ta >= 200 for b in bs) and any(b * ta >= 768 for b in bs), (name, bs)
        assert any(b * ta >= 1401 for b in bs) == (63 * ta >= 1401 or cfg["embed_dim"] == 128), (name, bs)
        assert (max(bs) >= 64) == (cfg["embed_dim"] == 128), (name, bs)


@pytest.mark.parametrize("name", NAMES)
def test_sample_ddim_across_the_batch_thresholds(name):
    """3-step sample_ddim against the float64 oracle at every batch of batches(); at B = 1 four calls, the last two
    replayed as a HIP graph."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    model, _ = model_of(name)
    cfg = LONG_ENVELOPE[name]["cfg"]
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
    """One native sampler call (sample_euler -> mdt_sample, the per-step denoiser disabled) at B = 3."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model, _ = model_of(name)

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    monkeypatch.setattr(GCDenoiser, "forward", boom)
    sig = gs.get_sigmas_exponential(4, 0.01, 80.0)
    B = 3
    state, goal, noise = inputs(name, B, 90 + B)
    want = oracle_sample(name, O.sample_euler, B, 90 + B, sig)
    with torch.no_grad():
        got = gs.sample_euler(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
    assert_close(got, want, what=f"{name} euler B = {B}")


def test_the_shipped_model_at_50_steps_samples_scores_steers_and_trains(monkeypatch):
    """GCDenoiser(configs.mdtv_default(action_seq_len=50), 0.5) -- the horizon real-time chunking is usually run at -- through
    its four uses at B = 2: 3-step sample_ddim against the float64 oracle; the native log-likelihood of the sampled chunks; a
    native steered sample_ddim that lowers the weighted error toward its known actions; one training step with finite gradients
    on every parameter that has one."""
    from mdt_policy_amd import configs
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.utils.action_steer import ActionSteer
    cfg, B = configs.mdtv_default(action_seq_len=50), 2
    model = GCDenoiser(cfg, 0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, 5, "rich").items()}
    model.load_state_dict(P, strict=False)
    model = model.cuda().eval()
    t = {k: torch.from_numpy(v) for k, v in synthetic.sampler_inputs(B, cfg, 77, "mdtv").items()}
    state, goal, x = {"state_images": t["state_images"], "modality": "lang"}, t["goal"], t["noise"] * 80.0
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    want = O.sample_ddim(O.to_dtype(P, torch.float64), cfg, to(state, torch.Tensor.double), x.double(), goal.double(), sig, arch="mdtv",
                         hoist=True)
    gstate = to(state, torch.Tensor.cuda)
    with monkeypatch.context() as mp:
        mp.setattr(GCDenoiser, "forward", lambda *a, **k: pytest.fail("the per-step denoiser ran: the native path was not taken"))
        with torch.no_grad():
            got = gs.sample_ddim(model, gstate, x.cuda(), goal.cuda(), sig)
            steer = ActionSteer(-got, torch.ones(B, 50, 1, device="cuda") * 0.5, 5.0)
            steered = gs.sample_ddim(model, gstate, x.cuda(), goal.cuda(), sig, extra_args={"steer": steer})
    assert_close(got.cpu(), want, what="Ta = 50 sample_ddim")
    werr = lambda out: float((0.5 * (-got - out) ** 2).sum())
    assert werr(steered) < werr(got), "the steer did not pull the chunk toward its known actions"
    ll, info = gs.log_likelihood(model, gstate, got, goal.cuda(), 0.001, 80.0)
    assert ll.shape == (B,) and bool(torch.isfinite(ll).all()) and info["fevals"] > 0
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, 78).items()}
    model.zero_grad(set_to_none=True)
    loss, _ = model.loss(gstate, li["actions"], goal.cuda(), li["noise_train"], li["sigma"])
    loss.backward()
    lo, _ = O.loss(O.to_dtype(P, torch.float64), cfg, to(state, torch.Tensor.double), li["actions"].cpu().double(), goal.double(),
                   li["noise_train"].cpu().double(), li["sigma"].cpu().double(), arch="mdtv")
    assert abs(loss.item() - lo.item()) <= 1e-3 * abs(lo.item())
    grads = [p.grad for p in model.inner_model.parameters() if p.grad is not None]
    assert len(grads) > 20 and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)


@pytest.mark.parametrize("name", NAMES)
def test_training_step_gradients(name):
    """One training step at B = 5 (eval mode: no dropout): the loss to 1e-3 relative, every parameter gradient and the input
    gradients against float64 autograd through the oracle, each gradient to 2e-3 of its own largest value."""
    e = LONG_ENVELOPE[name]
    cfg, arch = e["cfg"], e["arch"]
    model, P32 = model_of(name)
    B = 5
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
