"""Every configuration of tests/wide_action_configs.py (action vectors of 17 .. 64 elements) on the MI355X (pytest -m gpu):
sampling against the reference's recording and against the float64 oracle across the dispatcher's batch regimes, forward and
loss at per-sample sigmas, a training step's loss and every gradient (eval mode, and train mode against the replayed dropout
masks), denoise_grad, run-to-run bit repeatability of the gradients and graph replay.

Tolerances are those the same checks have at action_dim <= 16: the forward tolerance rtol 1e-3 / atol 1e-4 (tests/helpers.py,
test_gpu_parity.py), the loss to 1e-3 relative and every gradient to rtol 2e-3, atol 2e-3 * max |ref| + 1e-7 per tensor
(test_train_grads.py, test_gpu_train_dropout.py, test_gpu_denoise_grad.py)."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.family import Family
from tests.helpers import assert_close, load_fixture, params_of, to
from tests.wide_action_configs import WIDE_ENVELOPE, WIDE_GOLDEN, WIDE_SPEC

pytestmark = pytest.mark.gpu

NAMES = sorted(WIDE_ENVELOPE)
SEEDS = dict(weight_seed=201, input_seed=202, loss_seed=203, ctx_seed=204, obs_seed=205)   # the recorder's
# state_obs at the recorder's input_seed is drawn at its obs_seed, so that seed gives the recorded inputs
F = Family(WIDE_SPEC, WIDE_ENVELOPE, SEEDS, recorded_obs=True)
meta_of, model_of, inputs, oracle_sample = F.meta_of, F.model_of, F.inputs, F.oracle_sample


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_sample_ddim_matches_the_reference_recording(name):
    """The recorded 10-step sample_ddim at B = 2."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    meta, fx = load_fixture(f"g20_wide_{name}.npz")
    model, _ = model_of(name)
    state, goal, noise = inputs(name, meta["B"], meta["input_seed"])
    with torch.no_grad():
        got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), torch.from_numpy(fx["sigmas"])).cpu()
    assert_close(got, fx["actions"], what=f"{name} recorded actions")


@pytest.mark.parametrize("name", NAMES)
def test_sample_ddim_across_the_batch_regimes_and_graph_replay(name):
    """3-step sample_ddim against the float64 oracle at B = 1, 8 and 80 (80 x Ta rows: past 768, where the fp16 pair split
    launches are on); at B = 1 four calls, the last two replayed as a HIP graph and bit-identical to the eager calls."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    model, _ = model_of(name)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    for B in (8, 80):
        assert B != 80 or B * WIDE_ENVELOPE[name]["cfg"]["action_seq_len"] >= 768
        state, goal, noise = inputs(name, B, 40 + B)
        want = oracle_sample(name, B, 40 + B, sig)
        with torch.no_grad():
            got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu()
        assert_close(got, want, what=f"{name} B = {B}")
    seeds = (7, 8)
    want = {s: oracle_sample(name, 1, s, sig) for s in seeds}
    outs = []
    with torch.no_grad():
        for i in range(4):
            state, goal, noise = inputs(name, 1, seeds[i % 2])
            outs.append(gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), sig.cuda()).cpu())
            assert_close(outs[-1], want[seeds[i % 2]], what=f"{name} B = 1, call {i}")
    assert getattr(model, "_graphed_samplers", None), "the replay path was not taken"
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]), f"{name}: the replayed call differs from the eager one"


@pytest.mark.parametrize("name", NAMES)
def test_forward_and_loss_at_per_sample_sigmas(name):
    """B = 33 (three 16-row tiles' worth of samples and one more): GCDenoiser.forward and .loss against the float64 oracle."""
    e = WIDE_ENVELOPE[name]
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


def hip_step(model, name, state, goal, li):
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
    e = WIDE_ENVELOPE[name]
    cfg, arch, B = e["cfg"], e["arch"], 16
    model, meta = model_of(name)
    state, goal, _ = inputs(name, B, 61)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 62).items()}
    loss, wctx, got = hip_step(model, name, state, goal, li)
    loss2, _, again = hip_step(model, name, state, goal, li)
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
    assert n > 20 and "action_emb.weight" in got and any(k.startswith("action_pred") for k in got)
    for k, v in st64.items():
        if torch.is_tensor(v):
            assert_close(got["d_" + k].cpu(), v.grad, rtol=2e-3, atol=2e-3 * float(v.grad.abs().max()) + 1e-9, what=f"{name} d_{k}")
    assert_close(got["d_goal"].cpu(), g64.grad, rtol=2e-3, atol=2e-3 * float(g64.grad.abs().max()) + 1e-9, what=f"{name} d_goal")


@pytest.mark.parametrize("name", ["a17", "a64"])
def test_train_mode_step_matches_the_masked_float64_oracle(name):
    """Train mode at the shipped dropout probabilities against the oracle that replays the library's masks
    (tests/dropout_masks.py), as tests/test_gpu_train_dropout.py does at action_dim <= 16, with its checks."""
    from tests.test_gpu_train_dropout import check_step, facade, hip_loss_step, oracle_loss_step
    cfg, B = WIDE_ENVELOPE[name]["cfg"], 4
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    meta = meta_of(name)
    state, goal, _ = inputs(name, B, 71)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 72).items()}
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    ref = oracle_loss_step(meta, cfg, state, goal, li, seeds[0], None)
    check_step(hip, ref, name, at_least=30)


def test_denoise_grad_at_33_elements():
    """GCDenoiser.denoise_grad on a33_h3_d144 at B = 3: L = (D . w).sum() -- the value, then the gradients of the noisy actions,
    sigma, action_emb / action_pred and every other parameter and input, with tests/test_gpu_denoise_grad.py's checks."""
    from tests.test_gpu_denoise_grad import all_grads, check_grads, leaves, oracle_run, upstream
    name, B = "a33_h3_d144", 3
    cfg = WIDE_ENVELOPE[name]["cfg"]
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
    assert got["d_x"].shape == (B, cfg["action_seq_len"], 33) and got["d_sigma"].shape == (B,)
    for k in ("inner_model.action_emb.weight", "inner_model.action_pred.weight"):
        assert got[k] is not None and ref[k] is not None
    check_grads(got, ref, name, at_least=30)
