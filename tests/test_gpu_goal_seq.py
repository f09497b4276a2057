"""Every configuration of tests/goal_seq_configs.py (goals of G = goal_seq_len > 1 tokens) on the MI355X (pytest -m gpu): sampling
against the reference's recordings and against the float64 oracle across the dispatcher's batch regimes, graph replay, forward
and loss at per-sample sigmas, a training step's loss and every gradient (eval mode, train mode against the replayed dropout
masks, and at row counts where the goal embedder's B * G rows reach the tall GEMM body), a cross-check of the goal rows against
state rows that needs no oracle, and the contrastive head pooling the longer context.

Tolerances are those the same checks have at one goal token: the forward tolerance rtol 1e-3 / atol 1e-4 (tests/helpers.py), the
loss to 1e-3 relative and every gradient to rtol 2e-3, atol 2e-3 * max |ref| + 1e-7 per tensor (test_gpu_train_dropout.py)."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import configs, synthetic
from oracle import mdt_oracle as O
from tests.family import Family
from tests.goal_seq_configs import GOAL_ENVELOPE, GOAL_GOLDEN, GOAL_SPEC, GOAL_TE, goal_rows
from tests.helpers import assert_close, envelope_params, load_fixture, params_of, to

pytestmark = pytest.mark.gpu

NAMES = sorted(GOAL_ENVELOPE)
SEEDS = dict(weight_seed=231, input_seed=232, loss_seed=233, ctx_seed=234, obs_seed=235)   # the recorder's


class GoalFamily(Family):
    def inputs(self, name, B, seed, dtype=torch.float32, cfg=None):
        """(state, goal (B, G, goal_dim), noise) on the host; state_obs (B, 1, proprio_dim) when the case switches the token on."""
        cfg = cfg or GOAL_ENVELOPE[name]["cfg"]
        state, goal, noise = super().inputs(name, B, seed, dtype, cfg)
        assert tuple(goal.shape) == (B, cfg["goal_seq_len"], cfg["goal_dim"])
        return state, goal, noise

    def hip_sample(self, name, B, seed, sig):
        out = super().hip_sample(name, B, seed, sig)
        ctx = self.model_of(name)[0].inner_model.latent_encoder_emb
        assert tuple(ctx.shape) == (B, GOAL_TE[name], GOAL_ENVELOPE[name]["cfg"]["embed_dim"])
        return out


F = GoalFamily(GOAL_SPEC, GOAL_ENVELOPE, SEEDS)
meta_of, model_of, inputs, oracle_sample, hip_sample = F.meta_of, F.model_of, F.inputs, F.oracle_sample, F.hip_sample


# ------------------------------------------------------------------------------------------------------------ 1. recordings
@pytest.mark.parametrize("name", GOAL_GOLDEN)
def test_sample_ddim_matches_the_reference_recording(name):
    """The recorded 3-step sample_ddim at B = 2, and the context it left."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    meta, fx = load_fixture(f"g23_goalseq_{name}.npz")
    model, _ = model_of(name)
    state, goal, noise = inputs(name, meta["B"], meta["input_seed"])
    with torch.no_grad():
        got = gs.sample_ddim(model, to(state, torch.Tensor.cuda), noise.cuda() * 80.0, goal.cuda(), torch.from_numpy(fx["sigmas"])).cpu()
    assert_close(got, fx["actions"], what=f"{name} recorded actions")
    assert_close(model.inner_model.latent_encoder_emb.cpu(), fx["ctx"], what=f"{name} recorded context")


# ------------------------------------------------------------------------------------------------------------ 2. sampling
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
    """g32_top (Te = 64, Ta = 10): at B = 16 the encoder has 1024 rows -- the fp16 pair launches, from 768 rows on -- and the
    decoder 160, on the fp32 ones; at B = 80 both are past 768.  The goal embedder runs 512 / 2560 rows."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    name = "g32_top"
    Te, Ta = GOAL_TE[name], GOAL_ENVELOPE[name]["cfg"]["action_seq_len"]
    assert B * Te >= 768 and (B * Ta >= 768) == (B == 80)
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    assert_close(hip_sample(name, B, 40 + B, sig), oracle_sample(name, B, 40 + B, sig), what=f"{name} B = {B}")


# ------------------------------------------------------------------------------------------------------------ 3. forward, loss
@pytest.mark.parametrize("name", NAMES)
def test_forward_and_loss_at_per_sample_sigmas(name):
    """B = 33: GCDenoiser.forward and .loss against the float64 oracle."""
    e = GOAL_ENVELOPE[name]
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


# ------------------------------------------------------------------------------------------------------------ 4. training step
def oracle_step(meta, cfg, state, goal, li, seed=None):
    """loss + 0.1 <ctx, w> / numel through the float64 oracle (masks of ``seed`` when given) -> (loss, model_output, ctx, gradients)."""
    from tests.test_gpu_train_dropout import CachedMasks, grads_of, on_device, oracle_leaves

    def run(dev):
        P, st, g64 = oracle_leaves(meta, state, goal, dev)
        l = {k: v.double().to(dev) for k, v in li.items()}
        masks = None if seed is None else CachedMasks.of(seed, cfg)
        lo, mo = O.loss(P, cfg, st, l["actions"], g64, l["noise_train"], l["sigma"], arch=meta["arch"], masks=masks)
        ctx = O.encode(P, cfg, st, g64, meta["arch"], "forward", sigma=l["sigma"], masks=masks)
        w = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), meta["ctx_seed"])).double().to(dev)
        (lo + 0.1 * (ctx * w).sum() / ctx.numel()).backward()
        return lo.item(), mo.detach().cpu(), ctx.detach().cpu(), grads_of(P, st, g64)
    return on_device(run)


def check_goal_gradients(name, cfg, hip, B):
    """d_goal is (B, G, goal_dim) with every row filled; MDT with position rows: pos_emb rows 0 .. G carry the goal and state rows'
    column sums, the action rows (never read) stay zero."""
    G = cfg["goal_seq_len"]
    d_goal = hip[3]["d_goal"]
    assert tuple(d_goal.shape) == (B, G, cfg["goal_dim"])
    assert bool((d_goal.abs().amax(dim=(0, 2)) > 0).all()), f"{name}: a goal row without a gradient"
    if GOAL_ENVELOPE[name]["arch"] == "mdt" and cfg["use_abs_pos_emb"]:
        g_pos = hip[3]["inner_model.pos_emb"][0]
        assert bool((g_pos[:G + 1].abs().amax(dim=1) > 0).all()) and not g_pos[G + 1:].any(), f"{name}: pos_emb rows"


@pytest.mark.parametrize("name", NAMES)
def test_eval_mode_training_step_against_float64_autograd(name):
    """B = 4, no dropout: the loss, the model output, the context and every gradient -- d_goal (B, G, goal_dim), the goal embedder,
    MDT's pos_emb rows 0 .. G among them."""
    from tests.test_gpu_train_dropout import check_step, hip_loss_step
    cfg, B = GOAL_ENVELOPE[name]["cfg"], 4
    model, meta = model_of(name)
    state, goal, _ = inputs(name, B, 61)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 62).items()}
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=1)
    check_step(hip, oracle_step(meta, cfg, state, goal, li), name, at_least=30)
    check_goal_gradients(name, cfg, hip, B)
    model.zero_grad(set_to_none=True)


# embed_pdrob: the shipped 0 everywhere but on the two MDT cases (MDT drops every embedded goal and state row, G + 2 of them).
# g3_no_goal_cond runs at embed_pdrob = 0 too: the oracle's replay of MDT-V's embedding dropout, which falls on the goal rows
# appended behind the state tokens, is written for one goal row (oracle/mdt_oracle.py, encode).
TRAIN_CASES = [(n, 0.0) for n in NAMES] + [("mdt_g3_pos", 0.1), ("mdt_g5_plain", 0.1)]


@pytest.mark.parametrize("name,embed_p", TRAIN_CASES, ids=[f"{n}-embed{p}" for n, p in TRAIN_CASES])
def test_train_mode_step_matches_the_masked_float64_oracle(name, embed_p):
    """Train mode at the shipped dropout probabilities, B = 33, against the oracle that replays the library's masks
    (tests/dropout_masks.py), with tests/test_gpu_train_dropout.py's checks."""
    from tests.test_gpu_train_dropout import check_step, facade, hip_loss_step
    cfg, B = dict(GOAL_ENVELOPE[name]["cfg"], embed_pdrob=embed_p), 33
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    assert name != "g3_no_goal_cond" or embed_p == 0
    meta = meta_of(name)
    state, goal, _ = inputs(name, B, 71)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 72).items()}
    model, seeds = facade(meta, cfg)
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=31)
    assert len(seeds) == 1 and seeds[0] > 0
    check_step(hip, oracle_step(meta, cfg, state, goal, li, seeds[0]), name, at_least=30)
    check_goal_gradients(name, cfg, hip, B)


@pytest.mark.parametrize("name,G,B", [("g2_shipped", 8, 1024), ("mdt_g3_pos", 3, 2752)])
def test_training_step_where_the_goal_embedder_runs_more_than_8192_rows(name, G, B):
    """g2_shipped widened to G = 8 at B = 1024, mdt_g3_pos at B = 2752: the goal embedder's forward, input gradient and weight gradient
    run on B * G >= 8192 rows -- the tall GEMM body, with the group scatter into the context where the product has one (MDT-V
    d = 384: goal_emb.2, K = 768) -- and MDT's position rows are added to 8256 goal rows.  Eval mode against float64 autograd."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from tests.test_gpu_train_dropout import check_step, hip_loss_step
    assert B * G >= 8192
    meta = meta_of(name, dict(goal_seq_len=G))
    cfg = dict(GOAL_ENVELOPE[name]["cfg"], goal_seq_len=G)
    model = GCDenoiser(cfg, 0.5)
    model.load_state_dict(params_of(meta))
    model = model.cuda().eval()
    state, goal, _ = inputs(name, B, 65, cfg=cfg)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(B, cfg, 66).items()}
    hip = hip_loss_step(model, meta, state, goal, li, torch_seed=1)
    check_step(hip, oracle_step(meta, cfg, state, goal, li), f"{name} G = {G}, B = {B}", at_least=30)
    check_goal_gradients(name, cfg, hip, B)


# ------------------------------------------------------------------------------------------------------------ 6. no oracle
def test_three_goal_rows_are_three_more_state_rows_when_the_embedders_agree():
    """MDT-V, goal_dim == obs_dim, plain Linear embedders, no modality encoder, goal_emb loaded with tok_emb's values: a G = 3 model
    on goal (g0, g1, g2) and a G = 1 model with n_obs_token + 2 state tokens on goal g0 and state (g1, g2, states) build the same
    context rows.  forward at B = 5, and 3-step sample_ddim at B = 1 and B = 8, agree at the forward tolerance."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    base = dict(goal_dim=384, use_mlp_goal=False, use_modality_encoder=False)
    cfg3 = configs.mdtv_default(goal_seq_len=3, **base)
    cfg1 = configs.mdtv_default(n_obs_token=5, **base)
    m3, m1 = GCDenoiser(cfg3, 0.5), GCDenoiser(cfg1, 0.5)
    P3 = envelope_params([(k, tuple(v.shape)) for k, v in m3.state_dict().items()], 241)
    for k in list(P3):
        for emb in ("goal_emb.", "lang_emb."):
            if k.startswith("inner_model." + emb):
                P3[k] = P3[k.replace(emb, "tok_emb.")].clone()
    P1 = envelope_params([(k, tuple(v.shape)) for k, v in m1.state_dict().items()], 241)
    for k in P1:
        if P1[k].shape == P3[k].shape:
            P1[k] = P3[k].clone()
        else:
            assert k == "inner_model.pos_emb", k   # MDT-V never reads it
    m3.load_state_dict(P3)
    m1.load_state_dict(P1)
    m3, m1 = m3.cuda().eval(), m1.cuda().eval()
    sig = gs.get_sigmas_exponential(3, 0.01, 80.0)
    for B, sampling in ((5, False), (1, True), (8, True)):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg3, 242 + B).items()}
        s3 = {"state_images": t["state_images"], "modality": "lang"}
        s1 = {"state_images": torch.cat([t["goal"][:, 1:], t["state_images"]], 1).contiguous(), "modality": "lang"}
        g3, g1 = t["goal"], t["goal"][:, :1].contiguous()
        with torch.no_grad():
            if sampling:
                a, b = (gs.sample_ddim(m, s, t["noise"] * 80.0, g, sig) for m, s, g in ((m3, s3, g3), (m1, s1, g1)))
            else:
                sigma = torch.from_numpy(synthetic.loss_inputs(B, cfg3, 243)["sigma"]).cuda()
                a, b = (m(s, t["noise"] * sigma[:, None, None], g, sigma) for m, s, g in ((m3, s3, g3), (m1, s1, g1)))
            assert_close(m3.inner_model.latent_encoder_emb.cpu(), m1.inner_model.latent_encoder_emb.cpu(), what=f"context, B = {B}")
        assert float(a.abs().max()) > 0.1
        assert_close(a.cpu(), b.cpu(), what=f"{'sample_ddim' if sampling else 'forward'}, B = {B}")


# ------------------------------------------------------------------------------------------------------------ 7. contrastive head
def test_contrastive_loss_pools_the_context_of_two_goal_tokens():
    """compute_contrastive_loss on g2_shipped's context (Te = 5, dropout off), B = 6, with the HIP MAPBlock: value and gradients
    against float64 autograd through the two oracles, as tests/test_gpu_map_long.py checks them at one goal token."""
    from mdt_policy_amd.models.contrastive import compute_contrastive_loss
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.models.networks.transformers.transformer_blocks import ClipStyleProjection
    from oracle import cla_oracle as CO
    name, B, style = "g2_shipped", 6, "map"
    ov = dict(GOAL_SPEC[name][2], attn_pdrop=0.0, resid_pdrop=0.0, mlp_pdrop=0.0)
    cfg = configs.mdtv_default(**ov)
    Te, G = GOAL_TE[name], cfg["goal_seq_len"]
    model = GCDenoiser(cfg, 0.5)
    meta = dict(config="mdtv_default", overrides=ov, arch="mdtv", weight_seed=231, profile="rich",
                state_dict=[[k, list(v.shape)] for k, v in model.state_dict().items()])
    PM = params_of(meta)
    model.load_state_dict(PM)
    model = model.cuda().eval()
    clip = ClipStyleProjection(style, token_dim=384, clip_token_index=1, num_token=Te)
    PC = envelope_params([(k, tuple(v.shape)) for k, v in clip.state_dict().items()], 232)
    clip.load_state_dict(PC)
    clip = clip.cuda()
    ls = torch.nn.Parameter(torch.tensor(float(np.log(1 / 0.07)), device="cuda"))
    inp = synthetic.sampler_inputs(B, cfg, 31, "mdtv")
    li = synthetic.loss_inputs(B, cfg, 32)
    img_goal = torch.from_numpy(synthetic.normal("img_goal", (B, G, 512), 33))
    state = {"state_images": torch.from_numpy(inp["state_images"]).cuda(), "modality": "lang"}
    a, nz, sg = (torch.from_numpy(li[k]).cuda() for k in ("actions", "noise_train", "sigma"))
    loss, _ = model.loss(state, a, torch.from_numpy(inp["goal"]).cuda(), nz, sg)
    assert model.inner_model.latent_encoder_emb.shape[1] == Te
    cont = compute_contrastive_loss(model, clip, ls, dict(state, modality="vis"), img_goal.cuda(), a, sg, nz)
    (loss + cont).backward()
    P = {k: v.double().requires_grad_(v.dtype.is_floating_point) for k, v in PM.items()}
    Q = {k: v.double().requires_grad_() for k, v in PC.items()}
    st = {"state_images": torch.from_numpy(inp["state_images"]).double(), "modality": "lang"}
    l64, _ = O.loss(P, cfg, st, torch.from_numpy(li["actions"]).double(), torch.from_numpy(inp["goal"]).double(),
                    torch.from_numpy(li["noise_train"]).double(), torch.from_numpy(li["sigma"]).double())
    ctx_l = O.encode(P, cfg, st, torch.from_numpy(inp["goal"]).double(), "mdtv", "forward")
    ctx_v = O.forward_context_only(P, cfg, dict(st, modality="vis"), img_goal.double())
    assert ctx_l.shape[1] == ctx_v.shape[1] == Te
    ls64 = torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float64, requires_grad=True)
    c64 = CO.clip_auxiliary_loss(CO.clip_style_projection(Q, ctx_v, style), CO.clip_style_projection(Q, ctx_l, style), ls64)
    (l64 + c64).backward()
    assert abs(cont.item() - c64.item()) <= 1e-3 * abs(c64.item())
    assert abs(ls.grad.item() - ls64.grad.item()) <= 2e-3 * abs(ls64.grad.item()) + 1e-6
    for k, p in clip.named_parameters():
        ref = Q[k].grad
        assert_close(p.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what="clip " + k)
    for k in ("goal_emb.0.weight", "lang_emb.2.weight", "tok_emb.weight", "encoder.blocks.0.attn.key.weight", "encoder.ln.weight",
              "decoder.blocks.1.mlp.c_fc.weight"):
        ref = P["inner_model." + k].grad
        got = dict(model.inner_model.named_parameters())[k].grad
        assert_close(got.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what=k)
