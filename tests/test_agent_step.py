"""The agent's training step as the reference composes it (MDTVAgent.training_step, mdt/models/mdtv_agent.py:222-298), against
float64 autograd through the oracles.  Every module is pinned on its own elsewhere; here they train TOGETHER:

  for each modality scope (lang, vis):   PerceiverResampler(tokens) -> state_images, modality set as compute_input_embeddings
                                         sets it (:360-391);  GCDenoiser.loss;  gen_img(latent_encoder_emb, imgs) +
                                         compute_loss, times masked_beta;  lang only: compute_contrastive_loss (:440-484) --
                                         a second, context-only forward of the denoiser (clip_extra_forward puts the model in
                                         train() mode), the MAP pooling head twice, InfoNCE
  total / number of scopes, ONE backward.

So every weight of every HIP module receives two or more gradients in one backward pass, and autograd adds them.  The frozen
encoders (Voltron tokens, language / image goal embeddings) are seeded input tensors; dropout probabilities are 0, so the
oracles' eval arithmetic is the exact expectation.  The oracles run on the GPU's fp64 units (they are the checkers, never the
thing measured).  Gate: 2e-3 relative to each tensor's largest entry, as test_c3_step.py / test_cla.py."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import configs, synthetic
from oracle import cla_oracle as CO
from oracle import mae_oracle as MO
from oracle import mdt_oracle as O
from oracle import perceiver_oracle as PO
from tests.helpers import assert_close, load_fixture, params_of

pytestmark = pytest.mark.gpu

MASKED_BETA, CONT_ALPHA = 1.0, 1.0  # conf/model/mdtv_agent.yaml
NO_DROPOUT = dict(attn_pdrop=0.0, resid_pdrop=0.0, mlp_pdrop=0.0)
TINY_RESAMPLER = dict(dim=128, depth=2, dim_head=32, heads=4, num_latents=3, num_time_embeds=1)


class _Agent(torch.nn.Module):
    """The four trained modules of MDTVAgent and its CLA temperature; ``forward(batch)`` is training_step's loss."""

    def __init__(self, model, gen, clip, perceiver, logit_scale):
        super().__init__()
        self.model, self.gen, self.clip_proj, self.perceiver = model, gen, clip, perceiver
        self.logit_scale = torch.nn.Parameter(logit_scale)

    def forward(self, batch):
        from mdt_policy_amd.models.contrastive import compute_contrastive_loss
        total, terms = 0.0, {}
        for scope, d in batch.items():
            perceptual_emb = {"state_images": self.perceiver(d["tokens"])}
            perceptual_emb["modality"] = scope
            act, _ = self.model.loss(perceptual_emb, d["actions"], d["goal"], d["noise"], d["sigma"])
            ctx = self.model.inner_model.latent_encoder_emb
            rec, mask, restore, _ = self.gen(ctx, d["imgs"], noise=d["mask_noise"])
            img = self.gen.compute_loss(d["imgs"], rec, mask, restore)
            total = total + img * MASKED_BETA
            if scope == "lang":
                cont = compute_contrastive_loss(self.model, self.clip_proj, self.logit_scale, perceptual_emb, d["img_goal"],
                                                d["actions"], d["sigma"], d["noise"])
                total = total + CONT_ALPHA * cont
                terms["cont"] = cont
            total = total + act
            terms[scope + " act"], terms[scope + " img"] = act, img
            terms[scope + " state_images"] = perceptual_emb["state_images"]
        return total / len(batch), terms


def _setup(size):
    """(cfg, head kwargs, clip kwargs, resampler kwargs, {module: float32 parameters})."""
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    dmeta, _ = load_fixture(f"g11_grads_mdtv_{size}.npz")
    cfg = (configs.mdtv_tiny if size == "tiny" else configs.mdtv_default)(**NO_DROPOUT)
    hmeta, hfx = load_fixture(f"g15_mae_{size}.npz")
    kw = hmeta["kwargs"]
    PH = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(
        [(k, tuple(s)) for k, s in hmeta["state_dict"] if k != "decoder_pe"], hmeta["weight_seed"], hmeta["profile"]).items()}
    PH["decoder_pe"] = torch.from_numpy(hfx["decoder_pe"])
    cmeta, _ = load_fixture(f"g14_cla_map_{size}.npz")
    PC = {k: torch.from_numpy(v) for k, v in
          synthetic.fill_state_dict([(k, tuple(s)) for k, s in cmeta["state_dict"]], cmeta["weight_seed"], cmeta["profile"]).items()}
    if size == "tiny":  # a resampler as wide as the tiny denoiser's tokens
        rkw = TINY_RESAMPLER
        shapes = [(k, tuple(v.shape)) for k, v in PerceiverResampler(**rkw).state_dict().items()]
        PR = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, 171, "rich").items()}
    else:  # the shipped resampler (6 layers, 3 latents, d = 384)
        rmeta, _ = load_fixture("g9_perceiver_default.npz")
        rkw = rmeta["kwargs"]
        PR = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(
            [(k, tuple(s)) for k, s in rmeta["state_dict"]], rmeta["weight_seed"], rmeta["profile"]).items()}
    assert cfg["obs_dim"] == rkw["dim"] == kw["context_dim"] == cmeta["kwargs"]["token_dim"]
    return cfg, kw, cmeta["kwargs"], rkw, {"model": params_of(dmeta), "gen": PH, "clip": PC, "perceiver": PR}


def _agent(cfg, kw, ckw, rkw, P):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.models.img_generation.masked_transformer_decoder import MaskedTransformerImgDecoder
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    from mdt_policy_amd.models.networks.transformers.transformer_blocks import ClipStyleProjection
    model = GCDenoiser(cfg, 0.5)
    model.load_state_dict(P["model"])
    gen = MaskedTransformerImgDecoder(**kw)
    gen.load_state_dict(P["gen"], strict=True)
    clip = ClipStyleProjection(**ckw)
    clip.load_state_dict(P["clip"])
    perc = PerceiverResampler(**rkw)
    perc.load_state_dict(P["perceiver"], strict=True)
    agent = _Agent(model, gen, clip, perc, torch.tensor(float(np.log(1 / 0.07)))).cuda()
    agent.model.eval()  # clip_extra_forward switches it to train() (no dropout here)
    return agent


def _batch(cfg, kw, rkw, sizes, seed, n_tokens):
    """{scope: float32 CPU inputs}; the lang scope carries the image goal of the contrastive term."""
    out = {}
    R, p = kw["resolution"], kw["patch_size"]
    for j, (scope, B) in enumerate(sizes.items()):
        s = seed + 10 * j
        li = synthetic.loss_inputs(B, cfg, s)
        d = {"tokens": synthetic.normal("tokens", (B, 1, n_tokens, rkw["dim"]), s + 1),
             "goal": synthetic.normal("goal", (B, 1, cfg["goal_dim"]), s + 2),
             "actions": li["actions"], "noise": li["noise_train"], "sigma": li["sigma"],
             "imgs": synthetic.normal("img", (B, 2, 3, R, R), s + 3),
             "mask_noise": synthetic.uniform("mask_noise", (B, (R // p) ** 2), s + 4)}
        if scope == "lang":
            d["img_goal"] = synthetic.normal("img_goal", (B, 1, cfg["goal_dim"]), s + 5)
        out[scope] = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    return out


def _on(batch, dev, dtype=None):
    return {s: {k: v.to(dev, dtype if dtype is not None else v.dtype) for k, v in d.items()} for s, d in batch.items()}


def _oracle_params(P):
    dev = "cuda"
    return {"model": {k: v.double().to(dev).requires_grad_(v.dtype.is_floating_point) for k, v in P["model"].items()},
            "gen": {k: v.double().to(dev).requires_grad_(k != "decoder_pe") for k, v in P["gen"].items()},
            "clip": {k: v.double().to(dev).requires_grad_() for k, v in P["clip"].items()},
            "perceiver": {k: v.double().to(dev).requires_grad_() for k, v in P["perceiver"].items()},
            "logit_scale": torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float64, device=dev, requires_grad=True)}


def _oracle_step(Q, cfg, kw, ckw, rkw, b64):
    """The same composition through perceiver_oracle, mdt_oracle, mae_oracle and cla_oracle (float64)."""
    total, terms = 0.0, {}
    for scope, d in b64.items():
        st = {"state_images": PO.perceiver_resampler(Q["perceiver"], d["tokens"], rkw["heads"]), "modality": scope}
        act, _ = O.loss(Q["model"], cfg, st, d["actions"], d["goal"], d["noise"], d["sigma"])
        ctx = O.encode(Q["model"], cfg, st, d["goal"], "mdtv", "forward", sigma=d["sigma"])
        rec, m, _, _ = MO.forward(Q["gen"], kw, ctx, d["imgs"], torch.argsort(d["mask_noise"], dim=1))
        img = MO.compute_loss(kw, d["imgs"], rec, m)
        total = total + img * MASKED_BETA
        if scope == "lang":
            ctx_v = O.forward_context_only(Q["model"], cfg, st, d["img_goal"], sigma=d["sigma"])
            pool = lambda x: CO.clip_style_projection(Q["clip"], x, ckw["clip_style"], ckw.get("clip_token_index", 0))
            cont = CO.clip_auxiliary_loss(pool(ctx_v), pool(ctx), Q["logit_scale"])
            total = total + CONT_ALPHA * cont
            terms["cont"] = cont
        total = total + act
        terms[scope + " act"], terms[scope + " img"], terms[scope + " state_images"] = act, img, st["state_images"]
    return total / len(b64), terms


def _close(got, ref, what, floor):
    ref = ref.detach().double().cpu()
    assert_close(got.detach().cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + floor, what=what)


def _mismatch(got, ref, what, floor):
    """_close's verdict as a message (None: within the gate), so that a step reports every wrong tensor, not the first."""
    try:
        _close(got, ref, what, floor)
    except AssertionError as e:
        return str(e)
    return None


def _check_step(agent, Q, out, ref, tokens, tokens64):
    """Every loss term, the resampled state tokens, EVERY parameter gradient of the four modules, d logit_scale and the
    gradients of the resampler's input tokens."""
    total, terms = out
    rtotal, rterms = ref
    for k, v in rterms.items():
        if v.dim() == 0:
            tol = (1e-3 if k == "cont" else 2e-3) * abs(v.item())
            assert abs(terms[k].item() - v.item()) <= tol, (k, terms[k].item(), v.item())
        else:
            _close(terms[k], v, k, 1e-7)
    assert abs(total.item() - rtotal.item()) <= 2e-3 * abs(rtotal.item()), (total.item(), rtotal.item())
    n, bad = 0, []
    # gradients: the floors of test_cla.py's composed step (denoiser -- its key biases have a gradient of exactly zero in
    # theory, fp32 noise of ~1e-9 in practice -- pooling head), test_c3_step.py (head) and test_perceiver.py (resampler)
    for name, mod, floor in (("model", agent.model, 1e-7), ("gen", agent.gen, 1e-9), ("clip", agent.clip_proj, 1e-7),
                             ("perceiver", agent.perceiver, 1e-7)):
        for k, p in mod.named_parameters():
            if not p.requires_grad:
                continue
            r = Q[name][k].grad
            if r is None:
                assert p.grad is None, (name, k)
                continue
            assert p.grad is not None, (name, k)
            bad.append(_mismatch(p.grad, r, f"{name} {k}", floor))
            n += 1
    for scope in tokens:
        bad.append(_mismatch(tokens[scope].grad, tokens64[scope].grad, f"{scope} d tokens", 1e-9))
    bad = [b for b in bad if b is not None]
    assert not bad, f"{len(bad)} of {n + len(tokens)} gradients outside the gate:\n" + "\n".join(bad)
    g, r = agent.logit_scale.grad.item(), Q["logit_scale"].grad.item()
    assert abs(g - r) <= 2e-3 * abs(r) + 1e-6, ("logit_scale", g, r)
    return n


def _run(agent, batch, Q, cfg, kw, ckw, rkw, before_backward=None, steps=1, seeds=None):
    """``steps`` facade steps without zero_grad (gradient accumulation) and their float64 twins; returns both last steps."""
    tokens, tokens64 = {}, {}
    for i in range(steps):
        b = batch if i == 0 else seeds[i]
        g = _on(b, "cuda")
        b64 = _on(b, "cuda", torch.float64)
        for s in g:
            g[s]["tokens"].requires_grad_()
            b64[s]["tokens"].requires_grad_()
            if i == 0:
                tokens[s], tokens64[s] = g[s]["tokens"], b64[s]["tokens"]
        out = agent(g)
        if before_backward is not None:
            before_backward()
        out[0].backward()
        ref = _oracle_step(Q, cfg, kw, ckw, rkw, b64)
        ref[0].backward()
    torch.cuda.synchronize()
    return out, ref, tokens, tokens64


def _side_launches():
    from mdt_policy_amd.models.img_generation import _hip_ops
    return _hip_ops.SIDE_LAUNCHES


@pytest.mark.parametrize("size,sizes,n_tokens", [("tiny", {"lang": 6, "vis": 9}, 20), ("default", {"lang": 32, "vis": 32}, 392)],
                         ids=["tiny", "default"])
def test_two_scope_step_matches_float64_oracles(size, sizes, n_tokens):
    """(a) tiny modules with a different batch per scope (the reference's datasets differ in size: tapes and buffers grow
    between the two forwards of one graph); (b) the shipped sizes at 32 per scope."""
    cfg, kw, ckw, rkw, P = _setup(size)
    agent = _agent(cfg, kw, ckw, rkw, P)
    Q = _oracle_params(P)
    batch = _batch(cfg, kw, rkw, sizes, 401, n_tokens)
    side0 = _side_launches()
    out, ref, tok, tok64 = _run(agent, batch, Q, cfg, kw, ckw, rkw)
    assert _check_step(agent, Q, out, ref, tok, tok64) > 100
    # every head weight fed two autograd nodes: none of their gradients may leave the backward chain
    assert _side_launches() == side0


def test_two_scope_step_with_a_held_back_side_stream():
    """(c) the head's weight-gradient side stream runs 1e8 cycles behind (about 50 ms): a gradient that autograd sums on the
    chain's stream without waiting for the side stream is then wrong on every run, not by timing luck.  A warm-up step on
    OTHER inputs (one head forward, one backward: its gradients go beside) creates the stream and leaves allocator blocks
    that do not hold this step's values."""
    from mdt_policy_amd.models.img_generation import _hip_ops
    cfg, kw, ckw, rkw, P = _setup("tiny")
    agent = _agent(cfg, kw, ckw, rkw, P)
    warm = _on(_batch(cfg, kw, rkw, {"lang": 6, "vis": 9}, 901, 20), "cuda")["vis"]
    ctx = torch.from_numpy(synthetic.normal("ctx", (9, 4, kw["context_dim"]), 902)).cuda()
    rec, mask, restore, _ = agent.gen(ctx, warm["imgs"], noise=warm["mask_noise"])
    agent.gen.compute_loss(warm["imgs"], rec, mask, restore).backward()
    agent.zero_grad(set_to_none=True)
    side = _hip_ops._SIDE[torch.cuda.current_device()]["stream"]

    def hold_back():
        with torch.cuda.stream(side):
            torch.cuda._sleep(100_000_000)  # one bounded spin: a delay, not a fault

    Q = _oracle_params(P)
    batch = _batch(cfg, kw, rkw, {"lang": 6, "vis": 9}, 401, 20)
    out, ref, tok, tok64 = _run(agent, batch, Q, cfg, kw, ckw, rkw, before_backward=hold_back)
    assert _check_step(agent, Q, out, ref, tok, tok64) > 100


def test_two_scope_steps_accumulate_gradients():
    """(d) Lightning's accumulate_grad_batches: two steps on different batches without zero_grad; every gradient equals the
    sum of the oracle's (the second backward meets parameters whose .grad exists)."""
    cfg, kw, ckw, rkw, P = _setup("tiny")
    agent = _agent(cfg, kw, ckw, rkw, P)
    Q = _oracle_params(P)
    batch = _batch(cfg, kw, rkw, {"lang": 6, "vis": 9}, 401, 20)
    second = _batch(cfg, kw, rkw, {"lang": 6, "vis": 9}, 501, 20)
    out, ref, tok, tok64 = _run(agent, batch, Q, cfg, kw, ckw, rkw, steps=2, seeds={1: second})
    assert _check_step(agent, Q, out, ref, tok, tok64) > 100


def test_one_forward_head_step_keeps_its_weight_gradients_beside_the_chain():
    """The rule behind (c) must not cost the step that has one head forward per backward (bench.py's
    train_step_c3_mdtv_B1024, tools/mae_bench.py): there the weight gradients still go to the side stream, and they are right."""
    cfg, kw, ckw, rkw, P = _setup("tiny")
    agent = _agent(cfg, kw, ckw, rkw, P)
    b = _on(_batch(cfg, kw, rkw, {"vis": 7}, 601, 20), "cuda")["vis"]
    ctx = torch.from_numpy(synthetic.normal("ctx", (7, 4, kw["context_dim"]), 602))
    c = ctx.cuda().requires_grad_()
    side0 = _side_launches()
    rec, mask, restore, _ = agent.gen(c, b["imgs"], noise=b["mask_noise"])
    agent.gen.compute_loss(b["imgs"], rec, mask, restore).backward()
    torch.cuda.synchronize()
    assert _side_launches() > side0
    PH = {k: v.double().cuda().requires_grad_(k != "decoder_pe") for k, v in P["gen"].items()}
    c64 = ctx.double().cuda().requires_grad_()
    imgs = b["imgs"].double()
    r64, m64, _, _ = MO.forward(PH, kw, c64, imgs, torch.argsort(b["mask_noise"], dim=1))
    MO.compute_loss(kw, imgs, r64, m64).backward()
    for k, p in agent.gen.named_parameters():
        if p.requires_grad:
            _close(p.grad, PH[k].grad, k, 1e-9)
    _close(c.grad, c64.grad, "d_context", 1e-9)


def _ddp_worker(rank, world, port, sizes, q):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)  # both ranks share the box's one GPU: RCCL cannot
    try:
        cfg, kw, ckw, rkw, P = _setup("tiny")
        agent = _agent(cfg, kw, ckw, rkw, P)
        ddp = DDP(agent, find_unused_parameters=True)
        full = _batch(cfg, kw, rkw, sizes, 401, 20)
        part = {s: {k: v[rank * v.shape[0] // world:(rank + 1) * v.shape[0] // world] for k, v in d.items()}
                for s, d in full.items()}
        total, terms = ddp(_on(part, "cuda"))
        total.backward()
        torch.cuda.synchronize()
        g = {k: p.grad.cpu().numpy() for k, p in agent.named_parameters() if p.grad is not None}
        q.put((rank, (g, terms["cont"].item()) if rank == 0 else None))
    finally:
        dist.destroy_process_group()


def test_two_scope_step_under_distributed_data_parallel():
    """Two ranks (gloo, both on the one GPU), each with half of every scope's batch, inside DistributedDataParallel: the
    staged denoiser backward (two staged chains and a context-only tape in one graph) and the all-gather of the contrastive
    term.  The averaged gradients equal the single-process step's on the whole batch:

    Rank r's loss is (act_r + img_r)/S per scope (means over its half) plus CONT_ALPHA * L / S, where L is the InfoNCE over
    the GATHERED batch -- the same value on every rank, the single-process contrastive loss.  all_gather_with_grad's backward
    sums the gradient of the gathered embeddings over the ranks and hands rank r its own block, so rank r's pooled
    embeddings receive world * dL/dx_r (test_cla.py::test_all_gather_with_grad_reproduces_the_global_batch_loss).  DDP
    divides the sum over the ranks by world: the mean terms give the full-batch mean's gradient (equal halves), the
    contrastive term gives sum_r dL/dx_r dx_r/dtheta = dL/dtheta, and d logit_scale (outside the gather: dL/ds on every
    rank) averages to dL/ds.  So no factor remains: averaged gradient = single-process gradient."""
    import torch.multiprocessing as mp
    from tests.test_sharding_gloo import _free_port
    sizes = {"lang": 6, "vis": 8}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, sizes, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    grads, cont = got[0]
    cfg, kw, ckw, rkw, P = _setup("tiny")
    agent = _agent(cfg, kw, ckw, rkw, P)
    total, terms = agent(_on(_batch(cfg, kw, rkw, sizes, 401, 20), "cuda"))
    total.backward()
    torch.cuda.synchronize()
    assert abs(cont - terms["cont"].item()) <= 1e-4 * abs(terms["cont"].item())
    full = {k: p.grad.cpu() for k, p in agent.named_parameters() if p.grad is not None}
    assert set(full) == set(grads) and len(full) > 100
    for k, ref in full.items():
        _close(torch.from_numpy(grads[k]), ref, k, 1e-7)
