#!/usr/bin/env python3
"""Record the reference's results with goals of several tokens (goal_seq_len > 1): tests/golden/g23_goalseq_<name>.npz for the
cases of tests/goal_seq_configs.py named in GOAL_GOLDEN.

Runs ONLY where the reference checkout exists, like make_golden.py, whose helpers it imports unchanged (the import stubs, the
reference builder, the DDIM runner, save); no test imports this file.

    python tests/golden/make_golden_goal_seq.py

Each fixture holds what the g21 fixtures hold (make_golden_ctx.py), at B = 2 with 'rich' weights: the 3-step DDIM actions with the
per-step denoised chunks and the context, the training loss of an eval-mode step, the gradients of the encoder inputs in full
(d_goal is (B, G, goal_dim)) and every parameter's gradient summary (l2 norm, sum, first 6 entries, one float64 row each in
``grads`` with meta['grad_names'] beside it), and the reference's state_dict names and shapes.  Outputs only: weights and inputs are
not stored, the tests regenerate them from mdt_policy_amd/synthetic.py (sampler_inputs draws the goal as (B, goal_seq_len,
goal_dim))."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
from mdt_policy_amd import configs, synthetic  # noqa: E402
from tests.goal_seq_configs import GOAL_GOLDEN, GOAL_GOLDEN_B, GOAL_SPEC, GOAL_TE  # noqa: E402

WEIGHT_SEED, INPUT_SEED, LOSS_SEED, CTX_SEED = 231, 232, 233, 234


def record(name):
    arch, factory, ov, proprio = GOAL_SPEC[name]
    assert not proprio, "the recorded cases run without the proprioceptive token"
    cfg = configs.NAMED[factory](**ov)
    B, G = GOAL_GOLDEN_B, cfg["goal_seq_len"]
    model = MG.build_reference(cfg, arch, seed=WEIGHT_SEED, profile="rich")
    res = MG.run_ddim(model, cfg, arch, B=B, n_steps=3, modality="lang", in_seed=INPUT_SEED, record=True)
    assert res["ctx"].shape[1] == GOAL_TE[name], res["ctx"].shape
    # the training step of g11: loss.backward() in eval mode plus a scalar hung on latent_encoder_emb
    inp = synthetic.sampler_inputs(B, cfg, INPUT_SEED, arch)
    assert inp["goal"].shape == (B, G, cfg["goal_dim"]) and G > 1
    li = synthetic.loss_inputs(B, cfg, LOSS_SEED)
    state = MG.make_state(inp, arch, "lang")
    leaves = {k: v.requires_grad_() for k, v in state.items() if torch.is_tensor(v)}
    goal = torch.from_numpy(inp["goal"]).requires_grad_()
    loss, _ = model.loss(state, torch.from_numpy(li["actions"]), goal, torch.from_numpy(li["noise_train"]), torch.from_numpy(li["sigma"]))
    ctx = model.inner_model.latent_encoder_emb
    wctx = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), CTX_SEED))
    (loss + 0.1 * (ctx * wctx).sum() / ctx.numel()).backward()
    names, rows = [], []
    for k, p in model.named_parameters():
        names.append(k)
        row = np.full(8, np.nan)   # all NaN: the reference left no gradient
        if p.grad is not None:
            g = p.grad.detach().double()
            head = g.flatten()[:6]
            row[:2], row[2:2 + head.numel()], row[2 + head.numel():] = [float(g.norm()), float(g.sum())], head.numpy(), 0.0
        rows.append(row)
    arrays = {"d_" + k: v.grad.numpy() for k, v in leaves.items()}
    arrays["d_goal"] = goal.grad.numpy() if goal.grad is not None else np.zeros(tuple(goal.shape), np.float32)
    arrays["grads"] = np.stack(rows)
    meta = dict(config=factory, overrides=ov, arch=arch, B=B, n_steps=3, modality="lang", weight_seed=WEIGHT_SEED, profile="rich",
                input_seed=INPUT_SEED, loss_seed=LOSS_SEED, ctx_seed=CTX_SEED, sigma_min=0.001, sigma_max=80.0, grad_names=names,
                state_dict=[[k, list(v.shape)] for k, v in model.state_dict().items()])
    MG.save(f"g23_goalseq_{name}.npz", meta, loss=np.array(loss.item(), np.float32), **res, **arrays)


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), f"{MG.REF} not found: the recorder runs only beside the reference checkout"
    MG.install_stubs()
    torch.manual_seed(0)
    for case in sys.argv[1:] or GOAL_GOLDEN:
        record(case)
