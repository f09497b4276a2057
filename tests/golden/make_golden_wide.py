#!/usr/bin/env python3
"""Record the reference's results at action vectors of 17 .. 64 elements: tests/golden/g20_wide_<name>.npz for the cases of
tests/wide_action_configs.py named in WIDE_GOLDEN.

Runs ONLY where the reference checkout exists, like make_golden.py, whose helpers it imports unchanged (the import stubs, the
reference builder, make_state, save); no test imports this file.

    python tests/golden/make_golden_wide.py

Each fixture holds, at B = 2 with 'rich' weights: the 10-step DDIM actions with the denoised chunk of the first and the last step
and the context; the training loss of an eval-mode step at per-sample sigmas with its model_output; the reference's
loss.backward() gradients of action_emb.* and of the action-wide layer of action_pred in full (float32, ``g_<name>``), the gradients of the encoder inputs
in full and every parameter's gradient summary (l2 norm, sum, first 6 entries: g11's figures, kept as a float64 array ``grads``
with meta['grad_names'] beside it); and the reference's state_dict names and shapes.  Weights and inputs are not stored: the tests
regenerate them from mdt_policy_amd/synthetic.py (state_obs of the proprioceptive case from meta['obs_seed'])."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG  # noqa: E402
from mdt_policy_amd import configs, synthetic  # noqa: E402
from tests.wide_action_configs import WIDE_GOLDEN, WIDE_GOLDEN_B, WIDE_SPEC  # noqa: E402

WEIGHT_SEED, INPUT_SEED, LOSS_SEED, CTX_SEED, OBS_SEED = 201, 202, 203, 204, 205
N_STEPS = 10


def record(name):
    from mdt.models.edm_diffusion import gc_sampling
    arch, factory, ov, proprio = WIDE_SPEC[name]
    cfg = configs.NAMED[factory](**ov)
    B = WIDE_GOLDEN_B
    model = MG.build_reference(cfg, arch, seed=WEIGHT_SEED, profile="rich")
    inp = synthetic.sampler_inputs(B, cfg, INPUT_SEED, arch)
    li = synthetic.loss_inputs(B, cfg, LOSS_SEED)

    def fresh_state():
        state = MG.make_state(inp, arch, "lang")
        if proprio:
            state["state_obs"] = torch.from_numpy(synthetic.normal("state_obs", (B, 1, cfg["proprio_dim"]), OBS_SEED))
        return state

    arrays = {}
    with torch.no_grad():
        sigmas = gc_sampling.get_sigmas_exponential(N_STEPS, 0.001, 80.0)
        den = []
        out = gc_sampling.sample_ddim(model, fresh_state(), torch.from_numpy(inp["noise"]) * 80.0, torch.from_numpy(inp["goal"]), sigmas,
                                      disable=True, callback=lambda d: den.append(d["denoised"].clone()))
        arrays.update(actions=out.numpy(), sigmas=sigmas.numpy(), denoised_steps=torch.stack([den[0], den[-1]]).numpy(),
                      ctx=model.inner_model.latent_encoder_emb.detach().numpy())
    # the training step of g11: loss.backward() in eval mode plus a scalar hung on latent_encoder_emb
    state = fresh_state()
    leaves = {k: v.requires_grad_() for k, v in state.items() if torch.is_tensor(v)}
    goal = torch.from_numpy(inp["goal"]).requires_grad_()
    loss, mo = model.loss(state, torch.from_numpy(li["actions"]), goal, torch.from_numpy(li["noise_train"]), torch.from_numpy(li["sigma"]))
    ctx = model.inner_model.latent_encoder_emb
    wctx = torch.from_numpy(synthetic.normal("ctx_weight", tuple(ctx.shape), CTX_SEED))
    (loss + 0.1 * (ctx * wctx).sum() / ctx.numel()).backward()
    names, rows = [], []
    for k, p in model.named_parameters():
        names.append(k)
        row = np.full(8, np.nan)
        if p.grad is not None:
            g = p.grad.detach().double()
            head = g.flatten()[:6]
            row[:2], row[2:2 + head.numel()], row[2 + head.numel():] = [float(g.norm()), float(g.sum())], head.numpy(), 0.0
            if (".action_emb." in k or ".action_pred." in k) and ".action_pred.0." not in k:   # the layers as wide as the action
                arrays["g_" + k] = p.grad.detach().numpy()
        rows.append(row)
    arrays.update({"d_" + k: v.grad.numpy() for k, v in leaves.items()})
    arrays["d_goal"] = goal.grad.numpy()
    arrays["grads"] = np.stack(rows)
    arrays["model_output"] = mo.detach().numpy()
    meta = dict(config=factory, overrides=ov, arch=arch, proprio=proprio, B=B, n_steps=N_STEPS, modality="lang", weight_seed=WEIGHT_SEED,
                profile="rich", input_seed=INPUT_SEED, loss_seed=LOSS_SEED, ctx_seed=CTX_SEED, obs_seed=OBS_SEED, sigma_min=0.001,
                sigma_max=80.0, grad_names=names, state_dict=[[k, list(v.shape)] for k, v in model.state_dict().items()])
    MG.save(f"g20_wide_{name}.npz", meta, loss=np.array(loss.item(), np.float32), **arrays)


if __name__ == "__main__":
    assert os.path.isdir(MG.REF), f"{MG.REF} not found: the recorder runs only beside the reference checkout"
    MG.install_stubs()
    torch.manual_seed(0)
    for case in sys.argv[1:] or WIDE_GOLDEN:
        record(case)
