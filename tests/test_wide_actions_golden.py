"""The CPU oracle at action vectors of 17 .. 64 elements against what the reference recorded (tests/golden/g20_wide_*.npz,
written by tests/golden/make_golden_wide.py): the yardstick of the GPU tests in tests/test_gpu_wide_actions.py holds at these
widths.  The sampling check runs the oracle in float32 on the regenerated weights and the gradient check in float64 under
autograd, at exactly the tolerances of tests/test_long_chunks_golden.py (TIGHT on the context, 1e-4 / 1e-4 on the denoised chunks
and the actions; the loss to 1e-4, gradient summaries and input gradients to 2e-3); the action-wide layers' gradients, stored in
full, are held to the same 2e-3 of their own largest value.  Every check prints its largest error (pytest -s)."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.helpers import assert_close, cfg_of, load_fixture, observation, params_of
from tests.test_long_chunks_golden import recorded_summaries
from tests.test_oracle_golden import TIGHT
from tests.test_train_grads import check_summaries, oracle_total, summary
from tests.wide_action_configs import WIDE_GOLDEN


def case_inputs(meta):
    cfg = cfg_of(meta)
    state, goal, noise = observation(cfg, meta["arch"], meta["proprio"], meta["B"], meta["input_seed"], obs_seed=meta["obs_seed"])
    return cfg, dict(state, modality=meta["modality"]), goal, noise


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_oracle_sampling_matches_the_reference(name):
    """10-step DDIM at B = 2 (float32 oracle): the context of the last step, the first and the last step's denoised chunk and
    the actions."""
    meta, fx = load_fixture(f"g20_wide_{name}.npz")
    cfg, state, goal, noise = case_inputs(meta)
    P = params_of(meta)
    assert cfg["action_dim"] > 16 and fx["actions"].shape[-1] == cfg["action_dim"]
    sig = torch.from_numpy(fx["sigmas"])
    steps = []
    out = O.sample_ddim(P, cfg, state, noise * meta["sigma_max"], goal, sig, arch=meta["arch"], per_step=steps)
    last = sig[-2] * torch.ones(noise.shape[0])  # the fixture holds the context of the LAST step
    assert_close(O.encode(P, cfg, state, goal, meta["arch"], sigma=last).numpy(), fx["ctx"], what="ctx", **TIGHT)
    print(f"{name}: max |oracle - reference| denoised {np.abs(torch.stack([steps[0], steps[-1]]).numpy() - fx['denoised_steps']).max():.3e}, "
          f"actions {np.abs(out.numpy() - fx['actions']).max():.3e}")
    assert_close(torch.stack([steps[0], steps[-1]]).numpy(), fx["denoised_steps"], what="denoised", rtol=1e-4, atol=1e-4)
    assert_close(out.numpy(), fx["actions"], what="actions", rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", WIDE_GOLDEN)
def test_oracle_autograd_matches_the_reference_gradients(name):
    """The eval-mode training step at per-sample sigmas (float64 oracle): the loss to 1e-4, model_output, every parameter's
    gradient summary, the action-wide layers' gradients in full and the input gradients to 2e-3."""
    meta, fx = load_fixture(f"g20_wide_{name}.npz")
    cfg, state, goal, _ = case_inputs(meta)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(meta["B"], cfg, meta["loss_seed"]).items()}
    assert len(set(li["sigma"].tolist())) == meta["B"] > 1   # per-sample sigmas
    P = {k: v.double().requires_grad_(v.dtype.is_floating_point) for k, v in params_of(meta).items()}
    state = {k: (v.double().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    goal = goal.double().requires_grad_()
    loss, total = oracle_total(P, cfg, meta, state, goal, li, torch.float64)
    total.backward()
    want_loss = float(np.asarray(fx["loss"]).reshape(-1)[0])
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss)
    with torch.no_grad():
        _, mo = O.loss({k: v.detach() for k, v in P.items()}, cfg, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in state.items()},
                       li["actions"].double(), goal.detach(), li["noise_train"].double(), li["sigma"].double(), arch=meta["arch"])
    assert_close(mo.numpy(), fx["model_output"], what="model_output")
    got = {k[len("inner_model."):]: summary(v.grad) for k, v in P.items() if v.grad is not None}
    want = {k[len("inner_model."):]: v for k, v in recorded_summaries(meta, fx).items()}
    assert sum(v is not None for v in want.values()) > 20
    check_summaries({k: v for k, v in got.items() if k in want and want[k] is not None}, want, name)
    full = [k for k in fx if k.startswith("g_")]
    assert len(full) == 4
    worst = 0.0
    for k in full:
        ref = fx[k].astype(np.float64)
        scale = float(np.abs(ref).max())
        worst = max(worst, float(np.abs(P[k[2:]].grad.numpy() - ref).max()) / scale)
        assert_close(P[k[2:]].grad, ref, rtol=2e-3, atol=2e-3 * scale + 1e-7, what=k)
    print(f"{name}: loss {loss.item():.7g} / reference {want_loss:.7g}; action-wide gradients within {worst:.2e} of their largest value")
    for k, v in state.items():
        if torch.is_tensor(v):
            assert_close(v.grad, fx["d_" + k], rtol=2e-3, atol=1e-7, what="d_" + k)
    assert_close(goal.grad, fx["d_goal"], rtol=2e-3, atol=1e-7, what="d_goal")
