"""The CPU oracle with goals of several tokens against what the reference recorded (tests/golden/g23_goalseq_*.npz, written by
tests/golden/make_golden_goal_seq.py): the yardstick of the GPU tests in tests/test_gpu_goal_seq*.py holds at goal_seq_len > 1.
Tolerances are those of tests/test_long_context_golden.py: the float32 oracle's context TIGHT, the denoised chunks and the actions
to 1e-4 / 1e-4; the float64 oracle under autograd gives the loss to 1e-4 and the gradient summaries and input gradients (d_goal is
(B, G, goal_dim)) to 2e-3."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.goal_seq_configs import GOAL_ENVELOPE, GOAL_GOLDEN, GOAL_TE, context_len, goal_rows
from tests.helpers import assert_close, cfg_of, inputs_of, load_fixture, params_of
from tests.test_long_chunks_golden import recorded_summaries
from tests.test_oracle_golden import TIGHT
from tests.test_train_grads import check_summaries, oracle_total, summary


def test_the_table_states_its_context_lengths():
    assert {n: context_len(n) for n in GOAL_ENVELOPE} == GOAL_TE
    assert all(goal_rows(n) > 1 for n in GOAL_ENVELOPE)


@pytest.mark.parametrize("name", GOAL_GOLDEN)
def test_oracle_sampling_matches_the_reference(name):
    """3-step DDIM at B = 2 (float32 oracle): the context of the last step, every step's denoised chunk and the actions."""
    meta, fx = load_fixture(f"g23_goalseq_{name}.npz")
    cfg, P = cfg_of(meta), params_of(meta)
    assert cfg == GOAL_ENVELOPE[name]["cfg"] and fx["ctx"].shape[1] == GOAL_TE[name]
    state, goal, noise = inputs_of(meta)
    assert tuple(goal.shape) == (meta["B"], goal_rows(name), cfg["goal_dim"])
    sig = torch.from_numpy(fx["sigmas"])
    steps = []
    out = O.sample_ddim(P, cfg, state, noise * meta["sigma_max"], goal, sig, arch=meta["arch"], per_step=steps)
    last = sig[-2] * torch.ones(noise.shape[0])  # the fixture holds the context of the LAST step
    ctx = O.encode(P, cfg, state, goal, meta["arch"], sigma=last).numpy()
    print(f"{name}: max |oracle - reference| actions {np.abs(out.numpy() - fx['actions']).max():.2e}, "
          f"denoised {np.abs(torch.stack(steps).numpy() - fx['denoised_steps']).max():.2e}, ctx {np.abs(ctx - fx['ctx']).max():.2e}")
    assert_close(ctx, fx["ctx"], what="ctx", **TIGHT)
    assert_close(torch.stack(steps).numpy(), fx["denoised_steps"], what="denoised", rtol=1e-4, atol=1e-4)
    assert_close(out.numpy(), fx["actions"], what="actions", rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", GOAL_GOLDEN)
def test_oracle_autograd_matches_the_reference_gradients(name):
    """The eval-mode training step (float64 oracle): the loss to 1e-4, every parameter's gradient summary and the input gradients,
    d_goal (B, G, goal_dim) among them, to 2e-3."""
    meta, fx = load_fixture(f"g23_goalseq_{name}.npz")
    cfg = cfg_of(meta)
    state, goal, _ = inputs_of(meta)
    li = {k: torch.from_numpy(v) for k, v in synthetic.loss_inputs(meta["B"], cfg, meta["loss_seed"]).items()}
    P = {k: v.double().requires_grad_(v.dtype.is_floating_point) for k, v in params_of(meta).items()}
    state = {k: (v.double().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    goal = goal.double().requires_grad_()
    loss, total = oracle_total(P, cfg, meta, state, goal, li, torch.float64)
    total.backward()
    want_loss = float(np.asarray(fx["loss"]).reshape(-1)[0])
    assert abs(loss.item() - want_loss) <= 1e-4 * abs(want_loss)
    got = {k[len("inner_model."):]: summary(v.grad) for k, v in P.items() if v.grad is not None}
    want = {k[len("inner_model."):]: v for k, v in recorded_summaries(meta, fx).items()}
    assert sum(v is not None for v in want.values()) > 20
    check_summaries({k: v for k, v in got.items() if k in want and want[k] is not None}, want, name)
    for k, v in state.items():
        if torch.is_tensor(v):
            assert_close(v.grad, fx["d_" + k], rtol=2e-3, atol=1e-7, what="d_" + k)
    assert fx["d_goal"].shape == (meta["B"], goal_rows(name), cfg["goal_dim"]) and np.abs(fx["d_goal"]).min(axis=(0, 2)).shape == (goal_rows(name),)
    assert bool((np.abs(fx["d_goal"]).max(axis=(0, 2)) > 0).all()), "a goal row without a gradient"
    assert_close(goal.grad, fx["d_goal"], rtol=2e-3, atol=1e-7, what="d_goal")
