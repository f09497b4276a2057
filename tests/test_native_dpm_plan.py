"""DPM-Solver-fast as a sampler plan (CPU tier): mdt_sampler_plan for MDT_SAMPLER_DPM_FAST, applied in numpy with the closed-form
toy denoiser of test_native_sampler_plan.py, against gc_sampling.sample_dpm_fast driving the same toy model -- 1..12, 30 and 128
evaluations, both directions, eta in {0, 0.5} with recorded noise -- plus the plan's t grid against torch.linspace bit for bit,
its noise-row count against the loop's draws, and the argument checks."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.test_native_sampler_plan import A, B, TA, apply_plan, toy_model

NS = list(range(1, 13)) + [30, 128]
LEVELS = [(80.0, 0.001), (14.0, 0.03), (0.01, 80.0)]  # (sigma_max, sigma_min); the last one samples in reverse


class _Recorder:
    """A noise_sampler that hands out seeded Gaussian rows and records them."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.rows = []

    def __call__(self, s0, s1):
        z = torch.randn((B, TA, A), generator=self.g, dtype=torch.float64)
        self.rows.append(z.numpy())
        return z


def _step_starts(plan):
    """t of the first evaluation of every solver step."""
    return [plan.e[k].t for k in range(plan.n_evals) if k == 0 or plan.e[k].step != plan.e[k - 1].step]


# eta != 0 in reverse is rejected (test_dpm_fast_plan_rejects_bad_arguments)
SETTINGS = [(lv, eta) for lv in LEVELS for eta in (0.0, 0.5) if not (eta and lv[1] > lv[0])]


@pytest.mark.parametrize("levels,eta", SETTINGS, ids=[f"{lv[0]}-{lv[1]}-eta{eta}" for lv, eta in SETTINGS])
@pytest.mark.parametrize("n", NS)
def test_dpm_fast_plan_applied_with_a_toy_denoiser_matches_the_host_loop(n, levels, eta):
    smax, smin = levels
    x_T = torch.from_numpy(np.random.default_rng(n).standard_normal((B, TA, A))) * smax
    rec = _Recorder(7 + n)
    want = gs.sample_dpm_fast(toy_model, {}, x_T.clone(), None, smin, smax, n, eta=eta, noise_sampler=rec).numpy()

    plan = _lib.sampler_plan("dpm_fast", [smax, smin], n_steps=n, eta=eta)
    assert plan.n_evals == n
    assert plan.n_noise == len(rec.rows), "the plan's noise rows differ from the loop's noise_sampler calls"
    assert plan.y0_draws + sum(plan.e[k].draws for k in range(plan.n_evals)) == plan.n_noise
    noise = np.stack(rec.rows) if rec.rows else np.zeros((1, B, TA, A))
    got = apply_plan(plan, x_T.numpy(), noise)
    scale = float(np.abs(want).max())
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6 * scale)


@pytest.mark.parametrize("levels", LEVELS, ids=["80-0.001", "14-0.03", "reverse"])
def test_dpm_fast_plan_steps_on_the_torch_linspace_grid_bit_for_bit(levels):
    smax, smin = levels
    t0, t1 = gs._t(torch.tensor(smax)), gs._t(torch.tensor(smin))
    for n in range(1, _lib.SAMPLER_MAX_EVALS + 1):
        m = n // 3 + 1
        grid = torch.linspace(gs._f(t0), gs._f(t1), m + 1)
        plan = _lib.sampler_plan("dpm_fast", [smax, smin], n_steps=n, eta=0.)
        starts = np.asarray(_step_starts(plan), dtype=np.float32)
        assert len(starts) == m
        assert np.array_equal(starts, grid[:-1].numpy()), f"n={n}"


def test_dpm_fast_plan_orders_and_noise_shape():
    for n in (1, 2, 3, 9, 10, 11, 128):
        m = n // 3 + 1
        orders = [3] * (m - 2) + [2, 1] if n % 3 == 0 else [3] * (m - 1) + [n % 3]
        plan = _lib.sampler_plan("dpm_fast", [80.0, 0.001], n_steps=n, eta=0.)
        per_step = [sum(1 for k in range(plan.n_evals) if plan.e[k].step == i) for i in range(m)]
        assert per_step == orders
        assert plan.n_noise == 0
        assert all(list(plan.e[k].noise) == [-1, -1] for k in range(plan.n_evals))
        # with eta: at most one row per step, never on the last (it ends at sigma_min)
        pe = _lib.sampler_plan("dpm_fast", [80.0, 0.001], n_steps=n, eta=1.)
        assert pe.n_noise <= m - 1


def test_dpm_fast_plan_rejects_bad_arguments():
    for n in (0, -1, _lib.SAMPLER_MAX_EVALS + 1):
        with pytest.raises(_lib.MDTHipError):
            _lib.sampler_plan("dpm_fast", [80.0, 0.001], n_steps=n, eta=0.)
    for levels in ([0.0, 0.001], [80.0, 0.0], [-1.0, 0.001], [80.0, -0.5]):
        with pytest.raises(_lib.MDTHipError):
            _lib.sampler_plan("dpm_fast", levels, n_steps=10, eta=0.)
    with pytest.raises(_lib.MDTHipError):  # eta != 0 in reverse, as sample_dpm_fast's ValueError
        _lib.sampler_plan("dpm_fast", [0.01, 80.0], n_steps=10, eta=0.5)
    _lib.sampler_plan("dpm_fast", [0.01, 80.0], n_steps=10, eta=0.)
    _lib.sampler_plan("dpm_fast", [80.0, 0.001], n_steps=_lib.SAMPLER_MAX_EVALS, eta=1.)


def test_dpm_fast_routing_condition_keeps_other_models_on_the_host_loop():
    """A plain callable is not a GCDenoiser: the loop runs it (with the callback the native path cannot serve)."""
    calls = []
    x_T = torch.from_numpy(np.random.default_rng(3).standard_normal((B, TA, A))) * 80.0
    gs.sample_dpm_fast(toy_model, {}, x_T, None, 0.001, 80.0, 10, callback=calls.append)
    assert len(calls) == 10 // 3 + 1
