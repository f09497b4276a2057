"""The adaptive DPM-Solver's host pieces (CPU tier): the step-size controller mdt_sample_dpm_adaptive runs (mdt_dpm_control_*)
against gc_sampling._StepControl on the same error sequences -- rejects and NaN included -- and a replay of the native driver in
numpy (the step plans of mdt_dpm_adaptive_plan applied with the toy denoiser of test_native_sampler_plan.py, the controller
helper, the driver's fp32 step arithmetic) against gc_sampling.sample_dpm_adaptive driving the same toy model."""
import math

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.test_native_sampler_plan import A, B, TA, apply_plan, toy_model

ERRORS = [0.3, 2.5, 4.0, 0.9, 0.05, 1.2, 7.0, 0.0, 0.6, 1.0, 3.3, 0.01, 0.81, 1.5]


@pytest.mark.parametrize("kw", [dict(pcoeff=0., icoeff=1., dcoeff=0., order=3, safety=0.81),
                                dict(pcoeff=0.3, icoeff=0.6, dcoeff=0.1, order=2, safety=0.81),
                                dict(pcoeff=0.1, icoeff=0.5, dcoeff=0.2, order=3, safety=0.95)])
@pytest.mark.parametrize("h0", [0.05, -0.4])
def test_controller_reproduces_step_control_exactly(kw, h0):
    ref = gs._StepControl(h0, kw["pcoeff"], kw["icoeff"], kw["dcoeff"], kw["order"], kw["safety"])
    nat = _lib.DpmController(h0, kw["pcoeff"], kw["icoeff"], kw["dcoeff"], kw["order"], kw["safety"])
    decisions = []
    for err in ERRORS:
        e32 = float(np.float32(err))  # the driver hands over torch's fp32 error
        ok = ref.update(torch.tensor(e32, dtype=torch.float32))
        d = nat.update(e32)
        assert d == (_lib.DPM_ACCEPT if ok else _lib.DPM_REJECT)
        assert nat.h == ref.h, "h differs from _StepControl's"
        decisions.append(ok)
    assert True in decisions and False in decisions, "the sequence must exercise both accepts and rejects"


def test_controller_reports_a_stop_on_nan():
    nat = _lib.DpmController(0.05, 0., 1., 0., 3, 0.81)
    assert nat.update(0.4) in (_lib.DPM_ACCEPT, _lib.DPM_REJECT)
    assert nat.update(float("nan")) == _lib.DPM_STOP
    ref = gs._StepControl(0.05, 0., 1., 0., 3, 0.81)
    ref.update(torch.tensor(0.4))
    ref.update(torch.tensor(float("nan")))
    assert math.isnan(ref.h)  # where the Python loop would spin forever


def _replay(x_T, sigma_min, sigma_max, order, rtol=0.05, atol=0.0078, h_init=0.05, pcoeff=0., icoeff=1., dcoeff=0.,
            accept_safety=0.81):
    """mdt_sample_dpm_adaptive's loop in numpy float64 (the device's fp32 error and pointer swaps aside)."""
    f32 = np.float32
    t_start = f32(gs._t(torch.tensor(float(sigma_max))).item())
    t_end = f32(gs._t(torch.tensor(float(sigma_min))).item())
    forward = t_end > t_start
    ctl = _lib.DpmController(abs(h_init) if forward else -abs(h_init), pcoeff, icoeff, dcoeff, order, accept_safety)
    info = dict(steps=0, nfe=0, n_accept=0, n_reject=0)
    x, prev, s = x_T.copy(), x_T.copy(), t_start
    end_lo, end_hi = f32(t_end - f32(1e-5)), f32(t_end + f32(1e-5))
    while (s < end_lo) if forward else (s > end_hi):
        step = f32(s + f32(ctl.h))
        t = min(t_end, step) if forward else max(t_end, step)
        plan = _lib.dpm_adaptive_plan(order, s, t)
        hi, lo = _apply_pair(plan, x)
        tol = np.maximum(rtol * np.maximum(np.abs(lo), np.abs(prev)), atol)
        err = np.linalg.norm((lo - hi) / tol) / math.sqrt(lo.size)
        d = ctl.update(err)
        assert d != _lib.DPM_STOP
        info["steps"] += 1
        info["nfe"] += plan.n_evals
        if d == _lib.DPM_ACCEPT:
            x, prev, s = hi, lo, t
            info["n_accept"] += 1
        else:
            info["n_reject"] += 1
    return x, info


def _apply_pair(plan, x):
    """(high, low) of one attempt: apply_plan gives the last evaluation's X' (cx); its Y' (cy, no X' term) is the low result."""
    zero = np.zeros((1,) + x.shape)
    hi = apply_plan(plan, x, zero)
    z = plan.e[plan.n_evals - 1]
    assert z.cy[_lib.SAMPLER_NREG] == 0.0
    for k in range(_lib.SAMPLER_NREG):
        z.cx[k] = z.cy[k]
    return hi, apply_plan(plan, x, zero)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("levels,h_init", [((0.001, 80.0), 0.05), ((0.01, 80.0), 2.0), ((80.0, 0.01), 0.05)],
                         ids=["forward", "forward-large-h", "reverse"])
def test_native_driver_replay_matches_the_host_loop(order, levels, h_init):
    sigma_min, sigma_max = levels
    x_T = np.random.default_rng(order).standard_normal((B, TA, A)) * max(levels)
    want, winfo = gs.sample_dpm_adaptive(toy_model, {}, torch.from_numpy(x_T.copy()), None, sigma_min, sigma_max, order=order,
                                         h_init=h_init, return_info=True)
    got, info = _replay(x_T, sigma_min, sigma_max, order, h_init=h_init)
    assert info == winfo
    scale = float(np.abs(want.numpy()).max())
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-5, atol=1e-5 * scale)


def test_large_h_init_setting_has_rejects():
    x_T = np.random.default_rng(2).standard_normal((B, TA, A)) * 80.0
    _, info = gs.sample_dpm_adaptive(toy_model, {}, torch.from_numpy(x_T), None, 0.01, 80.0, order=3, h_init=2.0,
                                     return_info=True)
    assert info["n_reject"] > 0
