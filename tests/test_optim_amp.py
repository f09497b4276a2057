"""FusedAdamW's device-driven step (AMP scaling, overflow skip, norm clipping) and the multi-tensor norm reduction: what can be
checked without a GPU -- the C ABI's argument checks, the Python surface torch.amp.GradScaler looks at, and a float64
restatement of the control arithmetic of k_opt_ctl that the GPU tests (tests/test_gpu_optim_amp.py) share."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, ERR_HIP = 1, 4


def control_block(step, beta1, beta2, grad_scale=None, found_inf=None, grad_sumsq=None, max_norm=0.0):
    """What k_opt_ctl leaves behind, in float64 (rounded to fp32 where the kernel stores fp32): the new step count, skip,
    bc1, sqrt(bc2), g_mult and the unscaled gradient norm.  None = the pointer is NULL."""
    skip = found_inf is not None and not (np.float32(found_inf) == 0)
    t = float(step) if skip else float(np.float32(step) + np.float32(1))
    inv_scale = float(np.float32(1.0 / float(np.float32(grad_scale)))) if grad_scale is not None else 1.0
    coef, norm = 1.0, None
    if grad_sumsq is not None:
        norm = math.sqrt(float(np.float32(grad_sumsq))) * inv_scale
        if max_norm > 0:
            coef = min(1.0, float(np.float32(max_norm)) / (norm + 1e-6))
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return dict(step=t, skip=bool(skip), bc1=float(np.float32(1.0 - b1 ** t)), bc2_sqrt=float(np.float32(math.sqrt(1.0 - b2 ** t))),
                g_mult=float(np.float32(inv_scale * coef)), grad_norm=None if norm is None else float(np.float32(norm)))


def test_control_block_restatement_follows_adamw_and_clip_grad_norm():
    c = control_block(0.0, 0.9, 0.95)
    assert (c["step"], c["skip"], c["g_mult"], c["grad_norm"]) == (1.0, False, 1.0, None)
    assert c["bc1"] == pytest.approx(0.1, rel=1e-6) and c["bc2_sqrt"] == pytest.approx(math.sqrt(0.05), rel=1e-6)
    # a clean scaled step: the norm is unscaled before it is compared with max_norm
    c = control_block(4.0, 0.9, 0.999, grad_scale=1024.0, found_inf=0.0, grad_sumsq=(1024.0 * 3.0) ** 2, max_norm=1.0)
    assert c["step"] == 5.0 and not c["skip"]
    assert c["grad_norm"] == pytest.approx(3.0, rel=1e-6)
    assert c["g_mult"] == pytest.approx((1.0 / 1024.0) / (3.0 + 1e-6), rel=1e-6)
    # below the bound nothing is clipped; without max_norm the norm is still reported
    assert control_block(4.0, 0.9, 0.999, grad_scale=2.0, grad_sumsq=1.0, max_norm=1.0)["g_mult"] == 0.5
    assert control_block(4.0, 0.9, 0.999, grad_sumsq=16.0)["grad_norm"] == 4.0
    # an overflow (any nonzero found_inf, NaN included) leaves the count alone
    for bad in (1.0, 2.0, float("nan")):
        c = control_block(7.0, 0.9, 0.999, grad_scale=65536.0, found_inf=bad, grad_sumsq=float("inf"), max_norm=1.0)
        assert c["skip"] and c["step"] == 7.0


def test_library_exports_the_device_driven_optimizer_entry_points():
    lib = _lib.load()
    names = [n for n, _, _ in _lib.SYMBOLS]
    for name in ("mdt_op_multi_sumsq", "mdt_op_multi_sumsq_scratch", "mdt_op_multi_adamw_dev"):
        assert name in names and getattr(lib, name) is not None


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    """Status 1 (invalid argument) with a message, never 4 (a HIP call failed): the checks come first, GPU or not."""
    lib = _lib.load()
    one = (_lib.OptTensor * 1)()
    one[0] = _lib.OptTensor(p=64, g=64, m=64, v=64, ema=None, numel=8)
    out = C.c_void_p(64)

    def refused(status, needle):
        assert status == INVALID_ARG != ERR_HIP, status
        assert needle in lib.mdt_last_error().decode()

    refused(lib.mdt_op_multi_sumsq(None, 1, 0, out, None, 0, None), "mdt_op_multi_sumsq")
    refused(lib.mdt_op_multi_sumsq(one, -1, 0, out, None, 0, None), "mdt_op_multi_sumsq")
    refused(lib.mdt_op_multi_sumsq(one, 1, 0, None, None, 0, None), "mdt_op_multi_sumsq")
    refused(lib.mdt_op_multi_sumsq(one, 1, 2, out, None, 0, None), "mdt_op_multi_sumsq")
    refused(lib.mdt_op_multi_sumsq(one, 1, 0, out, out, 1, None), "partials")  # one chunk needs two floats
    nog = (_lib.OptTensor * 1)()
    nog[0] = _lib.OptTensor(p=64, g=None, m=None, v=None, ema=None, numel=8)
    refused(lib.mdt_op_multi_sumsq(nog, 1, 0, out, None, 0, None), "lacks g")
    hp = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    refused(lib.mdt_op_multi_adamw_dev(None, 1, *hp, out, None, None, None, 0.0, None, None), "mdt_op_multi_adamw_dev")
    refused(lib.mdt_op_multi_adamw_dev(one, -1, *hp, out, None, None, None, 0.0, None, None), "mdt_op_multi_adamw_dev")
    refused(lib.mdt_op_multi_adamw_dev(one, 1, *hp, None, None, None, None, 0.0, None, None), "mdt_op_multi_adamw_dev")
    refused(lib.mdt_op_multi_adamw_dev(one, 1, *hp, out, None, None, None, 1.0, None, None), "mdt_op_multi_adamw_dev")  # clip without a norm
    refused(lib.mdt_op_multi_adamw_dev(one, 1, *hp, out, None, None, None, float("nan"), None, None), "mdt_op_multi_adamw_dev")
    refused(lib.mdt_op_multi_adamw_dev(nog, 1, *hp, out, None, None, None, 0.0, None, None), "lacks p / g / m / v")
    assert lib.mdt_op_multi_sumsq_scratch(one, 1) == 2
    big = (_lib.OptTensor * 2)()
    big[0] = _lib.OptTensor(p=64, g=64, m=None, v=None, ema=None, numel=4097)
    big[1] = _lib.OptTensor(p=64, g=64, m=None, v=None, ema=None, numel=0)
    assert lib.mdt_op_multi_sumsq_scratch(big, 2) == 4
    assert lib.mdt_op_multi_sumsq_scratch(None, 2) == 0


def test_fused_adamw_speaks_the_grad_scaler_attribute_protocol():
    """torch.amp.GradScaler.step looks for _step_supports_amp_scaling and, on torch 2.10, hands grad_scale / found_inf over
    as attributes -- unless step() still takes the deprecated grad_scaler keyword."""
    import torch
    from mdt_policy_amd.optim import FusedAdamW, total_norms
    assert FusedAdamW._step_supports_amp_scaling is True
    assert "grad_scaler" not in inspect.signature(FusedAdamW.step).parameters
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedAdamW([p], lr=1e-3, max_grad_norm=1.0)
    assert "grad_scaler" not in inspect.signature(opt.step).parameters  # the instance's (profiler-wrapped) step too
    assert opt.max_grad_norm == 1.0 and opt.grad_norm is None
    assert FusedAdamW([p]).max_grad_norm is None
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW([p], max_grad_norm=bad)
    assert callable(total_norms)
    assert "grad" in FusedAdamW.__doc__ and "rewrite" in FusedAdamW.__doc__  # unlike clip_grad_norm_: says so


def test_device_path_refuses_cpu_parameters_as_the_plain_step_does():
    import torch
    from mdt_policy_amd.optim import FusedAdamW, total_norms
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        FusedAdamW([p], max_grad_norm=1.0).step()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        total_norms([p])
    with pytest.raises(ValueError):
        total_norms([])


def _function_body(src, name):
    start = src.index(f'extern "C" mdt_status {name}(')
    end = src.find('\nextern "C"', start + 1)
    return src[start:end if end > 0 else len(src)]


def test_the_two_entry_points_never_wait_for_the_stream():
    """torch's sync debug mode (tests/test_gpu_optim_amp.py) sees torch's own calls only: that the library's side of a device
    step enqueues and returns is read off its source.  (upload_opt_table, shared with mdt_op_multi_adamw, waits on an event only
    when it evicts a table that a kernel may still read.)"""
    src = open(os.path.join(ROOT, "mdt_policy_amd", "csrc", "mdt_train_ops.hip")).read()
    for name in ("mdt_op_multi_sumsq", "mdt_op_multi_adamw_dev"):
        body = re.sub(r"//[^\n]*", "", _function_body(src, name))
        for blocking in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy(", "hipMemcpyDtoH", "hipMemset("):
            assert blocking not in body, (name, blocking)
