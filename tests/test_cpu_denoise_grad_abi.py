"""CPU-tier checks of the differentiable denoiser's boundary (mdt_train_denoise_fwd / _bwd, GCDenoiser.denoise_grad): the
gfx950 build loads without a GPU, exports and declares both entry points, refuses bad calls with a status instead of touching a
device, and the facade refuses CPU execution.  What needs a live handle -- MDT_ERR_STATE without mdt_train_prepare, an unknown
tape, NULL arguments on a prepared handle -- runs in tests/test_gpu_denoise_grad.py: mdt_create needs a device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from mdt_policy_amd import _lib, configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mdt_train_denoise_fwd", "mdt_train_denoise_bwd")


def test_both_entry_points_are_exported_declared_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mdt_hip_train.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    table = {s[0]: s for s in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), f"libmdt_hip.so does not export {name}"
        assert re.search(r"\bmdt_status\s+" + name + r"\s*\(", code), f"{name} is not declared in mdt_hip_train.h"
        assert name in table and table[name][1] is C.c_int32
    assert len(table["mdt_train_denoise_fwd"][2]) == 9 and len(table["mdt_train_denoise_bwd"][2]) == 8
    # the header states the limit of d_sigma
    assert "MDT_ERR_UNSUPPORTED" in hdr[hdr.index("mdt_train_denoise_fwd"):hdr.index("kernel level")]


def test_null_and_bad_arguments_are_statuses_not_crashes():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    tape = C.c_int32(-1)
    # no handle: MDT_ERR_INVALID_ARG before anything else is looked at
    assert lib.mdt_train_denoise_fwd(None, p, p, p, 1, None, p, C.byref(tape), None) == 1
    assert lib.mdt_train_denoise_fwd(None, None, None, None, 0, None, None, None, None) == 1
    assert tape.value == -1
    assert lib.mdt_train_denoise_bwd(None, 0, p, p, p, p, p, None) == 1
    assert lib.mdt_train_denoise_bwd(None, -1, None, None, None, None, None, None) == 1
    assert b"null handle" in lib.mdt_last_error()


def test_denoise_grad_is_public_and_refuses_cpu_execution():
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    sig = inspect.signature(GCDenoiser.denoise_grad)
    assert list(sig.parameters)[1:] == ["state", "action", "goal", "sigma", "cond_lambda", "context", "uncond"]
    assert sig.parameters["cond_lambda"].default == 1.0 and sig.parameters["context"].default is None
    assert sig.parameters["uncond"].default is False
    m = GCDenoiser(configs.mdtv_tiny(), 0.5).eval()
    state = {"state_images": torch.zeros(1, 3, 128), "modality": "lang"}
    args = (state, torch.zeros(1, 10, 7), torch.zeros(1, 1, 512), torch.ones(1))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.denoise_grad(*args)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.denoise_grad(*args, context=torch.zeros(1, 4, 128))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.denoise_grad(*args, cond_lambda=2.5)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        m.denoise_grad(*args)
    with pytest.raises(ValueError):
        m.denoise_grad(*args, cond_lambda=float("nan"))
    with pytest.raises(ValueError):
        m.denoise_grad(*args, cond_lambda=2.0, uncond=True)
    # the implicit call keeps refusing autograd, and now says where the explicit form is
    with pytest.raises(NotImplementedError, match="autograd.*denoise_grad"):
        m(*args)

