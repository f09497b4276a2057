"""What the modules backed by one library handle share: the tape a training forward leaves in the library, the flat
gradient layout a handle reports, and the handle lifecycle of the single-handle facades (PerceiverResampler,
MAPBlock): creation on the module's device, parameter upload when a parameter changed, the tape-keeping autograd
Function.  The C entry points of a facade are ``<prefix>_*`` (include/mdt_resampler.h, include/mdt_map_pool.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch
from torch import nn

from ... import _lib


class LibTape:
    """Owns one library tape: released after the backward, or when the autograd node dies without one."""

    def __init__(self, tape_id: int, release):
        self.id, self._release = tape_id, release

    def release(self):
        if self.id is not None:
            try:
                self._release(self.id)
            except Exception:
                pass  # handle already destroyed
            self.id = None

    __del__ = release


def grad_layout(lib, prefix: str, handle):
    """({parameter name: (offset, numel)} in the handle's flat gradient, its total numel) from the ``<prefix>_param_name /
    _param_numel / _grad_offset / _grad_numel`` entry points (training prepared)."""
    name, numel, offset = (getattr(lib, f"{prefix}_{s}") for s in ("param_name", "param_numel", "grad_offset"))
    n = getattr(lib, f"{prefix}_param_count")(handle)
    layout = {name(handle, i).decode(): (int(offset(handle, i)), int(numel(handle, i))) for i in range(n)}
    return layout, int(getattr(lib, f"{prefix}_grad_numel")(handle))


class _HandleFn(torch.autograd.Function):
    """forward of a HandleModule under autograd: the HIP forward keeps a tape, the HIP backward turns it into the gradient of
    every parameter (views of one flat buffer) and of the input.  `extra` (the resampler's mask) is not differentiable."""

    @staticmethod
    def forward(ctx, mod, x, extra, names, *params):
        lib, stream = mod._engine(x.device, train=True)
        tape = C.c_int32(-1)
        out = mod._launch(lib, x, extra, stream, C.byref(tape))
        ctx.mod, ctx.tape = mod, LibTape(int(tape.value), mod._release_tape)
        ctx.named = list(zip(names, params))
        ctx.x_shape, ctx.need_x = x.shape, x.requires_grad
        return out

    @staticmethod
    def backward(ctx, g_out):
        mod = ctx.mod
        if ctx.tape.id is None:
            raise RuntimeError(f"the HIP {mod._what} tape of this forward was already consumed (no retain_graph support)")
        lib = _lib.load()
        stream = torch.cuda.current_stream(g_out.device).cuda_stream
        g = g_out.detach().float().contiguous()
        grads = torch.zeros(mod._grad_numel, device=g.device, dtype=torch.float32)
        d_x = torch.empty(ctx.x_shape, device=g.device, dtype=torch.float32) if ctx.need_x else None
        _lib.check(getattr(lib, mod._prefix + "_backward")(mod._handle, ctx.tape.id, g.data_ptr(), grads.data_ptr(),
                                                           None if d_x is None else d_x.data_ptr(), stream))
        ctx.tape.release()
        out = []
        for name, p in ctx.named:
            off, n = mod._grad_layout[name]
            out.append(grads[off:off + n].view(p.shape) if p.requires_grad else None)
        return (None, d_x, None, None, *out)


class HandleModule(nn.Module):
    """A module whose forward and backward run in one library handle.  Subclasses set ``_prefix`` (C symbol prefix),
    ``_config`` (the ctypes config struct, built from ``self._cfg``), ``_what`` (name in messages) and ``_no_cpu`` (the
    error for a non-GPU device), call ``_init_handle()`` in their constructor and implement ``_launch``."""

    _prefix: str
    _config: type
    _what: str
    _no_cpu: str

    def _init_handle(self):
        from ...utils import weight_cache
        weight_cache.track(self)
        self._handle: Optional[C.c_void_p] = None
        self._handle_device = None
        self._uploaded: Dict[str, tuple] = {}
        self._grad_layout = None

    def _launch(self, lib, x, extra, stream, tape=None) -> torch.Tensor:
        """The module's output for the prepared input x: the inference entry point, or with `tape` (a pointer to an int32)
        the training forward that keeps one."""
        raise NotImplementedError

    # -- library handle --------------------------------------------------------------------------
    def __getstate__(self):  # copy.deepcopy / pickle: never the library handle
        d = self.__dict__.copy()
        d["_handle"], d["_handle_device"], d["_uploaded"], d["_grad_layout"] = None, None, {}, None
        return d

    def __setstate__(self, state):  # the copy is a new module: register it with the optimizer hook (utils/weight_cache.py)
        super().__setstate__(state)
        from ...utils import weight_cache
        weight_cache.track(self)
        self.mark_dirty()

    def _apply(self, fn, *a, **kw):  # .to()/.cuda(): parameters are re-created, drop the stale handle
        out = super()._apply(fn, *a, **kw)
        self._drop_handle()
        return out

    def _drop_handle(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                getattr(_lib.load(), self._prefix + "_destroy")(h)
            except Exception:
                pass
        self._handle, self._handle_device, self._uploaded, self._grad_layout = None, None, {}, None

    def __del__(self):
        try:
            self._drop_handle()
        except Exception:
            pass

    def _release_tape(self, tape_id: int) -> None:
        if self._handle is not None:
            getattr(_lib.load(), self._prefix + "_tape_release")(self._handle, tape_id)

    def mark_dirty(self) -> None:
        """Forget what was uploaded (weights written through ``.data`` / a foreign fused optimizer are not seen by the
        version counter): the next call re-uploads every parameter."""
        self._uploaded = {}

    def train(self, mode: bool = True):
        out = super().train(mode)
        self._uploaded = {}
        return out

    def _engine(self, device: torch.device, train: bool = False):
        if device.type != "cuda":
            raise RuntimeError(self._no_cpu)
        lib = _lib.load()
        if self._handle is None or self._handle_device != device:
            self._drop_handle()
            cfg = self._config(**self._cfg)
            h = C.c_void_p()
            from ...utils import torch_allocator
            torch_allocator.install()  # workspace / tapes / scratch live in torch's caching allocator
            with torch.cuda.device(device):
                _lib.check(getattr(lib, self._prefix + "_create")(C.byref(cfg), C.byref(h)))
            self._handle, self._handle_device = h, device
        if train and self._grad_layout is None:
            _lib.check(getattr(lib, self._prefix + "_train_prepare")(self._handle))
            self._uploaded = {}  # every weight is uploaded again so that its transposed image exists
            self._grad_layout, self._grad_numel = grad_layout(lib, self._prefix, self._handle)
        stream = torch.cuda.current_stream(device).cuda_stream
        for name, p in self.named_parameters():
            tag = (p.data_ptr(), p._version)
            if self._uploaded.get(name) == tag:
                continue
            if p.device != device or p.dtype != torch.float32:
                raise RuntimeError(f"parameter {name} must be float32 on {device}, got {p.dtype} on {p.device}")
            src = p.detach().contiguous()
            _lib.check(getattr(lib, self._prefix + "_load_param")(self._handle, name.encode(), src.data_ptr(), src.numel(),
                                                                  stream))
            self._uploaded[name] = tag
        return lib, stream

    @staticmethod
    def _input(x: torch.Tensor) -> torch.Tensor:
        """x as the kernels read it: float32, contiguous, 16-byte aligned (x itself when it already is)."""
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        return x if x.data_ptr() % 16 == 0 else x.clone()

    def _run(self, x: torch.Tensor, extra=None) -> torch.Tensor:
        """The module's output for x: under autograd through the tape-keeping Function, else the inference entry point."""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if x.device.type != "cuda":
                self._engine(x.device)  # raises the no-CPU-path error
            named = list(self.named_parameters())
            return _HandleFn.apply(self, self._input(x), extra, [k for k, _ in named], *[p for _, p in named])
        lib, stream = self._engine(x.device)
        return self._launch(lib, self._input(x.detach()), extra, stream)
