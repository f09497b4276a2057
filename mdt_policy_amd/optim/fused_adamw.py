"""AdamW whose step() is ONE hand-written gfx950 launch per parameter group (``mdt_op_multi_adamw``).

Drop-in for the ``torch.optim.AdamW(optim_groups, lr=..., betas=...)`` the reference builds in
``MDTVAgent.configure_optimizers`` (mdt/models/mdtv_agent.py:164-199): same constructor arguments, same state_dict
layout (``step`` / ``exp_avg`` / ``exp_avg_sq`` per parameter), same arithmetic (decoupled weight decay, bias
correction).  fp32 CUDA(ROCm) parameters only; anything else raises -- there is no eager fallback here.

With ``torch.amp.GradScaler`` or ``max_grad_norm`` the step runs from device scalars (``mdt_op_multi_adamw_dev``): the
unscale, the overflow skip, the norm clip and the step count all stay on the GPU and ``step()`` reads nothing back.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .norms import multi_sumsq


class _Cohort:
    """Parameters of one group that share a step count, and that count as a (1,) fp32 device tensor."""
    __slots__ = ("counter", "params")

    def __init__(self, counter, params):
        self.counter, self.params = counter, params


def _bump_versions(ps):
    # the library wrote the parameters behind autograd's back: bump their version counters (no kernel) so
    # that the HIP engines see the change and re-upload the weights before the next forward
    try:
        torch._C._autograd._unsafe_set_version_counter(ps, [p._version + 1 for p in ps])
    except (AttributeError, TypeError):  # other torch builds: an in-place no-op bumps it the public way
        torch._foreach_add_(ps, 0.0)


def _device_scalar(t, dev, what):
    if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or t.numel() != 1:
        raise RuntimeError(f"FusedAdamW: {what} must be one float32 element on the parameters' device")
    return t.data_ptr()


class FusedAdamW(torch.optim.Optimizer):
    """``max_grad_norm``: clip the global gradient norm (over all groups, as ``torch.nn.utils.clip_grad_norm_`` does over the
    list it is given) inside the update.  After each such step ``grad_norm`` holds the unscaled norm before clipping as a
    0-dim device tensor (0 reports the norm and clips nothing).  Unlike ``clip_grad_norm_`` (and ``GradScaler.unscale_``) this
    does NOT rewrite ``p.grad``: the gradients keep their loss scale and their length, only the update sees them unscaled
    and clipped.

    ``GradScaler.step(opt)`` hands the scale and its overflow flag over as tensors (``_step_supports_amp_scaling``), so it
    runs neither ``unscale_`` nor the ``found_inf.item()`` that goes with it; leave Lightning's ``gradient_clip_val`` unset."""

    _step_supports_amp_scaling = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *,
                 max_grad_norm: float | None = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameter")
        if max_grad_norm is not None and not (float(max_grad_norm) >= 0):  # negative or NaN
            raise ValueError("max_grad_norm must be a non-negative number or None")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        # host-side caches (not part of state_dict): the step count as a Python int and the addresses of the moment
        # buffers, so that a step makes two tensor calls per parameter instead of seven
        self._nsteps, self._mv = {}, {}
        # device path: parameter -> its cohort.  While a parameter is in here the cohort's device counter is its step count
        # and state[p]["step"] is stale until _sync_steps()
        self._dev, self._partials = {}, None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._nsteps, self._mv, self._dev = {}, {}, {}

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def _sync_steps(self):
        """Materialise state[p]["step"] from the device counters: one read-back per cohort (state_dict(), or a plain step
        after device-path steps)."""
        done = set()
        for c in self._dev.values():
            if id(c) in done:
                continue
            done.add(id(c))
            n = float(c.counter.item())
            for p in c.params:
                self.state[p]["step"] = torch.tensor(n)
                self._nsteps[p] = int(n)

    def _state_of(self, p):
        """Checks, lazily created state and the cached moment addresses of a parameter that has a gradient; True if the
        cache was (re)built, i.e. the step count has to be taken from state[p]["step"]."""
        if p.device.type != "cuda" or p.dtype != torch.float32 or p.grad.dtype != torch.float32:
            raise RuntimeError("FusedAdamW updates float32 parameters on a ROCm GPU only")
        if p.grad.is_sparse:
            raise RuntimeError("FusedAdamW does not support sparse gradients")
        if not p.is_contiguous():
            raise RuntimeError("FusedAdamW needs contiguous parameters")
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        mv = self._mv.get(p)
        if mv is None or mv[0] is not st["exp_avg"] or mv[1] is not st["exp_avg_sq"]:
            self._mv[p] = (st["exp_avg"], st["exp_avg_sq"], st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
            return True
        return False

    @torch.no_grad()
    def _step_device(self, grad_scale, found_inf):
        lib = _lib.load()
        dev, work = None, []
        for group in self.param_groups:
            items, joining = [], {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if dev is None:
                    dev = p.device
                elif p.device != dev:
                    raise RuntimeError("FusedAdamW with a GradScaler or max_grad_norm needs all parameters on one device")
                fresh = self._state_of(p)
                c = self._dev.get(p)
                if c is not None and fresh:  # its state was replaced by hand: the step count is the new state's
                    c.params = [q for q in c.params if q is not p]
                    del self._dev[p]
                    self._nsteps.pop(p, None)
                    c = None
                if c is None:
                    n = self._nsteps.get(p)
                    if n is None or fresh:
                        n = int(self.state[p]["step"].item())
                    joining.setdefault(n, []).append(p)
                items.append((p, p.grad if p.grad.is_contiguous() else p.grad.contiguous()))
            for n, ps in joining.items():  # torch.full is a fill kernel: no host-to-device copy, nothing to wait for
                c = _Cohort(torch.full((1,), float(n), dtype=torch.float32, device=dev), ps)
                for p in ps:
                    self._dev[p] = c
            by = {}
            for it in items:
                c = self._dev[it[0]]
                by.setdefault(id(c), (c, []))[1].append(it)
            for c, its in by.values():
                if len(its) != len(c.params):  # members without a gradient keep their count: they leave with a copy of it
                    here = {id(p) for p, _ in its}
                    rest = _Cohort(c.counter.clone(), [q for q in c.params if id(q) not in here])
                    for q in rest.params:
                        self._dev[q] = rest
                    c.params = [p for p, _ in its]
                work.append((group, c, its))
        if dev is None:
            return
        scale_ptr = None if grad_scale is None else _device_scalar(grad_scale, dev, "grad_scale")
        inf_ptr = None if found_inf is None else _device_scalar(found_inf, dev, "found_inf")
        sumsq_ptr = norm_ptr = None
        if self.max_grad_norm is not None:  # ONE reduction over the gradients of all groups: the norm is global
            grads = [g for _, _, its in work for _, g in its]
            need = 2 * sum((g.numel() + 4095) // 4096 for g in grads)
            if self._partials is None or self._partials.numel() < need or self._partials.device != dev:
                self._partials = torch.empty(need, dtype=torch.float32, device=dev)
            sumsq = multi_sumsq(grads, 0, self._partials)
            self.grad_norm = torch.empty((), dtype=torch.float32, device=dev)
            sumsq_ptr, norm_ptr = sumsq.data_ptr(), self.grad_norm.data_ptr()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for group, c, its in work:
                tab = (_lib.OptTensor * len(its))()
                for i, (p, g) in enumerate(its):
                    _, _, m_ptr, v_ptr, numel = self._mv[p]
                    tab[i] = _lib.OptTensor(p=p.data_ptr(), g=g.data_ptr(), m=m_ptr, v=v_ptr, ema=None, numel=numel)
                _lib.check(lib.mdt_op_multi_adamw_dev(tab, len(its), float(group["lr"]), float(group["betas"][0]),
                                                      float(group["betas"][1]), float(group["eps"]),
                                                      float(group["weight_decay"]), c.counter.data_ptr(), scale_ptr, inf_ptr,
                                                      sumsq_ptr, self.max_grad_norm or 0.0, norm_ptr, stream))
                _bump_versions([p for p, _ in its])  # also when the device skips the step: the host cannot know

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        d = self.__dict__  # GradScaler.step sets the two attributes around this call and deletes them again
        if "found_inf" in d or "grad_scale" in d or self.max_grad_norm is not None:
            self._step_device(d.get("grad_scale"), d.get("found_inf"))
            return loss
        if self._dev:  # a plain step after device-path steps: take the counts back to the host
            self._sync_steps()
            self._dev = {}
        lib = _lib.load()
        for group in self.param_groups:
            by_step, steps = {}, []
            for p in group["params"]:
                if p.grad is None:
                    continue
                # the body of _state_of, inline: as a call per parameter it added about 5 us to a 0.51 ms step over 148 tensors
                if p.device.type != "cuda" or p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise RuntimeError("FusedAdamW updates float32 parameters on a ROCm GPU only")
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdamW does not support sparse gradients")
                if not p.is_contiguous():
                    raise RuntimeError("FusedAdamW needs contiguous parameters")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                n = self._nsteps.get(p)
                mv = self._mv.get(p)
                if n is None or mv is None or mv[0] is not st["exp_avg"] or mv[1] is not st["exp_avg_sq"]:
                    n = int(st["step"].item())
                    self._mv[p] = (st["exp_avg"], st["exp_avg_sq"], st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                                   p.numel())
                self._nsteps[p] = n + 1
                steps.append(st["step"])
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                by_step.setdefault(n + 1, []).append((p, g))
            if steps:
                torch._foreach_add_(steps, 1.0)  # the state_dict's per-parameter counters, one call for all of them
            for step, items in by_step.items():  # parameters that joined later carry their own step count
                tab = (_lib.OptTensor * len(items))()
                for i, (p, g) in enumerate(items):
                    _, _, m_ptr, v_ptr, numel = self._mv[p]
                    tab[i] = _lib.OptTensor(p=p.data_ptr(), g=g.data_ptr(), m=m_ptr, v=v_ptr, ema=None, numel=numel)
                dev = items[0][0].device
                with torch.cuda.device(dev):
                    _lib.check(lib.mdt_op_multi_adamw(tab, len(items), float(group["lr"]), float(group["betas"][0]),
                                                      float(group["betas"][1]), float(group["eps"]),
                                                      float(group["weight_decay"]), step,
                                                      torch.cuda.current_stream(dev).cuda_stream))
                _bump_versions([p for p, _ in items])
        return loss
