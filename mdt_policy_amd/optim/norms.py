"""Multi-tensor L2 norms on the device (``mdt_op_multi_sumsq``): one reduction over a whole list of tensors, no atomics, no
read-back.  ``total_norms`` replaces the body of the agent's ``on_before_zero_grad`` (mdt/models/mdtv_agent.py:201-212), which
reads one ``.norm().item()`` per tensor back to the host."""
from __future__ import annotations

import torch

from .. import _lib


def check_tensor(t: torch.Tensor, what: str) -> None:
    if t.device.type != "cuda" or t.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 tensors on a ROCm GPU only")
    if t.is_sparse:
        raise RuntimeError(f"{what}: sparse tensors are not supported")


def multi_sumsq(tensors, which: int = 0, partials: torch.Tensor | None = None) -> torch.Tensor:
    """(2,) fp32 device tensor: the sum of squares and the count of non-finite elements over ``tensors`` (a non-empty list of
    contiguous fp32 tensors of one GPU), handed to the library as the ``g`` (which = 0) or ``p`` (which = 1) members of its
    table.  ``partials``: scratch to reuse; a fresh buffer is taken from torch's allocator when it is missing or too small.
    Bit-identical from call to call; nothing here waits for the device."""
    lib = _lib.load()
    dev = tensors[0].device
    tab = (_lib.OptTensor * len(tensors))()
    for i, t in enumerate(tensors):
        if t.device != dev:
            raise RuntimeError("multi_sumsq: all tensors must live on one device")
        tab[i] = _lib.OptTensor(p=t.data_ptr() if which else None, g=None if which else t.data_ptr(), m=None, v=None, ema=None,
                                numel=t.numel())
    need = lib.mdt_op_multi_sumsq_scratch(tab, len(tensors))
    if partials is None or partials.numel() < need or partials.device != dev:
        partials = torch.empty(max(need, 1), dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.mdt_op_multi_sumsq(tab, len(tensors), which, out.data_ptr(), partials.data_ptr(), partials.numel(),
                                          torch.cuda.current_stream(dev).cuda_stream))
    return out


def total_norms(parameters):
    """``(grad_norm, param_norm)``: the L2 norm over all gradients and over all parameters as two 0-dim device tensors, i.e.
    ``sum(p.grad.norm() ** 2) ** 0.5`` and ``sum(p.norm() ** 2) ** 0.5`` of the reference's logging hook from two launches
    each and without a read-back -- call ``.item()`` on them when the logger wants the numbers.  Parameters without ``.grad``
    count in the parameter norm only, as in the hook."""
    ps = [p for p in parameters]
    if not ps:
        raise ValueError("total_norms: no parameters")
    vals, grads = [], []
    for p in ps:
        check_tensor(p, "total_norms")
        vals.append(p.detach() if p.is_contiguous() else p.detach().contiguous())
        if p.grad is not None:
            check_tensor(p.grad, "total_norms")
            grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
    param_norm = multi_sumsq(vals, which=1)[0].sqrt()
    grad_norm = multi_sumsq(grads, which=0)[0].sqrt() if grads else torch.zeros((), dtype=torch.float32, device=ps[0].device)
    return grad_norm, param_norm
