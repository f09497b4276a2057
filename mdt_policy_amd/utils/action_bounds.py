"""Per-dimension action bounds: the ``scaler`` of a harness run with ``use_scaler``.

The reference agent hands ``scaler=self.scaler`` to its samplers when ``use_scaler`` is set (mdtv_agent.py:606-614), and the sampler
loops call ``action = scaler.clip_output(action)`` after every step.  ``ActionBounds`` is that object for this package: its
``clip_output`` is ``torch.clamp`` to the bounds, and because it also exposes them (``clip_bounds``) the native samplers apply
the same clamp inside their one call (include/mdt_hip.h mdt_sample_opts) instead of falling back to the host loop.  Assign it
to ``agent.scaler``.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch


def _host_vector(v, name: str) -> torch.Tensor:
    t = torch.as_tensor(v).detach().to("cpu", torch.float32).reshape(-1).clone()
    if t.numel() < 1:
        raise ValueError(f"ActionBounds: {name} is empty")
    if bool(torch.isnan(t).any()):
        raise ValueError(f"ActionBounds: {name} holds NaN")
    return t


class ActionBounds:
    """``lo`` and ``hi``: sequences, arrays or tensors of ``action_dim`` values each (finite or +-inf, no NaN, lo <= hi),
    checked on the host here.  ``action_dim``: the length both must have (None: whatever ``lo`` has)."""

    def __init__(self, lo, hi, action_dim: int = None):
        self.lo, self.hi = _host_vector(lo, "lo"), _host_vector(hi, "hi")
        n = self.lo.numel() if action_dim is None else int(action_dim)
        if self.lo.numel() != n or self.hi.numel() != n:
            raise ValueError(f"ActionBounds: lo and hi must hold {n} values each, got {self.lo.numel()} and {self.hi.numel()}")
        if bool((self.lo > self.hi).any()):
            raise ValueError("ActionBounds: lo must not exceed hi in any dimension")
        self.action_dim = n
        self._on: Dict[torch.device, Tuple[torch.Tensor, torch.Tensor]] = {}

    @classmethod
    def from_statistics(cls, min, max, margin: float = 0.0, action_dim: int = None):  # noqa: A002 -- the statistics' own names
        """From the dataset's per-dimension action statistics: [min - margin * (max - min), max + margin * (max - min)]."""
        margin = float(margin)
        if not math.isfinite(margin) or margin < 0:
            raise ValueError(f"ActionBounds.from_statistics: margin must be finite and >= 0, got {margin}")
        lo, hi = _host_vector(min, "min"), _host_vector(max, "max")
        if lo.numel() != hi.numel():
            raise ValueError(f"ActionBounds.from_statistics: min and max hold {lo.numel()} and {hi.numel()} values")
        pad = (hi - lo) * margin if margin else torch.zeros_like(lo)
        return cls(lo - pad, hi + pad, action_dim=action_dim)

    def clip_bounds(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lo, hi) as fp32 (action_dim,) tensors on ``device``, created on first use and kept."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = (self.lo.to(device), self.hi.to(device))
        return self._on[device]

    def clip_output(self, x: torch.Tensor) -> torch.Tensor:
        lo, hi = self.clip_bounds(x.device)
        return torch.clamp(x, lo, hi)

    def __repr__(self):
        return f"ActionBounds(lo={self.lo.tolist()}, hi={self.hi.tolist()})"
