"""Steered actions: sampling pushed toward known actions through the denoiser's Jacobian.

A pin (utils/action_pin.py) overwrites the prediction element by element, so the tokens that are not pinned learn of the
constraint only through the next step's input.  A steer sends the constraint error back through the denoiser instead
(pseudo-inverse guidance, as real-time chunking uses it): with J = dD/dx,

    e       = weight * (known - D(x; sigma))
    g       = J^T e
    s(sigma) = min(beta, 1 + sigma^2 / sigma_data^2)
    D'(x; sigma) = D + s(sigma) * g

so every element of the chunk moves toward a chunk whose prediction agrees with the known part.  ``e`` is a constant of the step:
no second-order term, no gradient through it.  ``s`` is sigma^2 / r^2 with r^2 = sigma^2 sigma_data^2 / (sigma^2 + sigma_data^2),
clipped at ``beta`` (real-time chunking's clip).  A steer is a triple (``known``, ``weight``, ``beta``), ``known`` and ``weight``
(B, Ta, A), ``weight`` in [0, 1], and it is an argument of the denoiser: every sampler uses D' wherever it used D.

Hand it to a sampler as ``extra_args={"steer": steer}`` (gc_sampling.sample_*: sample_ddim, and sample_euler without churn, stay
one native call, include/mdt_hip_train.h mdt_sample_ddim_steer; the others run their host loops unless the steer was built with
``plan_native=True``, which makes every other fixed-step sampler one native call too, mdt_sample_steer), to
``GCDenoiser.sample_ddim(..., steer=steer)`` or to ``GCDenoiser.forward(..., steer=steer)``.  A steer whose weight is zero
everywhere is no steer: the call is then, bit for bit, the call without it.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from .action_pin import ActionPin


class ActionSteer:
    """``known``: broadcastable to (B, Ta, A), finite.  ``weight``: (Ta,), (B, Ta), (B, Ta, 1) or (B, Ta, A), every value finite
    and in [0, 1].  ``beta``: finite and > 0.  The tensors are checked here, in one reduction (one read-back where they live on
    a device), which also tells whether any weight is non-zero (``active``).  ``plan_native``: whether the fixed-step samplers
    other than sample_ddim and churn-free sample_euler run this steer as one native call (mdt_sample_steer) where they can; the
    default keeps the host loops they have always run under a steer.  It changes where the work runs, not the rule."""

    def __init__(self, known, weight, beta: float = 5.0, plan_native: bool = False):
        beta = float(beta)
        if not math.isfinite(beta) or not beta > 0:
            raise ValueError(f"ActionSteer: beta must be finite and > 0, got {beta}")
        known, weight = torch.as_tensor(known).detach(), torch.as_tensor(weight).detach()
        if weight.dim() == 1:
            weight = weight.reshape(1, -1, 1)
        elif weight.dim() == 2:
            weight = weight.unsqueeze(-1)
        elif weight.dim() != 3:
            raise ValueError(f"ActionSteer: weight must be (Ta,), (B, Ta), (B, Ta, 1) or (B, Ta, A), got {tuple(weight.shape)}")
        if known.dim() > 3:
            raise ValueError(f"ActionSteer: known must be broadcastable to (B, Ta, A), got {tuple(known.shape)}")
        weight, known = weight.to(torch.float32), known.to(torch.float32)
        if weight.numel() < 1:
            raise ValueError("ActionSteer: weight must be finite and lie in [0, 1]")
        # two flags, one read-back (NaN fails both compares): bit 0 = the values are in order, bit 1 = some weight is non-zero
        ok = ((weight >= 0) & (weight <= 1)).all().to(known.device) & torch.isfinite(known).all()
        flags = int(ok.to(torch.int32) + 2 * (weight != 0).any().to(known.device).to(torch.int32))
        if not flags & 1:
            if not bool(((weight >= 0) & (weight <= 1)).all()):
                raise ValueError("ActionSteer: weight must be finite and lie in [0, 1]")
            raise ValueError("ActionSteer: known must be finite")
        self.known, self.weight, self.beta = known, weight, beta
        self.active = bool(flags & 2)
        self.plan_native = bool(plan_native)

    @classmethod
    def overlap(cls, prev_chunk, executed: int, hard: int, soft: int = 0, beta: float = 5.0, plan_native: bool = False):
        """The receding-horizon steer, with ``ActionPin.overlap``'s ramp as the weight: 1 on the first ``hard`` tokens of the new
        chunk, 1 - (j - hard + 1) / (soft + 1) for j in [hard, hard + soft), 0 behind them and wherever ``prev_chunk`` has no value;
        ``known`` is ``prev_chunk`` moved up by ``executed`` tokens."""
        try:
            pin = ActionPin.overlap(prev_chunk, executed, hard, soft)
        except ValueError as exc:
            raise ValueError(str(exc).replace("ActionPin", "ActionSteer")) from None
        return cls(pin.known, pin.keep, beta, plan_native)

    def on(self, device, shape, candidates: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """(known, weight) as contiguous fp32 tensors of ``shape`` = (B, Ta, A) on ``device``.  ``candidates`` = K > 1: the B chunks
        are K per observation (chunk k of observation b is row b*K + k); a steer that fits (B, Ta, A) is per chunk and passes
        through, one that fits (B / K, Ta, A) is per observation and goes to each of that observation's K chunks."""
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3:
            raise ValueError(f"ActionSteer: the action chunk must be (B, Ta, A), got {shape}")
        try:
            known = torch.broadcast_to(self.known.to(device), shape)
            weight = torch.broadcast_to(self.weight.to(device), shape)
        except RuntimeError as exc:
            if candidates > 1 and shape[0] % candidates == 0:
                known, weight = self.on(device, (shape[0] // candidates,) + shape[1:])
                return known.repeat_interleave(candidates, 0), weight.repeat_interleave(candidates, 0)
            raise ValueError(f"ActionSteer: known {tuple(self.known.shape)} / weight {tuple(self.weight.shape)} do not fit an "
                             f"action chunk of {shape}") from exc
        return known.contiguous(), weight.contiguous()

    def scale(self, sigma, sigma_data):
        """s(sigma) = min(beta, 1 + sigma^2 / sigma_data^2): a float for a number, a tensor (per row, no read-back) for a tensor."""
        sigma_data = float(sigma_data)
        if torch.is_tensor(sigma):
            return torch.clamp(1.0 + (sigma * sigma) / (sigma_data * sigma_data), max=self.beta)
        sigma = float(sigma)
        return min(self.beta, 1.0 + sigma * sigma / (sigma_data * sigma_data))

    def error(self, denoised: torch.Tensor, candidates: int = 1) -> torch.Tensor:
        """e = weight * (known - D) of a denoised chunk D, in its dtype: the vector the Jacobian is applied to."""
        known, weight = self.on(denoised.device, denoised.shape, candidates)
        return weight.to(denoised.dtype) * (known.to(denoised.dtype) - denoised)

    def __repr__(self):
        return f"ActionSteer(known={tuple(self.known.shape)}, weight={tuple(self.weight.shape)}, beta={self.beta})"
