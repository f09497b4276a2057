"""Pinned actions: chunk inpainting inside the samplers.

A controller that replans while the previous chunk is still executing needs the new chunk to agree with the part of the old one
that is already committed (receding-horizon execution with overlap, "real-time chunking"); way-point conditioning and "first
action = current pose" are the same operation.  A pin is a pair (``known``, ``keep``), both (B, Ta, A), ``keep`` in [0, 1], and
it is an argument of the denoiser:

    D'(x; sigma) = keep * known + (1 - keep) * D(x; sigma)

``keep == 0`` gives the bits of D, ``keep == 1`` the bits of ``known`` (selects at both ends), anything between
``D + keep * (known - D)`` in fp32; with guidance D is the combined D_lambda.  Every sampler then uses D' wherever it used D.
Under every sampler whose schedule ends at sigma = 0 the elements with ``keep == 1`` arrive at ``known`` to rounding
(sample_dpm_fast and sample_dpm_adaptive stop at sigma_min and arrive within O(sigma_min)); a soft ``keep`` blends the prediction
toward ``known`` at every step.

Hand it to a sampler as ``extra_args={"pin": pin}`` (gc_sampling.sample_*: the native call stays native, include/mdt_hip.h
mdt_sample_opts.pin_known / pin_keep), to ``GCDenoiser.sample_ddim / sample_native(..., pin=pin)`` or to
``GCDenoiser.forward(..., pin=pin)``.  A steer (utils/action_steer.py, ``ActionSteer``) moves the whole chunk instead: it sends the
same error, known - D, back through the denoiser's Jacobian, so the tokens that are not pinned follow the known part.
"""
from __future__ import annotations

from typing import Tuple

import torch


class ActionPin:
    """``known``: broadcastable to (B, Ta, A).  ``keep``: (Ta,), (B, Ta), (B, Ta, 1) or (B, Ta, A), every value finite and in
    [0, 1]; ``known`` must be finite.  Both are checked here, in one reduction (one read-back where
    they live on a device)."""

    def __init__(self, known, keep):
        known, keep = torch.as_tensor(known).detach(), torch.as_tensor(keep).detach()
        if keep.dim() == 1:
            keep = keep.reshape(1, -1, 1)
        elif keep.dim() == 2:
            keep = keep.unsqueeze(-1)
        elif keep.dim() != 3:
            raise ValueError(f"ActionPin: keep must be (Ta,), (B, Ta), (B, Ta, 1) or (B, Ta, A), got {tuple(keep.shape)}")
        if known.dim() > 3:
            raise ValueError(f"ActionPin: known must be broadcastable to (B, Ta, A), got {tuple(known.shape)}")
        keep, known = keep.to(torch.float32), known.to(torch.float32)
        if keep.numel() < 1:
            raise ValueError("ActionPin: keep must be finite and lie in [0, 1]")
        # one flag, one read-back: a replan loop builds a pin from a device chunk at every replan (NaN fails both compares)
        ok = ((keep >= 0) & (keep <= 1)).all().to(known.device) & torch.isfinite(known).all()
        if not bool(ok):
            if not bool(((keep >= 0) & (keep <= 1)).all()):
                raise ValueError("ActionPin: keep must be finite and lie in [0, 1]")
            raise ValueError("ActionPin: known must be finite")
        self.known, self.keep = known, keep

    @classmethod
    def overlap(cls, prev_chunk, executed: int, hard: int, soft: int = 0):
        """The receding-horizon pin: ``executed`` actions of ``prev_chunk`` (B, Ta, A) have run since it was planned, so token j
        of the new chunk is token j + executed of the old one wherever that exists.  ``keep`` is 1 on the first ``hard`` tokens,
        1 - (j - hard + 1) / (soft + 1) for j in [hard, hard + soft), 0 behind them and wherever ``prev_chunk`` has no value."""
        prev = torch.as_tensor(prev_chunk).detach()
        executed, hard, soft = int(executed), int(hard), int(soft)
        if prev.dim() != 3:
            raise ValueError(f"ActionPin.overlap: prev_chunk must be (B, Ta, A), got {tuple(prev.shape)}")
        if executed < 0 or hard < 0 or soft < 0:
            raise ValueError("ActionPin.overlap: executed, hard and soft must be >= 0")
        Ta = prev.shape[1]
        n = max(Ta - executed, 0)  # tokens of the new chunk the old one has a value for
        known = torch.zeros_like(prev, dtype=torch.float32)
        known[:, :n] = prev[:, executed:executed + n]
        keep = torch.zeros(Ta, dtype=torch.float32)
        for j in range(min(n, hard + soft)):
            keep[j] = 1.0 if j < hard else 1.0 - (j - hard + 1) / (soft + 1)
        return cls(known, keep.to(prev.device))

    def on(self, device, shape, candidates: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """(known, keep) as contiguous fp32 tensors of ``shape`` = (B, Ta, A) on ``device``.  ``candidates`` = K > 1: the B chunks
        are K per observation (chunk k of observation b is row b*K + k); a pin that fits (B, Ta, A) is per chunk and passes
        through, one that fits (B / K, Ta, A) is per observation and goes to each of that observation's K chunks."""
        shape = tuple(int(v) for v in shape)
        if len(shape) != 3:
            raise ValueError(f"ActionPin: the action chunk must be (B, Ta, A), got {shape}")
        try:
            known = torch.broadcast_to(self.known.to(device), shape)
            keep = torch.broadcast_to(self.keep.to(device), shape)
        except RuntimeError as exc:
            if candidates > 1 and shape[0] % candidates == 0:
                known, keep = self.on(device, (shape[0] // candidates,) + shape[1:])
                return known.repeat_interleave(candidates, 0), keep.repeat_interleave(candidates, 0)
            raise ValueError(f"ActionPin: known {tuple(self.known.shape)} / keep {tuple(self.keep.shape)} do not fit an action "
                             f"chunk of {shape}") from exc
        return known.contiguous(), keep.contiguous()

    def apply(self, denoised: torch.Tensor, candidates: int = 1) -> torch.Tensor:
        """D' of a denoised chunk D, by the rule above (what GCDenoiser.forward and the host loops compute).  ``candidates``: as
        in ``on``."""
        known, keep = self.on(denoised.device, denoised.shape, candidates)
        known, keep = known.to(denoised.dtype), keep.to(denoised.dtype)
        return torch.where(keep == 0, denoised, torch.where(keep == 1, known, denoised + keep * (known - denoised)))

    def __repr__(self):
        return f"ActionPin(known={tuple(self.known.shape)}, keep={tuple(self.keep.shape)})"
