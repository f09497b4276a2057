"""Perceiver resampler with the reference's constructor, parameter tree and forward signature; the arithmetic
runs in libmdt_hip.so (``mdt_resampler_*`` of include/mdt_resampler.h, gfx950 kernels).

Reference: mdt/models/networks/transformers/perceiver_resampler.py (PerceiverAttentionLayer :11-82,
PerceiverResampler :85-162); built by the agent at mdt/models/mdtv_agent.py:90-97 and called in
``compute_voltron_embeddings`` (:392-404) on the two cameras' Voltron patch tokens,
``(B, 1, 2*196, 384) -> (B, 3, 384)`` = the ``state_images`` tokens of the denoiser.

Differentiable: under autograd the forward keeps a tape in the library handle and the backward (HIP) returns the
gradient of every parameter and of the media tokens, so the module trains inside the agent like the reference's.
There is no eager fallback: CPU tensors or a missing library raise.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .... import _lib
from .._handle import HandleModule
from .utils import feed_forward_layer


class PerceiverAttentionLayer(nn.Module):
    """Parameters of one latent cross-attention layer (reference perceiver_resampler.py:14-30)."""

    def __init__(self, dim: int, dim_head: int = 64, heads: int = 8):
        super().__init__()
        self.scale = dim_head ** -0.5
        self.heads = heads
        self.dim_head = dim_head
        inner_dim = dim_head * heads
        self.norm_media = nn.LayerNorm(dim)
        self.norm_latents = nn.LayerNorm(dim)
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_k = nn.Linear(dim, inner_dim, bias=False)
        self.to_v = nn.Linear(dim, inner_dim, bias=False)
        self.to_out = nn.Linear(inner_dim, dim, bias=False)

    def forward(self, features, latents):  # pragma: no cover - guard
        raise RuntimeError("PerceiverAttentionLayer is a parameter container; call the owning PerceiverResampler")


class PerceiverResampler(HandleModule):
    _prefix, _config, _what = "mdt_resampler", _lib.ResamplerConfig, "resampler"
    _no_cpu = ("the Perceiver resampler runs only on a ROCm GPU (hand-written gfx950 kernels); move the module and its "
               "input with .to('cuda') -- there is no CPU execution path")

    def __init__(self, dim: int, depth: int, dim_head: int = 64, heads: int = 8, num_latents: int = 64,
                 num_time_embeds: int = 4, ff_mult: int = 4, activation: str = "gelu", trainable: bool = True):
        super().__init__()
        self.dim = dim
        self.num_queries = num_latents
        self._cfg = dict(dim=dim, depth=depth, dim_head=dim_head, heads=heads, num_latents=num_latents,
                         num_time_embeds=num_time_embeds, ff_mult=int(ff_mult), activation=0)
        if int(ff_mult) != ff_mult:
            raise NotImplementedError("ff_mult must be an integer")
        self.latents = nn.Parameter(torch.randn(num_latents, dim))
        self.time_pos_emb = nn.Parameter(torch.randn(num_time_embeds, 1, dim))
        self.layers = nn.ModuleList([])
        for _ in range(depth):
            self.layers.append(nn.ModuleList([PerceiverAttentionLayer(dim=dim, dim_head=dim_head, heads=heads),
                                              feed_forward_layer(dim=dim, mult=ff_mult, activation=activation)]))
        self.norm = nn.LayerNorm(dim)
        self._update_trainable_state(trainable)
        self._init_handle()

    def _update_trainable_state(self, trainable: bool = True):
        for param in self.parameters():
            param.requires_grad = trainable

    def _launch(self, lib, x, mask, stream, tape=None):
        B, T, n, dim = x.shape
        out = torch.empty((B, self.num_queries, dim), device=x.device, dtype=torch.float32)
        m = None if mask is None else mask.data_ptr()
        if tape is None:
            _lib.check(lib.mdt_resampler_forward(self._handle, x.data_ptr(), m, B, T, n, out.data_ptr(), stream))
        else:
            _lib.check(lib.mdt_resampler_forward_train(self._handle, x.data_ptr(), m, B, T, n, out.data_ptr(), tape, stream))
        return out

    # -- reference API -----------------------------------------------------------------------------
    def forward(self, x_f: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_f (batch, n_frames, n_features, dim), mask (batch, n_frames) bool -> (batch, num_latents, dim)
        (reference perceiver_resampler.py:124-162)."""
        assert x_f.ndim == 4
        batch_size, max_length, n_features, dim = x_f.shape
        assert dim == self.dim
        m = None
        if mask is not None:
            m = mask.to(device=x_f.device, dtype=torch.bool).reshape(batch_size, max_length).contiguous().view(torch.uint8)
        return self._run(x_f, m)

    def flops(self, n_frames: int, n_features: int) -> float:
        """Algorithmic FLOPs of one forward per sample (needs a live handle, i.e. a previous forward)."""
        if self._handle is None:
            raise RuntimeError("call forward() once first")
        return float(_lib.load().mdt_resampler_flops(self._handle, int(n_frames), int(n_features)))
