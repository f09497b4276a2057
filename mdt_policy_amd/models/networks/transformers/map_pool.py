"""ClipStyleProjection and its MAPBlock pooling head with the reference's constructors, parameter trees and forward
signatures; MAPBlock's arithmetic (forward AND backward) runs in libmdt_hip.so (``mdt_map_pool_*`` of
include/mdt_map_pool.h, gfx950 kernels).

Reference: mdt/models/networks/transformers/transformer_blocks.py -- RMSNorm :43, SwishGLU :55, MAPAttention :718,
MAPBlock :746, ClipStyleProjection :833, MeanPooling :873.  The agent builds ``ClipStyleProjection('map', 384,
clip_token_index=1, num_token=...)`` (mdt/models/mdtv_agent.py:133-138) and pools ``latent_encoder_emb`` of the language
and of the vision goal with it for the contrastive loss (:440-484).

'map' / 'map_state_only' run the HIP MAPBlock.  The other clip styles are index / mean / one small Linear over a
(B, 4, d) tensor -- a slice, a mean and torch's own modules, kept as host PyTorch (none of them is the shipped
configuration).  There is no eager fallback for MAPBlock: CPU tensors or a missing library raise.
"""
from __future__ import annotations

import torch
from torch import nn

from .... import _lib
from .._handle import HandleModule


class RMSNorm(nn.Module):
    """Parameter container (reference transformer_blocks.py:43-51); the arithmetic runs in the owning MAPBlock."""

    def __init__(self, dim: int, eps: float = 1e-8) -> None:
        super().__init__()
        self.scale, self.eps = dim ** -0.5, eps
        self.g = nn.Parameter(torch.ones(dim))


class SwishGLU(nn.Module):
    """Parameter container (reference transformer_blocks.py:55-62)."""

    def __init__(self, in_dim: int, out_dim: int) -> None:
        super().__init__()
        self.act, self.project = nn.SiLU(), nn.Linear(in_dim, 2 * out_dim)


class MAPAttention(nn.Module):
    """Parameter container (reference transformer_blocks.py:718-743)."""

    def __init__(self, embed_dim: int, n_heads: int) -> None:
        super().__init__()
        assert embed_dim % n_heads == 0, "`embed_dim` must be divisible by `n_heads`!"
        self.n_heads, self.scale = n_heads, (embed_dim // n_heads) ** -0.5
        self.q, self.kv = nn.Linear(embed_dim, embed_dim, bias=False), nn.Linear(embed_dim, 2 * embed_dim, bias=False)
        self.proj = nn.Linear(embed_dim, embed_dim)


class MAPBlock(HandleModule):
    """Multiheaded attention pooling block (reference transformer_blocks.py:746-791).  Pools 1 .. 64 tokens per sample, the
    denoiser's own context limit; the library picks the attention kernels by the token count (include/mdt_map_pool.h: up to 16
    tokens a call can exceed the 64 KiB LDS rule of its kernels and raise, from 17 on nothing is refused for LDS)."""

    _prefix, _config, _what = "mdt_map_pool", _lib.MapPoolConfig, "MAPBlock"
    _no_cpu = ("MAPBlock runs only on a ROCm GPU (hand-written gfx950 kernels); move the module and its input with "
               ".to('cuda') -- there is no CPU execution path")

    def __init__(self, n_latents: int, embed_dim: int, n_heads: int, output_dim: None, mlp_ratio: float = 4.0,
                 do_rms_norm: bool = True, do_swish_glu: bool = True) -> None:
        super().__init__()
        if not (do_rms_norm and do_swish_glu):
            raise NotImplementedError("the HIP MAPBlock implements the reference's defaults (RMSNorm + SwishGLU)")
        self.n_latents, self.in_dim, self.n_heads = n_latents, embed_dim, 2 * n_heads
        self.embed_dim = output_dim if output_dim is not None else embed_dim
        self.projection = nn.Linear(embed_dim, self.embed_dim)
        self.latents = nn.Parameter(torch.zeros(self.n_latents, self.embed_dim))
        nn.init.normal_(self.latents, std=0.02)
        self.attn_norm = RMSNorm(self.embed_dim)
        self.attn = MAPAttention(self.embed_dim, n_heads=self.n_heads)
        self.mlp_norm = RMSNorm(self.embed_dim)
        hidden = int(mlp_ratio * self.embed_dim)
        self.mlp = nn.Sequential(SwishGLU(self.embed_dim, hidden), nn.Linear(hidden, self.embed_dim))
        self._cfg = dict(n_latents=n_latents, embed_dim=embed_dim, output_dim=self.embed_dim, n_heads=n_heads,
                         mlp_hidden=hidden)
        self._init_handle()

    def _launch(self, lib, x, _extra, stream, tape=None):
        B, N, _ = x.shape
        out = torch.empty((B, self.n_latents, self.embed_dim), device=x.device, dtype=torch.float32)
        if tape is None:
            _lib.check(lib.mdt_map_pool_forward(self._handle, x.data_ptr(), B, N, out.data_ptr(), stream))
        else:
            _lib.check(lib.mdt_map_pool_forward_train(self._handle, x.data_ptr(), B, N, out.data_ptr(), tape, stream))
        return out

    # -- reference API -----------------------------------------------------------------------------
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, N, embed_dim) -> (B, n_latents, output_dim), squeezed on dim 1 (reference :787-791)."""
        assert x.ndim == 3 and x.shape[-1] == self.in_dim
        return self._run(x).squeeze(dim=1)


class MeanPooling(nn.Module):
    """Mean over the tokens (reference transformer_blocks.py:873-880)."""

    def __init__(self, token_dim):
        super().__init__()
        self.token_dim = token_dim

    def forward(self, x):
        return x.mean(dim=1).view(-1, self.token_dim)


# clip_style -> (pooling kind, drop the goal token first)
_CLIP_STYLES = {
    "map": ("map", False), "map_state_only": ("map", True),
    "mean_pooling": ("mean", False), "mean_pool_state_only": ("mean", True),
    "mlp": ("mlp", False), "single_token": ("token", False), "multihead": ("keep", False),
}


class ClipStyleProjection(nn.Module):
    """Pools the (B, tokens, d) context into the embedding the contrastive loss compares (reference
    transformer_blocks.py:833-870: same constructor, same ``latent_proj`` sub-module per style, same outputs).  'map' and
    'map_state_only' take a context of up to 64 tokens, e.g. the 34 of two cameras x 16 resampler latents, goal and proprio."""

    def __init__(self, clip_style, token_dim=384, clip_token_index=0, num_token=4):
        super().__init__()
        if clip_style not in _CLIP_STYLES:
            raise ValueError("Invalid clip_style. Expected 'map', 'mean_pooling', or 'single_token' or 'multihead'.")
        self.clip_style = clip_style
        self.clip_token_index = clip_token_index
        kind, self._state_only = _CLIP_STYLES[clip_style]
        self._kind = kind
        if kind == "map":
            self.latent_proj = MAPBlock(1, token_dim, 8, output_dim=token_dim)
        elif kind == "mean":
            self.latent_proj = MeanPooling(token_dim)
        elif kind == "mlp":
            self.latent_proj = nn.Sequential(nn.Linear(num_token * token_dim, token_dim), nn.LayerNorm(token_dim), nn.Tanh())
        else:  # one token / all tokens: nothing to learn
            self.latent_proj = nn.Identity()

    def forward(self, x):
        if self._kind == "token":
            x = x[:, self.clip_token_index, :]
        elif self._state_only:
            x = x[:, 1:]
        elif self._kind == "mlp":
            x = x.flatten(1)
        return self.latent_proj(x)
