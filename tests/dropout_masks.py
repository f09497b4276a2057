"""The library's train-mode dropout masks, restated in numpy -- TEST INFRASTRUCTURE.

The masks of a training forward are counter based and therefore replayable exactly (include/mdt_hip_train.h: mdt_dropout;
csrc/mdt_device.h: philox4, dropout_keep, dropout_scale):

    words    = Philox4x32-10(counter = (element >> 2 lo, element >> 2 hi, site, 0x9e3779b9), key = (seed lo, seed hi))
    keep     = float32(words[element & 3] >> 8) * 2^-24 >= float32(p)          (exact in fp32: no borderline element)
    multiply = keep ? 1 / (1 - p) : 0;       p <= 0 or seed == 0: 1 everywhere

Nothing here reads the library: the site numbering and the element indices are written out again from the documented contract,
so a test that compares a kernel with these masks fails when either side leaves the contract."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4(seed, site, ctr):
    """The library's philox4(seed, site, ctr) (csrc/mdt_device.h) in uint64 arithmetic: Philox4x32-10 with counter
    (ctr lo, ctr hi, site, 0x9e3779b9) and key (seed lo, seed hi).  ``site`` and ``ctr`` may be arrays (broadcast)."""
    site, ctr = np.broadcast_arrays(np.asarray(site, dtype=np.uint64), np.asarray(ctr, dtype=np.uint64))
    seed = np.uint64(seed)
    c0 = ctr & M32
    c1 = ctr >> _S32
    c2 = site & M32
    c3 = np.full(site.shape, 0x9E3779B9, dtype=np.uint64)
    k0, k1 = seed & M32, seed >> _S32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> _S32) ^ c1 ^ k0
        n2 = (p0 >> _S32) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def words(seed, site, idx):
    """The 32-bit word of every element index in ``idx`` (any shape): word idx & 3 of block idx >> 2."""
    idx = np.asarray(idx, dtype=np.uint64)
    flat = idx.reshape(-1)
    blocks, inverse = np.unique(flat >> np.uint64(2), return_inverse=True)
    w = np.stack(philox4(seed, np.uint64(site), blocks), axis=1)              # (n_blocks, 4)
    return w[inverse.reshape(-1), (flat & np.uint64(3)).astype(np.int64)].reshape(idx.shape)


def scale(seed, site, shape_or_indices, p):
    """dropout_scale of the library for a whole site: float64 array of 0 / 1 / (1 - float32(p)).  ``shape_or_indices``: a
    shape (tuple / int: the elements 0 .. prod - 1 in C order) or an integer array of element indices."""
    if isinstance(shape_or_indices, (tuple, list, int, np.integer)):
        shape = (int(shape_or_indices),) if isinstance(shape_or_indices, (int, np.integer)) else tuple(int(s) for s in shape_or_indices)
        idx = None
    else:
        idx = np.asarray(shape_or_indices, dtype=np.uint64)
        shape = idx.shape
    p32 = np.float32(p)
    if p32 <= 0 or int(seed) == 0:
        return np.ones(shape, dtype=np.float64)
    if idx is None:   # a whole site: block after block, no gather
        n = int(np.prod(shape, dtype=np.int64))
        blocks = np.arange((n + 3) // 4, dtype=np.uint64)
        w = np.stack(philox4(seed, np.uint64(site), blocks), axis=1).reshape(-1)[:n].reshape(shape)
    else:
        w = words(seed, site, idx)
    u = (w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)   # 24-bit grid: exact in fp32
    return np.where(u >= p32, 1.0 / (1.0 - np.float64(p32)), 0.0)


# Restated from csrc/mdt_train.hip ("dropout sites: one id per (block, place)", the two enums and site_id below them):
# blocks are numbered encoder first, then decoder; the two embedding dropouts are places 0 / 1 of the pseudo block Le + Ld.
ATTN, RESID, MLP, XATTN, XRESID = 0, 1, 2, 3, 4
EMBED_CTX, EMBED_ACTION = 0, 1
PLACES = {"attn": ATTN, "resid": RESID, "mlp": MLP, "xattn": XATTN, "xresid": XRESID}


def site_id(block, place):
    return block * 8 + place + 1


class Masks:
    """The multipliers of one train-mode forward, per place, in the oracle's layout (float64 torch tensors on the CPU).
    ``block`` counts encoder blocks first, then decoder blocks (decoder block l is Le + l).  Element indices as documented in
    include/mdt_hip_train.h: attention ((b H + h) Tq + i) Tk + j, merges row * D + column, embeddings the flat index of the
    (B * rows, D) array with the rows below ``drop_lo`` of every sample left alone."""

    def __init__(self, seed, Le, Ld, H, D, attn_p, resid_p, mlp_p, embed_p=0.0):
        self.seed, self.Le, self.Ld, self.H, self.D = int(seed), Le, Ld, H, D
        self.attn_p, self.resid_p, self.mlp_p, self.embed_p = attn_p, resid_p, mlp_p, embed_p

    def _t(self, site, shape, p):
        return torch.from_numpy(scale(self.seed, site, shape, p))

    def attn(self, block, B, Tq, Tk):
        return self._t(site_id(block, ATTN), (B, self.H, Tq, Tk), self.attn_p)

    def xattn(self, block, B, Tq, Tk):
        return self._t(site_id(block, XATTN), (B, self.H, Tq, Tk), self.attn_p)

    def resid(self, block, B, T):
        return self._t(site_id(block, RESID), (B, T, self.D), self.resid_p)

    def xresid(self, block, B, T):
        return self._t(site_id(block, XRESID), (B, T, self.D), self.resid_p)

    def mlp(self, block, B, T):
        return self._t(site_id(block, MLP), (B, T, self.D), self.mlp_p)

    def embed_ctx(self, B, Te, drop_lo):
        m = self._t(site_id(self.Le + self.Ld, EMBED_CTX), (B, Te, self.D), self.embed_p)
        m[:, :drop_lo] = 1.0
        return m

    def embed_action(self, B, Ta):
        return self._t(site_id(self.Le + self.Ld, EMBED_ACTION), (B, Ta, self.D), self.embed_p)

    @classmethod
    def of(cls, seed, cfg):
        """From a score-network configuration (the keys of mdt_policy_amd.configs)."""
        return cls(seed, cfg["n_enc_layers"], cfg["n_dec_layers"], cfg["n_heads"], cfg["embed_dim"], cfg["attn_pdrop"],
                   cfg["resid_pdrop"], cfg["mlp_pdrop"], cfg.get("embed_pdrob", 0.0))
