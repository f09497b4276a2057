"""The cases, float64 references and bounds behind tests/test_gpu_mae_ops_bounds.py (the ops of include/mdt_mae.h
between guard bands) and tests/test_cpu_mae_ops_reference.py (the same bounds shown to hold the reference and to refuse a
planted defect); importable without a device.  DESIGN.md section 20 has the table of what each case is for.

Every *_case() returns a Case: inp, the fp32 operands by name; want[op][output], a Want (the float64 value and the bound it is
held to); bad[op][output], the float64 value of the same op with ONE defect planted, which at least one Want of that op must
refuse.  Row-op inputs have magnitudes in [0.5, 1.5] and random signs (tests/test_gpu_narrow_ops.py): a dropped, doubled or
misplaced row moves a result by a quarter at least.

Bounds.  Where the same op already has a tolerance in tests/test_mae.py / tests/test_mae_long.py, that one is used.  New ones:
  * dx of the norms at D = 1 and on clamped rows: the kernels form  v = g dy / n - x k + res,  k = (sum_j g_j dy_j x_j) / (D n^3)
    (k = 0, n = eps on a clamped row).  Roundings, from k_rms_bwd / k_sr_rms_bwd: the sum of squares and the dot are 8 fma per
    lane and 6 butterfly adds (14 each); n = sqrt(ss) * rsqrt(D) adds sqrt, rsqrt (2 ulp) and a product: n is within 11 u;
    n^3 and D n^3 three more products (36 u); the quotient 1; x k 1; g dy 1; g dy / n 1 + 11; the two sums 2.  Counting every
    term at the largest of these, |error| <= 64 u (|g dy| / n + |x| sum_j |g_j dy_j x_j| / (D n^3) + |res| + |dx before|),
    u = 2^-24 (ROUNDINGS = 64).  d_z = gamma d_x has one more; d_gamma = sum_rows d_x z adds the rows of a slice and the slices.
  * 12 N(0,1) attention inputs: the same formula evaluated in fp32 torch on the host; the kernel may be FACTOR = 4 times as
    far from float64 as that, as max |error| / max |reference| per output (5 for the long backward, see LONG_BWD_FACTOR)."""
import types

import torch

from oracle import mae_oracle as O
from tests.envelope_configs import MAE_MID_LDS_BUDGET, mae_mid_lds_bytes
from tests.helpers import ATOL, RTOL
from tests.test_mae_long import _ref as attn_ref

U = 2.0 ** -24
ROUNDINGS = 64
FACTOR = 4
LONG_BWD_FACTOR = 5   # measured 4.73 at hd = 64, T = 65: the long backward rebuilds P = 2^(s' - lse log2 e) from an
#                       lse that was rounded to fp32 on its way through memory and is rounded again by the product with log2 e --
#                       two roundings at the magnitude of the logits (up to 800 in base 2) that the host's fp32 softmax does not have
EPS = 1e-8

# ---------------------------------------------------------------------------------------------------------------- tables
RMS_D, RMS_M = [1, 3, 63, 64, 65, 500, 512], [1, 4, 5]
RMS_FLAG_SHAPES = [(5, 65), (4, 512)]
RMS_FLAGS = [(1, 0, False), (0, 1, False), (1, 1, False), (0, 0, True)]        # accumulate_dx, accumulate_dg, dg = NULL
SWIGLU = [(1, 1), (5, 3), (1, 64), (5, 255)]
SR_D, SR_M = [4, 252, 256, 260, 344, 516, 1024], [1, 63, 64, 65]
SRN_D, SRN_M = [4, 252, 256, 260, 500, 512], [1, 3, 64, 65]
CLAMP_D = [(65, 68), (260, 260)]     # (k_rms_*, k_sr_rms_*: D % 4 == 0): one lane loop trip and a bit, and past 64 groups of 4
HEAD_DIMS = [16, 24, 32, 48, 64]
MID_T, MID_B, MID_H = [1, 15, 16, 17, 33, 113], 3, 2
MID_LDS_EDGE = [(2, 2, 64, 80), (2, 2, 48, 96), (2, 3, 64, 128), (2, 2, 48, 128)]   # the last two: the backward is refused
MID_HEAD_WALK = (1024, 2, 16, 17)
LONG_T, LONG_B, LONG_H = [1, 63, 64, 65, 129], 2, 2
HARD_KINDS = ["big", "q0", "onehot"]
HARD_MID_T, HARD_LONG_T, HARD_HD = [17, 113], [65, 129], [24, 64]
PATCH = [(1, 1, 1, 4, 4), (2, 2, 3, 8, 4), (1, 2, 3, 16, 8), (3, 1, 1, 32, 16), (2, 1, 1, 36, 12), (5, 2, 1, 48, 4), (9, 1, 1, 48, 4)]
PATCH_MASKS = ["random", "ones", "one"]
PATCH_G = -2.5


def strides(D):
    """Four different row strides, every one a multiple of 4: (ld_qkv, ld_out, ld_do, ld_dqkv)."""
    return 3 * D + 4, D + 4, D + 8, 3 * D + 12


def mid_backward_fits(hd, T):
    return mae_mid_lds_bytes(hd, T, True) <= MAE_MID_LDS_BUDGET


def seeded(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def draw(g, *shape):
    """Magnitudes in [0.5, 1.5], random signs."""
    return (0.5 + torch.rand(*shape, generator=g)) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)


# ---------------------------------------------------------------------------------------------------------------- bounds
class Want:
    """A float64 value and its bound: rtol / atol as tests.helpers.assert_close, `bound` a tensor of absolute bounds, or
    `fp32` -- the same formula evaluated in fp32 -- with the factor the kernel may be further from `value` than that."""

    def __init__(self, value, rtol=RTOL, atol=ATOL, bound=None, fp32=None, factor=FACTOR):
        self.value = value.detach().double()
        self.rtol, self.atol, self.bound, self.factor = rtol, atol, bound, factor
        self.fp32_err = None if fp32 is None else self.rel_err(fp32)

    def rel_err(self, got):
        return float((got.detach().double().cpu().reshape(self.value.shape) - self.value).abs().max()) / float(self.value.abs().max())

    def outside(self, got):
        """None, or a text that names the worst element."""
        got = got.detach().double().cpu().reshape(self.value.shape)
        if bool(got.isnan().any()):
            return f"NaN at {tuple(int(v) for v in got.isnan().nonzero()[0])}"
        if self.fp32_err is not None:
            e = self.rel_err(got)
            return None if e <= self.factor * self.fp32_err else \
                f"max error / max magnitude {e:.3g}, fp32 on the host {self.fp32_err:.3g}: ratio {e / self.fp32_err:.2f} > {self.factor}"
        err = (got - self.value).abs()
        tol = self.bound if self.bound is not None else self.atol + self.rtol * self.value.abs()
        excess = err - tol
        if not bool((excess > 0).any()):
            return None
        i = int(excess.argmax())
        return (f"{int((excess > 0).sum())}/{err.numel()} outside; worst at flat index {i}: got {float(got.flatten()[i])!r}, want "
                f"{float(self.value.flatten()[i])!r}, allowed {float((tol if torch.is_tensor(tol) else torch.tensor(tol)).expand_as(err).flatten()[i]):.3g}")


def Case(inp, want, bad, **extra):
    return types.SimpleNamespace(inp=inp, want=want, bad=bad, **extra)


def _leaf(t):
    return t.double().requires_grad_()


# ---------------------------------------------------------------------------------------------------------------- norms
def clamped_rows(g, D):
    """Five rows: 0 all zeros, 2 of 1e-12 N(0,1), 4 of 1e-25 N(0,1) (its sum of squares underflows in fp32), 1 and 3 ordinary."""
    x = draw(g, 5, D)
    x[0] = 0.0
    x[2] = 1e-12 * torch.randn(D, generator=g)
    x[4] = 1e-25 * torch.randn(D, generator=g)
    raw = x.double().norm(dim=-1) * D ** -0.5
    assert bool(((raw > 4 * EPS) | (raw < EPS / 4)).all()), "a row sits within a factor 4 of the clamp"
    assert (raw < EPS).tolist() == [True, False, True, False, True]
    return x


def _norm_terms(x, g, dy):
    """sum of the absolute terms of the norm's backward per element (float64), as the kernels form it."""
    D = x.shape[-1]
    raw = x.norm(dim=-1, keepdim=True) * D ** -0.5
    n = raw.clamp(min=EPS)
    gd = (g * dy).abs()
    second = x.abs() * (gd * x.abs()).sum(-1, keepdim=True) / (D * n ** 3)
    return gd / n + torch.where(raw < EPS, torch.zeros_like(second), second)


def _wrong_clamp(x, g):
    """The defect `clamp taken on the wrong side`: x / min(norm, eps) * g."""
    norm = x.norm(dim=-1, keepdim=True) * x.shape[-1] ** -0.5
    return x / norm.clamp(max=EPS) * g


def _unclamped_dx(x, g, dy):
    """The same defect in the backward: the clamped-row branch never taken (n = the raw norm, k as on an ordinary row)."""
    D = x.shape[-1]
    n = x.norm(dim=-1, keepdim=True) * D ** -0.5
    return g * dy / n - x * (g * dy * x).sum(-1, keepdim=True) / (D * n ** 3)


def _dg_tol(M):
    return dict(rtol=1e-3, atol=1e-4 * max(1.0, (M / 64) ** 0.5))      # tests/test_mae.py


def rms_case(M, D, flags=(0, 0, False), clamped=False):
    """mdt_op_rms_fwd, _bwd and _bwd_res on (M, D); flags = (accumulate_dx, accumulate_dg, dg = NULL) of _bwd."""
    acc_dx, acc_dg, no_dg = flags
    g = seeded("rms", M, D, int(clamped))
    x = clamped_rows(g, D) if clamped else draw(g, M, D)
    inp = dict(x=x, g=1.0 + 0.1 * torch.randn(D, generator=g), dy=draw(g, M, D), d_res=draw(g, M, D), dx0=draw(g, M, D),
               dg0=draw(g, 1, D)[0])
    x64, g64 = _leaf(inp["x"]), _leaf(inp["g"])
    y = O.rms_norm(x64, g64, EPS)
    y.backward(inp["dy"].double())
    dx, dg = x64.grad, g64.grad
    derived = D == 1 or clamped
    terms = _norm_terms(x64.detach(), g64.detach(), inp["dy"].double())
    dx_w = dx + acc_dx * inp["dx0"].double()
    dxr_w = dx + inp["d_res"].double()
    want = {"rms_fwd": {"out": Want(y)},
            "rms_bwd": {"dx": Want(dx_w, bound=ROUNDINGS * U * (terms + acc_dx * inp["dx0"].double().abs()) if derived else None)},
            "rms_bwd_res": {"dx": Want(dxr_w, bound=ROUNDINGS * U * (terms + inp["d_res"].double().abs()) if derived else None)}}
    dg_last = dg - (inp["dy"].double() * x64.detach() / (x64.detach().norm(dim=-1, keepdim=True) * D ** -0.5).clamp(min=EPS))[-1]
    bad = {"rms_fwd": {"out": _wrong_clamp(x64.detach(), g64.detach())},
           "rms_bwd": {"dx": dx_w, "dg": dg_last + acc_dg * inp["dg0"].double()},
           "rms_bwd_res": {"dx": dxr_w, "dg": dg_last}}
    if not no_dg:
        want["rms_bwd"]["dg"] = Want(dg + acc_dg * inp["dg0"].double(), **_dg_tol(M))
    else:
        bad["rms_bwd"] = {"dx": dx_w - terms}      # (no dg to drop a row from: a dx without its first term instead)
    want["rms_bwd_res"]["dg"] = Want(dg, **_dg_tol(M))
    if clamped:      # (the last row is a clamped one and adds 1e-17 to dg: the defect here is the clamp's)
        wrong = _unclamped_dx(x64.detach(), g64.detach(), inp["dy"].double())
        bad["rms_bwd"]["dx"], bad["rms_bwd_res"]["dx"] = wrong, wrong + inp["d_res"].double()
    return Case(inp, want, bad, M=M, D=D, flags=flags)


def swiglu_case(M, H):
    g = seeded("swiglu", M, H)
    u = draw(g, M, 2 * H)
    u[0::2, H] = 30.0                      # silu saturates: silu(30) = 30, silu(-30) = -2.8e-12
    u[1::2, H] = -30.0
    if H > 1:
        u[0::2, 2 * H - 1] = -30.0
        u[1::2, 2 * H - 1] = 30.0
    inp = dict(u=u, d_out=draw(g, M, H))
    u64 = _leaf(u)
    p, gt = u64.tensor_split(2, dim=-1)
    out = p * torch.nn.functional.silu(gt)
    out.backward(inp["d_out"].double())
    du = u64.grad.clone()
    u64.grad = None
    (u64.tensor_split(2, dim=-1)[0] * torch.nn.functional.silu(u64.tensor_split(2, dim=-1)[1])).sum().backward()
    swapped = (gt * torch.nn.functional.silu(p)).detach()
    return Case(inp, {"swiglu_fwd": {"out": Want(out)}, "swiglu_bwd": {"du": Want(du)}},
                {"swiglu_fwd": {"out": swapped}, "swiglu_bwd": {"du": u64.grad}}, M=M, H=H)   # halves swapped; d_out ignored


def scale_residual_case(M, D):
    g = seeded("scale_residual", M, D)
    inp = dict(x=draw(g, M, D), z=draw(g, M, D), gamma=draw(g, 1, D)[0], g=draw(g, M, D))
    x, z, gamma, gr = (inp[k].double() for k in ("x", "z", "gamma", "g"))
    out, dz, dgamma = x + gamma * z, gamma * gr, (gr * z).sum(0)
    out_bad = out.clone()
    out_bad[-1] = x[-1]
    want = {"scale_residual_fwd": {"out": Want(out)},
            "scale_residual_bwd": {"dz": Want(dz), "dgamma": Want(dgamma, rtol=1e-3, atol=1e-4 * float(dgamma.abs().max()))}}
    bad = {"scale_residual_fwd": {"out": out_bad}, "scale_residual_bwd": {"dz": dz, "dgamma": dgamma - gr[-1] * z[-1]}}
    return Case(inp, want, bad, M=M, D=D)


def srn_case(M, D, with_res=True, clamped=False):
    """mdt_op_scale_residual_rms_fwd on (x, z, gamma, g_norm) and _bwd on the fp32 x_new of the float64 forward."""
    g = seeded("srn", M, D, int(clamped))
    x = clamped_rows(g, D) if clamped else draw(g, M, D)
    z = draw(g, M, D)
    inp = dict(x=x, z=z, gamma=0.3 * draw(g, 1, D)[0], g_norm=1.0 + 0.1 * torch.randn(D, generator=g), d_h=draw(g, M, D),
               d_res=draw(g, M, D))
    if clamped:
        inp["z_fwd"] = z.clone()
        inp["z_fwd"][0::2] = 0.0            # the forward's x_new = x on the rows that are to be clamped
    zf = inp.get("z_fwd", z).double()
    gam, gn, dh, dr = (inp[k].double() for k in ("gamma", "g_norm", "d_h", "d_res"))
    xn = x.double() + gam * zf
    inp["x_new"] = xn.float()
    h = O.rms_norm(xn, gn, EPS)
    xn64, gn64 = _leaf(inp["x_new"]), _leaf(inp["g_norm"])
    O.rms_norm(xn64, gn64, EPS).backward(dh)
    res = dr if with_res else torch.zeros_like(dr)
    d_x = xn64.grad + res
    d_z, d_gamma, d_gnorm = gam * d_x, (d_x * z.double()).sum(0), gn64.grad
    terms = _norm_terms(xn64.detach(), gn, dh) + res.abs()
    slices = -(-M // 64)
    b_dx = ROUNDINGS * U * terms if clamped else None
    b_dz = (ROUNDINGS + 1) * U * gam.abs() * terms if clamped else None
    b_dgam = (ROUNDINGS + 64 + slices + 8) * U * (terms * z.double().abs()).sum(0) if clamped else None
    want = {"scale_residual_rms_fwd": {"x_new": Want(xn), "h": Want(h)},
            "scale_residual_rms_bwd": {"d_x": Want(d_x, bound=b_dx), "d_z": Want(d_z, bound=b_dz),
                                       "d_gamma": Want(d_gamma, bound=b_dgam, **_dg_tol(M)), "d_gnorm": Want(d_gnorm, **_dg_tol(M))}}
    n_last = (xn64.detach()[-1].norm() * D ** -0.5).clamp(min=EPS)
    bad = {"scale_residual_rms_fwd": {"x_new": xn, "h": _wrong_clamp(xn, gn)},
           "scale_residual_rms_bwd": {"d_x": d_x, "d_z": d_z, "d_gamma": d_gamma - d_x[-1] * z.double()[-1],
                                      "d_gnorm": d_gnorm - dh[-1] * xn64.detach()[-1] / n_last}}
    if clamped:
        bad["scale_residual_rms_bwd"]["d_x"] = _unclamped_dx(xn64.detach(), gn, dh) + res
    return Case(inp, want, bad, M=M, D=D, with_res=with_res)


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_inputs(kind, B, H, hd, T):
    """normal: N(0,1).  big: 12 N(0,1), logits of standard deviation near 140.  q0: q = 0, uniform rows.  onehot: every query of a
    head is the same vector u and key 0 of every sample is 20 u: one-hot rows."""
    D = H * hd
    g = seeded("attn", kind, B, H, hd, T)
    qkv = torch.randn(B, T, 3 * D, generator=g)
    if kind == "big":
        qkv *= 12.0
    elif kind == "q0":
        qkv[..., :D] = 0.0
    elif kind == "onehot":
        u = torch.randn(D, generator=g)
        qkv[..., :D] = u
        qkv[..., D:2 * D] *= 0.1
        qkv[:, 0, D:2 * D] = 20.0 * u
    return qkv, torch.randn(B, T, D, generator=g)


def _attn_with_key_T(qkv, H, hd, scale):
    """The defect `key T included`: every row's softmax runs over one more key and value, the row that follows the sample's last
    in memory (the next sample's first; the first sample's for the last)."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    k = torch.cat([k, k.roll(-1, 0)[:, :, :1]], dim=2)
    v = torch.cat([v, v.roll(-1, 0)[:, :, :1]], dim=2)
    s = q @ k.transpose(-1, -2) * scale
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D), s.logsumexp(-1)


def _d_out_at_the_wrong_stride(do, ld_do, ld_out):
    """The defect `d_out read at the wrong stride`: row r taken at r * ld_out of the buffer whose rows are ld_do apart (pads 0)."""
    B, T, D = do.shape
    buf = torch.zeros(B * T, ld_do, dtype=do.dtype)
    buf[:, :D] = do.reshape(B * T, D)
    flat = buf.flatten()
    return torch.stack([flat[r * ld_out:r * ld_out + D] for r in range(B * T)]).reshape(B, T, D)


def attn_case(op, kind, B, H, hd, T, backward=True):
    """op: "attn_mid" or "attn_long" (the second has lse among the forward's outputs)."""
    D = H * hd
    scale = hd ** -0.5
    qkv, do = attn_inputs(kind, B, H, hd, T)
    q64 = _leaf(qkv)
    out, lse = attn_ref(q64, H, hd, scale)
    fp32 = {}
    if kind == "big":
        q32 = qkv.clone().requires_grad_()
        o32, l32 = attn_ref(q32, H, hd, scale)
        o32.backward(do)
        fp32 = {"out": o32.detach(), "lse": l32.detach(), "d_qkv": q32.grad}
    fwd, bwd = op + "_fwd", op + "_bwd"
    want = {fwd: {"out": Want(out, fp32=fp32.get("out"))}}
    o_bad, l_bad = _attn_with_key_T(qkv.double(), H, hd, scale)
    bad = {fwd: {"out": o_bad}}
    if op == "attn_long":
        want[fwd]["lse"] = Want(lse, fp32=fp32.get("lse"))
        bad[fwd]["lse"] = l_bad
    if backward:
        out.backward(do.double(), retain_graph=True)
        want[bwd] = {"d_qkv": Want(q64.grad.clone(), rtol=1e-3, atol=1e-4, fp32=fp32.get("d_qkv"),
                                   factor=LONG_BWD_FACTOR if op == "attn_long" else FACTOR)}
        q64.grad = None
        _, ld_out, ld_do, _ = strides(D)
        out.backward(_d_out_at_the_wrong_stride(do.double(), ld_do, ld_out))
        bad[bwd] = {"d_qkv": q64.grad}
    return Case(dict(qkv=qkv, d_out=do), want, bad, B=B, H=H, hd=hd, T=T, scale=scale, kind=kind)


# ---------------------------------------------------------------------------------------------------------------- patch loss
def patch_case(B, X, C_, R, P, mask_kind):
    gs = R // P
    n, E = gs * gs, P * P * C_
    g = seeded("patch", B, X, C_, R, P, mask_kind)
    rec, imgs = torch.randn(B, X, n, E, generator=g), torch.randn(B, X, C_, R, R, generator=g)
    if mask_kind == "ones":
        mask = torch.ones(B, n)
    elif mask_kind == "one":
        mask = torch.zeros(B, n)
        mask[-1, -1] = 1.0
    else:
        mask = (torch.rand(B, n, generator=g) < 0.5).float()
        mask[0, 0] = 1.0
    patches = imgs.double().reshape(B, X, C_, gs, P, gs, P).permute(0, 1, 3, 5, 4, 6, 2).reshape(B, X, n, E)   # test_patch_loss_op
    r64, m64 = _leaf(rec), mask.double()
    per_patch = ((r64 - patches) ** 2).mean(-1)
    loss = sum((per_patch[:, x] * m64).sum() / m64.sum() for x in range(X)) / X
    loss.backward()
    d_unit = r64.grad
    last = (m64[:, None, :].expand(B, X, n).reshape(-1) != 0).nonzero()[-1]          # the last partial that is not zero
    loss_bad = loss.detach() - per_patch.detach().reshape(-1)[last].sum() / m64.sum() / X
    both = lambda a, b: torch.stack([a.reshape(()), b.reshape(())]).reshape(1, 2)   # noqa: E731
    want = {"patch_mse_fwd": {"loss_and_mask_sum": Want(both(loss.detach(), m64.sum()), rtol=1e-5, atol=1e-6)},
            "patch_mse_bwd": {"d_rec": Want(PATCH_G * d_unit, rtol=1e-4, atol=1e-8)}}
    bad = {"patch_mse_fwd": {"loss_and_mask_sum": both(loss_bad, m64.sum())}, "patch_mse_bwd": {"d_rec": d_unit}}
    return Case(dict(rec=rec.reshape(B * X * n, E), imgs=imgs.reshape(B * X * C_ * R, R), mask=mask, g=torch.tensor([[PATCH_G]])),
                want, bad, B=B, X=X, C_=C_, R=R, P=P, n=n, E=E, mask_sum=float(m64.sum()))


# ---------------------------------------------------------------------------------------------------------------- the list
def all_cases():
    """(id, builder) of every case both test modules walk; the builders are cheap, the head-walk case aside."""
    out = []
    for D in RMS_D:
        for M in RMS_M:
            out.append((f"rms-{M}x{D}", lambda M=M, D=D: rms_case(M, D)))
    for M, D in RMS_FLAG_SHAPES:
        for f in RMS_FLAGS:
            out.append((f"rms-{M}x{D}-flags{f[0]}{f[1]}{int(f[2])}", lambda M=M, D=D, f=f: rms_case(M, D, f)))
    for D, D4 in CLAMP_D:
        out.append((f"rms-clamped-{D}", lambda D=D: rms_case(5, D, clamped=True)))
        out.append((f"srn-clamped-{D4}", lambda D=D4: srn_case(5, D, clamped=True)))
    for M, H in SWIGLU:
        out.append((f"swiglu-{M}x{H}", lambda M=M, H=H: swiglu_case(M, H)))
    for D in SR_D:
        for M in SR_M:
            out.append((f"sr-{M}x{D}", lambda M=M, D=D: scale_residual_case(M, D)))
    for D in SRN_D:
        for M in SRN_M:
            for r in (True, False):
                out.append((f"srn-{M}x{D}-res{int(r)}", lambda M=M, D=D, r=r: srn_case(M, D, r)))
    for hd in HEAD_DIMS:
        for T in MID_T:
            out.append((f"mid-{hd}-{T}", lambda hd=hd, T=T: attn_case("attn_mid", "normal", MID_B, MID_H, hd, T, mid_backward_fits(hd, T))))
        for T in LONG_T:
            out.append((f"long-{hd}-{T}", lambda hd=hd, T=T: attn_case("attn_long", "normal", LONG_B, LONG_H, hd, T)))
    for B, H, hd, T in MID_LDS_EDGE:
        out.append((f"mid-lds-{hd}-{T}", lambda B=B, H=H, hd=hd, T=T: attn_case("attn_mid", "normal", B, H, hd, T, mid_backward_fits(hd, T))))
    B, H, hd, T = MID_HEAD_WALK
    out.append(("mid-head-walk", lambda: attn_case("attn_mid", "normal", B, H, hd, T, backward=False)))
    for kind in HARD_KINDS:
        for hd in HARD_HD:
            for T in HARD_MID_T:
                out.append((f"mid-{kind}-{hd}-{T}", lambda k=kind, hd=hd, T=T: attn_case("attn_mid", k, MID_B, MID_H, hd, T, mid_backward_fits(hd, T))))
            for T in HARD_LONG_T:
                out.append((f"long-{kind}-{hd}-{T}", lambda k=kind, hd=hd, T=T: attn_case("attn_long", k, LONG_B, LONG_H, hd, T)))
    for shape in PATCH:
        for mk in PATCH_MASKS:
            out.append((f"patch-{'x'.join(map(str, shape))}-{mk}", lambda s=shape, mk=mk: patch_case(*s, mk)))
    return out
