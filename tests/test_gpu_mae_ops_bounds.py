"""The ops of include/mdt_mae.h -- the masked-image head's training step -- held to their buffers, flags and edges
(pytest -m gpu).  Every pointer of every call lies in a Guarded (tests/guarded.py): inputs must come back
intact and unchanged, outputs start as NaN and must be written completely and nowhere else, outputs a call must not touch hold
the canary, accumulating outputs start as random values, scratch / partial / lse have exactly the stated size.  Every call runs
a second time on dense torch tensors and must give the same bits.  Values go against the float64 references of
tests/mae_ops_cases.py at the tolerance the op has in tests/test_mae.py / tests/test_mae_long.py; the derived bounds of that
module hold dx at D = 1, the clamped rows and the 12 N(0,1) attention inputs.  tests/test_cpu_mae_ops_reference.py shows on the
host that every one of those bounds refuses a planted defect."""
import pytest
import torch

from tests import mae_ops_cases as K
from tests.guarded import NAN, GuardedSet, canary, same_bits
from tests.test_gpu_ops import stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from mdt_policy_amd import _lib
    return _lib


class Ops:
    """The operands of one call, twice: between guard bands (row stride ld) and as dense torch tensors."""

    def __init__(self):
        self.gs, self.g, self.d, self.outs, self.free = GuardedSet(), {}, {}, [], set()

    def inp(self, name, t, ld=None):
        t = t.reshape(1, -1) if t.dim() == 1 else t
        self.g[name], self.d[name] = self.gs.inp(name, t, ld), t.contiguous().cuda()

    def out(self, name, rows, cols, ld=None, fill=None, untouched=False):
        """fill None: NaN, the call has to write all of it; untouched: the canary, the call must leave it."""
        fill = canary(rows, cols) if untouched else fill
        self.g[name] = self.gs.out(name, rows, cols, ld, fill=fill)
        self.d[name] = (torch.full((rows, cols), NAN) if fill is None else fill.reshape(rows, cols).clone()).cuda()
        self.outs.append(name)
        if untouched:
            self.free.add(name)

    def call(self, f, dense=False, off=None, ld_off=None):
        """f(p, ld) with p(name, floats=0) -> address and ld(name) -> row stride; off / ld_off: bytes / floats added to one."""
        off, ld_off = off or {}, ld_off or {}

        def p(name, floats=0):
            base = self.d[name].data_ptr() if dense else self.g[name].ptr
            return base + 4 * floats + off.get(name, 0)

        def ld(name):
            return (self.d[name].shape[1] if dense else self.g[name].ld) + ld_off.get(name, 0)
        return f(p, ld)

    def run(self, L, f, what):
        """The call between the guard bands, then on the dense tensors; every check of the module's rules."""
        L.check(self.call(f))
        L.check(self.call(f, dense=True))
        torch.cuda.synchronize()
        self.gs.check(what)
        for name in self.outs:
            if name in self.free:
                assert self.g[name].keeps(), f"{what}: {name} was touched"
            else:
                self.g[name].check(f"{what}: output {name}", written=True)
            assert same_bits(self.g[name].region, self.d[name]), f"{what}: {name} differs between the guarded and the dense call"

    def refused(self, L, f, what, status=None, text=None, **kw):
        st = self.call(f, **kw)
        torch.cuda.synchronize()
        assert st != 0 if status is None else st == status, (what, st, L.load().mdt_last_error())
        if text:
            assert text in L.load().mdt_last_error().decode(), (what, L.load().mdt_last_error())
        self.gs.check(what)
        for name in self.outs:
            assert self.g[name].keeps(), f"{what}: refused, yet {name} was written"

    def got(self, name):
        return self.g[name].host()


def expect(case, op, o, names=None):
    for name, w in case.want[op].items():
        if names is None or name in names:
            msg = w.outside(o.got(name))
            assert msg is None, f"{op} {name}: {msg}"


# ---------------------------------------------------------------------------------------------------------------- norms
def rms_fwd(L, c):
    lib, i = L.load(), c.inp
    o = Ops()
    o.inp("x", i["x"]), o.inp("g", i["g"])
    o.out("out", c.M, c.D)
    o.run(L, lambda p, ld: lib.mdt_op_rms_fwd(p("x"), p("g"), p("out"), c.M, c.D, K.EPS, stream()), "rms_fwd")
    expect(c, "rms_fwd", o)


def rms_bwd(L, c, res=False, acc_dg=None):
    """mdt_op_rms_bwd with the case's flags, or (res) mdt_op_rms_bwd_res with accumulate_dg = acc_dg; returns the operands."""
    lib, i, (M, D) = L.load(), c.inp, (c.M, c.D)
    acc_dx, adg, no_dg = (0, acc_dg, False) if res else c.flags
    n = lib.mdt_op_rms_bwd_scratch(M, D)
    assert n == -(-M // 4) * D
    o = Ops()
    for k in ("x", "g", "dy") + (("d_res",) if res else ()):
        o.inp(k, i[k])
    o.out("dx", M, D, fill=i["dx0"] if acc_dx else None)
    o.out("dg", 1, D, fill=i["dg0"] if adg else None, untouched=no_dg)
    o.out("scratch", 1, n)
    if res:
        f = lambda p, ld: lib.mdt_op_rms_bwd_res(p("x"), p("g"), p("dy"), p("d_res"), p("dx"), p("dg"), adg, M, D, K.EPS,  # noqa: E731
                                                 p("scratch"), stream())
    else:
        f = lambda p, ld: lib.mdt_op_rms_bwd(p("x"), p("g"), p("dy"), p("dx"), acc_dx, None if no_dg else p("dg"), adg, M, D,  # noqa: E731
                                             K.EPS, p("scratch"), stream())
    o.run(L, f, "rms_bwd_res" if res else "rms_bwd")
    return o


def run_rms(L, c):
    rms_fwd(L, c)
    o = rms_bwd(L, c)
    expect(c, "rms_bwd", o)
    if c.flags != (0, 0, False):
        return
    for acc_dg in (0, 1):
        r = rms_bwd(L, c, res=True, acc_dg=acc_dg)
        expect(c, "rms_bwd_res", r, {"dx"})
        assert torch.equal(r.g["dx"].region, o.g["dx"].region + c.inp["d_res"].cuda()), "dx is not the bits of _bwd + d_res"
        w = c.want["rms_bwd_res"]["dg"]
        msg = K.Want(w.value + acc_dg * c.inp["dg0"].double(), rtol=w.rtol, atol=w.atol).outside(r.got("dg"))
        assert msg is None, f"rms_bwd_res dg, accumulate_dg = {acc_dg}: {msg}"
        if not acc_dg:
            assert same_bits(r.g["dg"].region, o.g["dg"].region)


@pytest.mark.parametrize("M", K.RMS_M)
@pytest.mark.parametrize("D", K.RMS_D)
def test_rmsnorm_forward_backward_and_residual_form(L, M, D):
    """D = 1 and 3 (one lane), 63 / 64 / 65 (a second trip of the lane loop), 500 (D % 64 != 0), 512 (the limit); M = 1, 4, 5: a
    workgroup of four rows short, full, and one row into the next.  dx at D = 1 is exactly zero: the derived bound."""
    run_rms(L, K.rms_case(M, D))


@pytest.mark.parametrize("flags", K.RMS_FLAGS)
@pytest.mark.parametrize("M,D", K.RMS_FLAG_SHAPES)
def test_rmsnorm_backward_flags(L, M, D, flags):
    """accumulate_dx, accumulate_dg, both (the outputs start as random values), and dg = NULL (dx right, dg's canary kept)."""
    run_rms(L, K.rms_case(M, D, flags))


def srn_fwd(L, c):
    lib, i, (M, D) = L.load(), c.inp, (c.M, c.D)
    o = Ops()
    o.inp("x", i["x"]), o.inp("z", i.get("z_fwd", i["z"])), o.inp("gamma", i["gamma"]), o.inp("g_norm", i["g_norm"])
    o.out("x_new", M, D), o.out("h", M, D)
    o.run(L, lambda p, ld: lib.mdt_op_scale_residual_rms_fwd(p("x"), p("z"), p("gamma"), p("g_norm"), p("x_new"), p("h"), M, D,
                                                             K.EPS, stream()), "scale_residual_rms_fwd")
    expect(c, "scale_residual_rms_fwd", o)
    alone = torch.full((M, D), NAN, device="cuda")
    L.check(lib.mdt_op_scale_residual_fwd(o.d["x"].data_ptr(), o.d["z"].data_ptr(), o.d["gamma"].data_ptr(), alone.data_ptr(), M, D,
                                          stream()))
    assert same_bits(o.g["x_new"].region, alone), "x_new is not the bits of mdt_op_scale_residual_fwd"


def srn_bwd(L, c):
    lib, i, (M, D) = L.load(), c.inp, (c.M, c.D)
    n = lib.mdt_op_scale_residual_rms_bwd_scratch(M, D)
    assert n == 2 * -(-M // 64) * D
    o = Ops()
    for k in ("x_new", "g_norm", "d_h", "z", "gamma") + (("d_res",) if c.with_res else ()):
        o.inp(k, i[k])
    o.out("d_x", M, D), o.out("d_z", M, D), o.out("d_gamma", 1, D), o.out("d_gnorm", 1, D), o.out("scratch", 1, n)
    o.run(L, lambda p, ld: lib.mdt_op_scale_residual_rms_bwd(
        p("x_new"), p("g_norm"), p("d_h"), p("d_res") if c.with_res else None, p("z"), p("gamma"), p("d_x"), p("d_z"), p("d_gamma"),
        p("d_gnorm"), M, D, K.EPS, p("scratch"), stream()), "scale_residual_rms_bwd")
    expect(c, "scale_residual_rms_bwd", o)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("M", K.SRN_M)
@pytest.mark.parametrize("D", K.SRN_D)
def test_scale_residual_with_the_next_norm(L, M, D, with_res):
    """D / 4 = 1, 63, 64, 65 (the second column group of a lane begins), 125, 128 (the limit); M = 1, 3 (one workgroup of four rows,
    short), 64 / 65 (one slice of the backward full, a second begun); d_res given and NULL."""
    c = K.srn_case(M, D, with_res)
    if with_res:
        srn_fwd(L, c)
    srn_bwd(L, c)


@pytest.mark.parametrize("D,D4", K.CLAMP_D)
def test_clamped_rows_in_all_four_norm_kernels(L, D, D4):
    """Rows of zeros, of 1e-12 and of 1e-25 (the sum of squares underflows) among ordinary ones, eps = 1e-8: the branch
    `clamped ? eps : raw`, k = 0 of k_rms_fwd / k_rms_bwd / k_sr_rms_fwd / k_sr_rms_bwd against float64 autograd of
    x / norm.clamp(min=eps) * g; the gradients of order 1e8 at the derived bound."""
    run_rms(L, K.rms_case(5, D, clamped=True))
    c = K.srn_case(5, D4, clamped=True)
    srn_fwd(L, c)
    srn_bwd(L, c)


# ---------------------------------------------------------------------------------------------------------------- SwishGLU, LayerScale
@pytest.mark.parametrize("M,H", K.SWIGLU)
def test_swiglu(L, M, H):
    """One element, an odd width, one wave, and 5 x 255 = 1275 elements: five 256-thread blocks whose borders fall inside rows;
    gates of +-30, where silu saturates."""
    lib, c = L.load(), K.swiglu_case(M, H)
    o = Ops()
    o.inp("u", c.inp["u"])
    o.out("out", M, H)
    o.run(L, lambda p, ld: lib.mdt_op_swiglu_fwd(p("u"), p("out"), M, H, stream()), "swiglu_fwd")
    expect(c, "swiglu_fwd", o)
    o = Ops()
    o.inp("u", c.inp["u"]), o.inp("d_out", c.inp["d_out"])
    o.out("du", M, 2 * H)
    o.run(L, lambda p, ld: lib.mdt_op_swiglu_bwd(p("u"), p("d_out"), p("du"), M, H, stream()), "swiglu_bwd")
    expect(c, "swiglu_bwd", o)


@pytest.mark.parametrize("M", K.SR_M)
@pytest.mark.parametrize("D", K.SR_D)
def test_scale_residual(L, M, D):
    """D / 4 = 1, 63, 64, 65, 86 (256 / 86 = 2 row lanes, 84 idle threads), 129 (one row lane, 127 idle), 256 (the limit); M = 1,
    63 / 64 / 65 around the 64 rows of a workgroup.  dgamma is overwritten: it starts as NaN."""
    lib, c = L.load(), K.scale_residual_case(M, D)
    o = Ops()
    o.inp("x", c.inp["x"]), o.inp("z", c.inp["z"]), o.inp("gamma", c.inp["gamma"])
    o.out("out", M, D)
    o.run(L, lambda p, ld: lib.mdt_op_scale_residual_fwd(p("x"), p("z"), p("gamma"), p("out"), M, D, stream()), "scale_residual_fwd")
    expect(c, "scale_residual_fwd", o)
    n = lib.mdt_op_scale_residual_bwd_scratch(M, D)
    assert n == -(-M // 64) * D
    o = Ops()
    o.inp("g", c.inp["g"]), o.inp("z", c.inp["z"]), o.inp("gamma", c.inp["gamma"])
    o.out("dz", M, D), o.out("dgamma", 1, D), o.out("scratch", 1, n)
    o.run(L, lambda p, ld: lib.mdt_op_scale_residual_bwd(p("g"), p("z"), p("gamma"), p("dz"), p("dgamma"), M, D, p("scratch"), stream()),
          "scale_residual_bwd")
    expect(c, "scale_residual_bwd", o)


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_ops(L, c, op, backward=True, show=None):
    """Forward and (where the case has one) backward of "attn_mid" / "attn_long" on four different padded strides."""
    lib = L.load()
    B, H, hd, T, scale = c.B, c.H, c.hd, c.T, c.scale
    D = H * hd
    ld_qkv, ld_out, ld_do, ld_dqkv = K.strides(D)
    long = op == "attn_long"
    qkv = c.inp["qkv"].reshape(B * T, 3 * D)
    o = Ops()
    o.inp("qkv", qkv, ld_qkv)
    o.out("out", B * T, D, ld_out)
    if long:
        o.out("lse", 1, B * H * T)
        f = lambda p, ld: lib.mdt_op_attn_long_fwd(p("qkv"), ld("qkv"), p("out"), ld("out"), p("lse"), B, H, hd, T, scale, stream())  # noqa: E731
    else:
        f = lambda p, ld: lib.mdt_op_attn_mid_fwd(p("qkv"), ld("qkv"), p("out"), ld("out"), B, H, hd, T, scale, stream())  # noqa: E731
    o.run(L, f, op + "_fwd")
    if show is not None:
        show(op + "_fwd", c, o)
    expect(c, op + "_fwd", o)
    if not backward:
        return o
    fits = long or K.mid_backward_fits(hd, T)
    assert fits == (op + "_bwd" in c.want)
    b = Ops()
    b.inp("qkv", qkv, ld_qkv), b.inp("out", o.got("out"), ld_out), b.inp("d_out", c.inp["d_out"].reshape(B * T, D), ld_do)
    b.out("d_qkv", B * T, 3 * D, ld_dqkv, untouched=not fits)
    if not fits:   # the header's LDS rule: refused, nothing launched, d_qkv keeps its canary
        b.refused(L, lambda p, ld: lib.mdt_op_attn_mid_bwd(p("qkv"), ld("qkv"), p("out"), ld("out"), p("d_out"), ld("d_out"), p("d_qkv"),
                                                           ld("d_qkv"), B, H, hd, T, scale, stream()), "mid backward past its LDS", 2,
                  "does not fit LDS")
        return o
    if long:
        n = lib.mdt_op_attn_long_bwd_scratch(B, H, T)
        assert n == B * H * T
        b.inp("lse", o.got("lse")), b.out("scratch", 1, n)
        f = lambda p, ld: lib.mdt_op_attn_long_bwd(p("qkv"), ld("qkv"), p("out"), ld("out"), p("lse"), p("d_out"), ld("d_out"),  # noqa: E731
                                                   p("d_qkv"), ld("d_qkv"), B, H, hd, T, scale, p("scratch"), stream())
    else:
        f = lambda p, ld: lib.mdt_op_attn_mid_bwd(p("qkv"), ld("qkv"), p("out"), ld("out"), p("d_out"), ld("d_out"), p("d_qkv"),  # noqa: E731
                                                  ld("d_qkv"), B, H, hd, T, scale, stream())
    b.run(L, f, op + "_bwd")
    if show is not None:
        show(op + "_bwd", c, b)
    expect(c, op + "_bwd", b)
    return o


@pytest.mark.parametrize("T", K.MID_T)
@pytest.mark.parametrize("hd", K.HEAD_DIMS)
def test_attention_mid_on_four_different_strides(L, hd, T):
    """Every head dim (both forward forms, both backward forms) x T = 1, 15 / 16 / 17 around one tile of 16, 33 (three tiles,
    the last of one row) and 113 (eight tiles: the 512-thread forward); ld_qkv, ld_out, ld_do and ld_dqkv all different, so a
    kernel that took one for another reads or writes a pad column.  (hd = 48 and 64 at T = 113: the backward does not fit its
    LDS and must refuse with d_qkv untouched.)"""
    attn_ops(L, K.attn_case("attn_mid", "normal", K.MID_B, K.MID_H, hd, T, K.mid_backward_fits(hd, T)), "attn_mid")


@pytest.mark.parametrize("B,H,hd,T", K.MID_LDS_EDGE)
def test_attention_mid_at_the_last_shapes_its_lds_holds(L, B, H, hd, T):
    """The last shapes the backward's LDS holds, and the last the forward's does, whose backward is refused with d_qkv untouched."""
    assert [K.mid_backward_fits(hd, T), K.mid_backward_fits(hd, T + 1)] in ([True, False], [False, False])
    attn_ops(L, K.attn_case("attn_mid", "normal", B, H, hd, T, K.mid_backward_fits(hd, T)), "attn_mid")


def test_attention_mid_forward_walks_both_heads_in_one_workgroup(L):
    """B = 1024, H = 2: the forward's second form runs both heads of a sample in one workgroup (hpw = 2; the first head's output
    waits in registers while the second's rows are committed); T = 17: the second tile holds one row."""
    B, H, hd, T = K.MID_HEAD_WALK
    attn_ops(L, K.attn_case("attn_mid", "normal", B, H, hd, T, backward=False), "attn_mid", backward=False)


@pytest.mark.parametrize("T", K.LONG_T)
@pytest.mark.parametrize("hd", K.HEAD_DIMS)
def test_attention_long_on_four_different_strides(L, hd, T):
    """T = 1, 63 / 64 / 65 around one stage of 64 keys and one block of 64 queries, 129 (three of each, the last of one row);
    lse of exactly B H T floats, scratch of exactly mdt_op_attn_long_bwd_scratch floats."""
    attn_ops(L, K.attn_case("attn_long", "normal", K.LONG_B, K.LONG_H, hd, T), "attn_long")


def show_ratio(op, c, o):
    for name, w in c.want[op].items():
        if w.fp32_err is not None:
            e = w.rel_err(o.got(name))
            print(f"{op} hd={c.hd} T={c.T} {name}: kernel {e:.3g}, fp32 on the host {w.fp32_err:.3g}, ratio {e / w.fp32_err:.2f}")


@pytest.mark.parametrize("kind", K.HARD_KINDS)
@pytest.mark.parametrize("T", K.HARD_MID_T)
@pytest.mark.parametrize("hd", K.HARD_HD)
def test_attention_mid_hard_softmax_inputs(L, hd, T, kind):
    """12 N(0,1): logits of standard deviation near 140 -- exp overflows unless the row maximum is subtracted; q = 0: uniform
    rows; key 0 = 20 x every query: one-hot rows.  (hd = 64, T = 113: the backward does not fit its LDS; forward only.)"""
    attn_ops(L, K.attn_case("attn_mid", kind, K.MID_B, K.MID_H, hd, T, K.mid_backward_fits(hd, T)), "attn_mid", show=show_ratio)


@pytest.mark.parametrize("kind", K.HARD_KINDS)
@pytest.mark.parametrize("T", K.HARD_LONG_T)
@pytest.mark.parametrize("hd", K.HARD_HD)
def test_attention_long_hard_softmax_inputs(L, hd, T, kind):
    """The same inputs through the online softmax: a running maximum that starts at -inf and jumps by hundreds between stages
    (alpha = 2^(old - new) underflows to 0), base-2 exponents of logits of order 100, and the lse that carries them backward."""
    attn_ops(L, K.attn_case("attn_long", kind, K.LONG_B, K.LONG_H, hd, T), "attn_long", show=show_ratio)


# ---------------------------------------------------------------------------------------------------------------- patch loss
def patch_ops(c):
    o = Ops()
    o.inp("rec", c.inp["rec"]), o.inp("imgs", c.inp["imgs"]), o.inp("mask", c.inp["mask"])
    return o


def patch_fwd_call(lib, c):
    return lambda p, ld: lib.mdt_op_patch_mse_fwd(p("rec"), p("imgs"), p("mask"), p("partial"), p("loss_and_mask_sum"),
                                                  p("loss_and_mask_sum", 1), c.B, c.X, c.C_, c.R, c.P, stream())


def patch_bwd_call(lib, c):
    return lambda p, ld: lib.mdt_op_patch_mse_bwd(p("rec"), p("imgs"), p("mask"), p("loss_and_mask_sum", 1), p("g"), p("d_rec"),
                                                  c.B, c.X, c.C_, c.R, c.P, stream())


@pytest.mark.parametrize("mask_kind", K.PATCH_MASKS)
@pytest.mark.parametrize("B,X,C_,R,P", K.PATCH)
def test_patch_loss(L, B, X, C_, R, P, mask_kind):
    """Patches of 16, 48 and 144 elements (less than one wave, less than one trip of 256 threads), grids of 1, 2, 3 and 12 patches
    a side, 1440 partials and 1296 mask entries (both loops of the reduction take a second trip); random, all-ones and single-one
    masks; an incoming gradient of -2.5; loss and mask_sum side by side as the Python mirror lays them."""
    lib, c = L.load(), K.patch_case(B, X, C_, R, P, mask_kind)
    o = patch_ops(c)
    o.out("partial", 1, B * X * c.n), o.out("loss_and_mask_sum", 1, 2)
    o.run(L, patch_fwd_call(lib, c), "patch_mse_fwd")
    expect(c, "patch_mse_fwd", o)
    assert float(o.got("loss_and_mask_sum")[0, 1]) == c.mask_sum
    b = patch_ops(c)
    b.inp("loss_and_mask_sum", o.got("loss_and_mask_sum")), b.inp("g", c.inp["g"])
    b.out("d_rec", B * X * c.n, c.E)
    b.run(L, patch_bwd_call(lib, c), "patch_mse_bwd")
    expect(c, "patch_mse_bwd", b)
    visible = (c.inp["mask"] == 0)[:, None, :, None].expand(B, X, c.n, c.E).reshape(B * X * c.n, c.E)
    assert bool((b.got("d_rec")[visible] == 0).all()), "d_rec is not exactly zero on a visible patch"


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_row_ops_refuse_one_bad_argument_at_a_time(L):
    """A pointer 4 bytes off, D % 4, D above the limit: status MDT_ERR_INVALID_ARG, every output keeps its canary; then the
    legal call on fresh operands is right (the tests above run after this one in any order: each builds its own)."""
    lib = L.load()
    M, D = 3, 8
    c = K.scale_residual_case(M, D)
    o = Ops()
    o.inp("x", c.inp["x"]), o.inp("z", c.inp["z"]), o.inp("gamma", c.inp["gamma"])
    o.out("out", M, D, untouched=True)
    f = lambda D_: lambda p, ld: lib.mdt_op_scale_residual_fwd(p("x"), p("z"), p("gamma"), p("out"), M, D_, stream())  # noqa: E731
    for name in ("x", "z", "gamma", "out"):
        o.refused(L, f(D), f"scale_residual_fwd, {name} + 4", 1, "aligned", off={name: 4})
    for bad in (6, 1028, 0):
        o.refused(L, f(bad), f"scale_residual_fwd, D = {bad}", 1, "multiple of 4")
    n = lib.mdt_op_scale_residual_bwd_scratch(M, D)
    o = Ops()
    o.inp("g", c.inp["g"]), o.inp("z", c.inp["z"]), o.inp("gamma", c.inp["gamma"])
    o.out("dz", M, D, untouched=True), o.out("dgamma", 1, D, untouched=True), o.out("scratch", 1, n, untouched=True)
    f = lambda D_: lambda p, ld: lib.mdt_op_scale_residual_bwd(p("g"), p("z"), p("gamma"), p("dz"), p("dgamma"), M, D_,  # noqa: E731
                                                               p("scratch"), stream())
    for name in ("g", "z", "gamma", "dz", "scratch"):
        o.refused(L, f(D), f"scale_residual_bwd, {name} + 4", 1, "aligned", off={name: 4})
    for bad in (6, 1028):
        o.refused(L, f(bad), f"scale_residual_bwd, D = {bad}", 1, "multiple of 4")
    s = K.srn_case(M, D)
    o = Ops()
    o.inp("x", s.inp["x"]), o.inp("z", s.inp["z"]), o.inp("gamma", s.inp["gamma"]), o.inp("g_norm", s.inp["g_norm"])
    o.out("x_new", M, D, untouched=True), o.out("h", M, D, untouched=True)
    f = lambda D_: lambda p, ld: lib.mdt_op_scale_residual_rms_fwd(p("x"), p("z"), p("gamma"), p("g_norm"), p("x_new"), p("h"), M,  # noqa: E731
                                                                   D_, K.EPS, stream())
    for name in ("x", "z", "gamma", "g_norm", "x_new", "h"):
        o.refused(L, f(D), f"scale_residual_rms_fwd, {name} + 4", 1, "aligned", off={name: 4})
    for bad in (6, 516):
        o.refused(L, f(bad), f"scale_residual_rms_fwd, D = {bad}", 1, "multiple of 4")
    n = lib.mdt_op_scale_residual_rms_bwd_scratch(M, D)
    o = Ops()
    for k in ("x_new", "g_norm", "d_h", "d_res", "z", "gamma"):
        o.inp(k, s.inp[k])
    for k, rows in (("d_x", M), ("d_z", M), ("d_gamma", 1), ("d_gnorm", 1)):
        o.out(k, rows, D, untouched=True)
    o.out("scratch", 1, n, untouched=True)
    f = lambda D_: lambda p, ld: lib.mdt_op_scale_residual_rms_bwd(  # noqa: E731
        p("x_new"), p("g_norm"), p("d_h"), p("d_res"), p("z"), p("gamma"), p("d_x"), p("d_z"), p("d_gamma"), p("d_gnorm"), M, D_, K.EPS,
        p("scratch"), stream())
    for name in ("x_new", "g_norm", "d_h", "d_res", "z", "gamma", "d_x", "d_z", "scratch"):
        o.refused(L, f(D), f"scale_residual_rms_bwd, {name} + 4", 1, "aligned", off={name: 4})
    for bad in (6, 516):
        o.refused(L, f(bad), f"scale_residual_rms_bwd, D = {bad}", 1, "multiple of 4")
    r = K.rms_case(M, D)
    o = Ops()
    o.inp("x", r.inp["x"]), o.inp("g", r.inp["g"]), o.inp("dy", r.inp["dy"])
    o.out("out", M, D, untouched=True), o.out("dg", 1, D, untouched=True), o.out("scratch", 1, lib.mdt_op_rms_bwd_scratch(M, D), untouched=True)
    o.refused(L, lambda p, ld: lib.mdt_op_rms_fwd(p("x"), p("g"), p("out"), M, 513, K.EPS, stream()), "rms_fwd, D = 513", 1, "D <= 512")
    o.refused(L, lambda p, ld: lib.mdt_op_rms_bwd(p("x"), p("g"), p("dy"), p("out"), 0, p("dg"), 0, M, 513, K.EPS, p("scratch"), stream()),
              "rms_bwd, D = 513", 1, "D <= 512")
    # the next legal call of every op refused above
    run_rms(L, r)
    srn_fwd(L, s), srn_bwd(L, s)
    test_scale_residual(L, M, D)


@pytest.mark.parametrize("op", ["attn_mid", "attn_long"])
def test_attention_refuses_one_bad_argument_at_a_time(L, op):
    """A pointer 4 bytes off, a stride that is no multiple of 4, T above the limit, a foreign head dim, and the first shapes past
    the mid backward's LDS: non-zero status, out / lse / d_qkv / scratch keep their canaries; then the legal call is right."""
    lib = L.load()
    B, H, hd, T = 2, 2, 24, 17
    long = op == "attn_long"
    c = K.attn_case(op, "normal", B, H, hd, T)
    D = H * hd
    ld_qkv, ld_out, ld_do, ld_dqkv = K.strides(D)
    o = Ops()
    o.inp("qkv", c.inp["qkv"].reshape(B * T, 3 * D), ld_qkv), o.inp("fwd_out", c.want[op + "_fwd"]["out"].value.float().reshape(B * T, D), ld_out)
    o.inp("d_out", c.inp["d_out"].reshape(B * T, D), ld_do), o.inp("fwd_lse", torch.zeros(1, B * H * T))
    o.out("out", B * T, D, ld_out, untouched=True), o.out("d_qkv", B * T, 3 * D, ld_dqkv, untouched=True)
    o.out("lse", 1, B * H * T, untouched=True), o.out("scratch", 1, B * H * T, untouched=True)

    def fwd(hd_=hd, T_=T):
        if long:
            return lambda p, ld: lib.mdt_op_attn_long_fwd(p("qkv"), ld("qkv"), p("out"), ld("out"), p("lse"), B, H, hd_, T_, c.scale, stream())
        return lambda p, ld: lib.mdt_op_attn_mid_fwd(p("qkv"), ld("qkv"), p("out"), ld("out"), B, H, hd_, T_, c.scale, stream())

    def bwd(hd_=hd, T_=T):
        if long:
            return lambda p, ld: lib.mdt_op_attn_long_bwd(p("qkv"), ld("qkv"), p("fwd_out"), ld("fwd_out"), p("fwd_lse"), p("d_out"),
                                                          ld("d_out"), p("d_qkv"), ld("d_qkv"), B, H, hd_, T_, c.scale, p("scratch"), stream())
        return lambda p, ld: lib.mdt_op_attn_mid_bwd(p("qkv"), ld("qkv"), p("fwd_out"), ld("fwd_out"), p("d_out"), ld("d_out"),
                                                     p("d_qkv"), ld("d_qkv"), B, H, hd_, T_, c.scale, stream())
    for name in ("qkv", "out"):
        o.refused(L, fwd(), f"{op}_fwd, {name} + 4", 1, "aligned", off={name: 4})
        o.refused(L, fwd(), f"{op}_fwd, ld_{name} + 2", 1, "multiples of 4", ld_off={name: 2})
    for name in ("qkv", "fwd_out", "d_out", "d_qkv"):
        o.refused(L, bwd(), f"{op}_bwd, {name} + 4", 1, "aligned", off={name: 4})
        o.refused(L, bwd(), f"{op}_bwd, ld_{name} + 2", 1, "multiples of 4", ld_off={name: 2})
    limit = 4096 if long else 128
    for call, what in ((fwd, "fwd"), (bwd, "bwd")):
        o.refused(L, call(T_=limit + 1), f"{op}_{what}, T = {limit + 1}", 2, f"T must be <= {limit}")
        o.refused(L, call(hd_=12), f"{op}_{what}, head dim 12", 2, "head dim 12")
        o.refused(L, call(T_=0), f"{op}_{what}, T = 0", 1)
    if not long:
        for hd_, T_ in ((64, 81), (48, 97)):
            o.refused(L, bwd(hd_, T_), f"attn_mid_bwd, hd = {hd_}, T = {T_}", 2, "does not fit LDS")
    attn_ops(L, c, op)


def test_patch_loss_refuses_a_resolution_its_patches_do_not_divide(L):
    lib = L.load()
    c = K.patch_case(2, 2, 3, 8, 4, "random")
    o = patch_ops(c)
    o.inp("g", c.inp["g"])
    o.out("partial", 1, c.B * c.X * c.n, untouched=True), o.out("loss_and_mask_sum", 1, 2, untouched=True)
    o.out("d_rec", c.B * c.X * c.n, c.E, untouched=True)
    for R, P in ((10, 4), (4, 8), (8, 0)):
        c.R, c.P = R, P
        o.refused(L, patch_fwd_call(lib, c), f"patch_mse_fwd, R = {R}, P = {P}", 1)
        o.refused(L, patch_bwd_call(lib, c), f"patch_mse_bwd, R = {R}, P = {P}", 1)
    test_patch_loss(L, 2, 2, 3, 8, 4, "random")
