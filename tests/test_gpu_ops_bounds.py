"""Every kernel-level op of include/mdt_hip_ops.h held to its buffers (pytest -m gpu).

Each call runs twice on the same values: once with every pointer inside a tests/guarded.py Guarded -- guard bands in front and
behind, the smallest legal pad on every row stride (+4 floats where the op wants a multiple of 4, else +1), pad columns and gaps
filled with the guard NaN -- and once on dense, unguarded torch tensors.  Asserted for every call:
  (a) the valid region against a float64 reference, at the tolerance the op has in tests/test_gpu_ops.py;
  (b) the valid region bit for bit against the dense call (no dispatch rule reads a stride beyond its alignment);
  (c) every output intact() and without a NaN where the call had to write;
  (d) every input intact() and with the bits it started with;
  (e) rows a row remap skips keep the canary.
Shapes are the smallest that reach each path: rows one off each row-tile height, columns 16 past each tile width."""
import ctypes as C
import functools
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests.guarded import NAN, GuardedSet, bits, canary, same_bits
from tests.helpers import assert_close
from tests.test_gpu_f16_pair import expected_pack_pair
from tests.test_gpu_ops import expected_pack, expected_pack_split, ref_attn, ref_mlp, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


class Dense:
    """The unguarded twin of a Guarded: the same values in a dense torch tensor."""

    def __init__(self, rows, cols, fill=None, slabs=1, ld=None):
        ld = ld or cols   # (ld > cols: a stride that belongs to the call itself, such as sigma_stride; NaN between the values)
        shape = (rows, ld) if slabs == 1 else (slabs, rows, ld)
        t = torch.full(shape, NAN)
        if torch.is_tensor(fill):
            t[..., :cols] = fill.to(torch.float32).reshape(shape[:-1] + (cols,))
        elif fill is not None:
            t[..., :cols] = float(fill)
        self.buf = t.cuda()
        self.rows, self.cols, self.ld, self.slab_stride, self.ptr = rows, cols, ld, rows * ld, self.buf.data_ptr()

    @property
    def region(self):
        return self.buf[..., :self.cols]

    def host(self):
        return self.region.cpu()

    def at(self, row=0, col=0):
        return self.ptr + 4 * (row * self.ld + col)

    def check(self, what, written=False, unchanged=False):
        pass


class Lay:
    """The operands of one call: guarded with padded strides, or dense (pads and gaps dropped)."""

    def __init__(self, guarded):
        self.guarded, self.set, self.dense = guarded, GuardedSet(), []

    def inp(self, name, t, pad=0, gap=0, fixed=False):
        """(cols,), (rows, cols) or (slabs, rows, cols) input; pad: extra floats of row stride, gap: extra floats between slabs;
        fixed: the stride is the call's own (sigma_stride), so the dense twin keeps it."""
        t = t.reshape(1, -1) if t.dim() == 1 else t
        rows, cols = t.shape[-2:]
        if self.guarded:
            return self.set.inp(name, t, cols + pad, (rows * (cols + pad) + gap) if t.dim() == 3 else None)
        self.dense.append(Dense(rows, cols, t, t.shape[0] if t.dim() == 3 else 1, ld=cols + pad if fixed else None))
        return self.dense[-1]

    def image(self, name, flat):
        """A packed weight image (no stride: guards only), as rows of up to 256 floats."""
        flat = flat.reshape(-1)
        flat = flat if flat.dtype == torch.float32 else flat.contiguous().view(torch.float32)
        return self.inp(name, flat.reshape(-1, math.gcd(flat.numel(), 256)))

    def out(self, name, rows, cols, pad=0, fill=None, slabs=1, gap=0):
        if self.guarded:
            return self.set.out(name, rows, cols, cols + pad, fill, slabs, (rows * (cols + pad) + gap) if slabs > 1 else None)
        self.dense.append(Dense(rows, cols, fill, slabs))
        return self.dense[-1]

    def check(self, what):
        torch.cuda.synchronize()
        self.set.check(what)


def ptr(o):
    return None if o is None else o.ptr


def seeded(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + (k if isinstance(k, int) else sum(map(ord, str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def act_fn(name):
    return {"none": lambda v: v, "gelu": F.gelu, "mish": F.mish, "silu": F.silu}[name]


# the tolerances of tests/test_gpu_ops.py
TOL_GEMM = dict(rtol=1e-4, atol=1e-4)          # test_gemm_plain_bias, test_gemm_every_geometry, the tall / weight-stationary bodies
TOL_LN = dict(rtol=2e-4, atol=2e-4)            # test_gemm_layernorm_modulate_prologue, test_gemm_small_m_kernel_...
TOL_AUX2 = dict(rtol=1e-4, atol=2e-4)          # aux_mode 2 in the tall / weight-stationary tests; TOL_ACT of test_gpu_linear_bwd.py
TOL_MLP = dict(rtol=2e-4, atol=2e-4)           # test_fused_mlp_slabs_sum_to_the_sublayer and its split form
TOL_ATTN = dict(rtol=1e-4, atol=1e-5)          # test_attention
TOL_ATTN_PROJ = dict(rtol=1e-4, atol=2e-5)     # test_attention_fused_into_projection_per_sample and the wide form
TOL_XATTN = dict(rtol=2e-4, atol=2e-4)         # test_collapsed_cross_attention and the launches built on it
TOL_XATTN_FC = dict(rtol=2e-4, atol=3e-4)      # c_fc in test_cross_attention_inside_the_linear_that_follows_it
TOL_LAYERNORM = dict(rtol=1e-4, atol=1e-5)     # test_layernorm
TOL_HEAD = dict(rtol=1e-4, atol=1e-4)          # check_head
TOL_EMBED = dict(rtol=1e-4, atol=1e-5)         # check_action_embed

VARIANTS = ["bias", "ln", "mod_rows1", "mod_rows3", "mod_bcast", "gelu", "gated", "remap", "aux1", "aux2"]
LN_VARIANTS = ("ln", "mod_rows1", "mod_rows3", "mod_bcast")


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, variant):
    """Host operands of one mdt_op_gemm call and its float64 results (shared between the guarded and the dense call and between
    the bodies: never written to).  A mod row is [shift (K) | scale (K) | gate (N)]."""
    g = seeded(M, N, K, variant)
    c = types.SimpleNamespace(M=M, N=N, K=K, variant=variant, bias=None, ln_w=None, ln_b=None, mod=None, rps=1, bcast=False,
                              modded=False, act="none", y0=None, gated=False, gin=1, gout=1, goff=0, rowvec=None, aux_mode=0,
                              aux_in=None, out_rows=M)
    c.A = torch.randn(M, K, generator=g) * (2.0 if variant in LN_VARIANTS else 1.0) + (0.3 if variant in LN_VARIANTS else 0.0)
    c.W = torch.randn(N, K, generator=g) / math.sqrt(K)
    if variant != "aux2":
        c.bias = torch.randn(N, generator=g)
    if variant in LN_VARIANTS:
        c.ln_w, c.ln_b = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.2
    if variant.startswith("mod_") or variant == "gated":
        c.rps = {"mod_rows1": 1, "mod_rows3": 3, "mod_bcast": 5, "gated": 3}[variant]
        c.bcast = variant == "mod_bcast"
        c.mod = torch.randn(1 if c.bcast else (M + c.rps - 1) // c.rps, 2 * K + N, generator=g)
        c.modded, c.gated = variant != "gated", variant == "gated"
    if variant in ("gelu", "aux1", "aux2"):
        c.act = "gelu"
    if variant == "gated":
        c.y0 = torch.randn(M, N, generator=g)
    if variant == "remap":
        c.gin, c.gout, c.goff, c.rowvec = 3, 4, 1, torch.randn(N, generator=g)
        c.out_rows = ((M - 1) // 3 + 1) * 4
    if variant in ("aux1", "aux2"):
        c.aux_mode = int(variant[-1])
        c.aux_in = torch.randn(M, N, generator=g) if c.aux_mode == 2 else None
    # float64
    x = c.A.double()
    if c.ln_w is not None:
        x = F.layer_norm(x, (K,), c.ln_w.double(), c.ln_b.double(), 1e-5)
    srow = torch.zeros(M, dtype=torch.long) if (c.bcast or c.mod is None) else torch.arange(M) // c.rps
    if c.modded:
        x = c.mod[srow, :K].double() + x * c.mod[srow, K:2 * K].double()
    v = x @ c.W.double().T
    if c.bias is not None:
        v = v + c.bias.double()
    if c.rowvec is not None:
        v = v + c.rowvec.double()
    c.want = {}
    if c.aux_mode == 2:
        u = c.aux_in.double().requires_grad_()
        act_fn(c.act)(u).sum().backward()
        out = v * u.grad
    else:
        if c.aux_mode == 1:
            c.want["aux"] = v
        out = act_fn(c.act)(v)
    if c.y0 is not None:
        out = c.y0.double() + (c.mod[srow, 2 * K:].double() * out if c.gated else out)
    c.want["out"] = out
    m = torch.arange(M)
    c.orow = (m // c.gin) * c.gout + m % c.gin + c.goff
    c.image = torch.from_numpy(expected_pack(c.W))
    return c


def run_gemm(lib, c, guarded, what):
    """One mdt_op_gemm call on the case's operands -> {name: host tensor} of what it wrote."""
    M, N, K = c.M, c.N, c.K
    L = Lay(guarded)
    A, Wp = L.inp("A", c.A, pad=4), L.image("Wp", c.image)
    fill = c.y0 if c.y0 is not None else (canary(c.out_rows, N) if c.out_rows != M else None)
    out = L.out("out", c.out_rows, N, pad=4, fill=fill)
    opt = {k: L.inp(k, getattr(c, k)) for k in ("bias", "ln_w", "ln_b", "rowvec") if getattr(c, k) is not None}
    mod = L.inp("mod", c.mod, pad=4) if c.mod is not None else None
    aux = None
    if c.aux_mode == 1:
        aux = L.out("aux", M, N, pad=4)
    elif c.aux_mode == 2:
        aux = L.inp("aux", c.aux_in, pad=4)
    a = lib.GemmArgs()
    a.A, a.lda, a.Wp, a.out, a.ldo, a.M, a.N, a.K = A.ptr, A.ld, Wp.ptr, out.ptr, out.ld, M, N, K
    for k, o in opt.items():
        setattr(a, k, o.ptr)
    a.ln = int(c.ln_w is not None)
    a.shift_off = a.scale_off = a.gate_off = -1
    if mod is not None:
        a.mod, a.mod_stride = mod.ptr, 0 if c.bcast else mod.ld
        if c.modded:
            a.shift_off, a.scale_off = 0, K
        if c.gated:
            a.gate_off = 2 * K
    a.rows_per_sample, a.act, a.residual = c.rps, lib.ACT[c.act], int(c.y0 is not None)
    a.gin, a.gout, a.goff = c.gin, c.gout, c.goff
    a.aux, a.aux_mode = ptr(aux), c.aux_mode
    lib.check(lib.load().mdt_op_gemm(C.byref(a), stream()))
    L.check(what)
    res = {"out": out.host()}
    if c.aux_mode == 1:
        aux.check(f"{what}: aux", written=True)
        res["aux"] = aux.host()
    if c.out_rows == M:
        out.check(f"{what}: out", written=True)
    return res


def check_gemm(lib, c, tol, what):
    """(a) - (e) for one case under whatever geometry is set."""
    dense, guard = run_gemm(lib, c, False, what + " (dense)"), run_gemm(lib, c, True, what)
    for name, want in c.want.items():
        got = guard[name][c.orow] if name == "out" else guard[name]
        assert not got.isnan().any(), f"{what}: NaN in {name}"
        assert_close(got, want, what=f"{what}: {name}", **tol)
        assert same_bits(guard[name], dense[name]), f"{what}: {name} differs from the dense call's bits"
    if c.out_rows != c.M:   # (e) the rows the remap skips
        skipped = torch.ones(c.out_rows, dtype=torch.bool)
        skipped[c.orow] = False
        assert same_bits(guard["out"][skipped], canary(c.out_rows, c.N)[skipped]), f"{what}: a row the remap skips was touched"


def tol_of(c, geo):
    if c.variant == "aux2":
        return TOL_AUX2
    return TOL_LN if (c.variant in LN_VARIANTS or geo <= 0) else TOL_GEMM   # (geometry 0 / -1: the split-K kernel's tolerance)


class geometry:
    """mdt_op_set_gemm_geometry for a block, reset to 0 behind it."""

    def __init__(self, lib, geo):
        self.L, self.geo = lib.load(), geo

    def __enter__(self):
        self.L.mdt_op_set_gemm_geometry(self.geo)

    def __exit__(self, *exc):
        self.L.mdt_op_set_gemm_geometry(0)


# geometry -> the width of its column tile (mdt_launch_gemm: NWAVES x NTW x 16; 0 / -1: the 16-column split-K workgroups)
TILE_N = {0: 64, -1: 64, 1: 64, 2: 128, 3: 384, 4: 512, 5: 128, 6: 64, 7: 128, 8: 256, 9: 192}
ROW_GEOS = sorted(TILE_N)


@pytest.mark.parametrize("geo", ROW_GEOS)
def test_gemm_plain_bias_every_row_tile_body(lib, geo):
    """Plain rows + bias on the heuristic choice, the split-K kernel (-1) and geometries 1 - 9: M one off each row-tile height,
    N = 16 and 16 past the tile width, K in one LDS chunk (48) and in several (528: the loader-wave kernels of geometries 2, 6)."""
    with geometry(lib, geo):
        for M in (1, 15, 17, 33):
            for N in (16, TILE_N[geo] + 16):
                for K in (48, 528):
                    c = gemm_case(M, N, K, "bias")
                    check_gemm(lib, c, tol_of(c, geo), f"geometry {geo}, {M} x {N} x {K}")


@pytest.mark.parametrize("geo", ROW_GEOS)
def test_gemm_layernorm_prologue_every_row_tile_body(lib, geo):
    """LayerNorm with ln_b on the same bodies, K = 80 (five float4 per lane group: a ragged column mask) and 512 (the limit)."""
    with geometry(lib, geo):
        for M in (1, 15, 17, 33):
            for N in (16, TILE_N[geo] + 16):
                for K in (80, 512):
                    c = gemm_case(M, N, K, "ln")
                    check_gemm(lib, c, tol_of(c, geo), f"geometry {geo}, LayerNorm, {M} x {N} x {K}")


# (the split-K kernel has no training hooks: under -1 mdt_op_gemm sends them to the tiles, which geometry 0 covers)
FEATURES = [(geo, v) for geo in ROW_GEOS for v in VARIANTS if v not in ("bias", "ln") and not (geo == -1 and v.startswith("aux"))]


@pytest.mark.parametrize("geo,variant", FEATURES)
def test_gemm_prologues_and_epilogues_every_row_tile_body(lib, geo, variant):
    """Each fused feature once at a ragged M = 33: modulate by rows (one row per sample -- the slow path -- and three, a sample
    straddling a tile), modulate broadcast, GELU, gated residual with gate_off, rowvec with the remap gin = 3, gout = 4, goff = 1,
    aux_mode 1 and 2."""
    c = gemm_case(33, TILE_N[geo] + 16, 80 if variant in LN_VARIANTS else 48, variant)
    with geometry(lib, geo):
        check_gemm(lib, c, tol_of(c, geo), f"geometry {geo}, {variant}")


def test_gemm_tall_body(lib):
    """Geometry 23 (128-row tiles, K % 32 == 0, plain prologue): M one off its tile height, N = 16 and 80 (64-wide tiles), one and
    three 32-deep K blocks, and every epilogue it carries at M = 129."""
    with geometry(lib, 23):
        for M in (1, 127, 129):
            for N in (16, 80):
                for K in (64, 96):
                    c = gemm_case(M, N, K, "bias")
                    check_gemm(lib, c, TOL_GEMM, f"tall body, {M} x {N} x {K}")
        for variant in ("gelu", "gated", "remap", "aux1", "aux2"):
            c = gemm_case(129, 80, 64, variant)
            check_gemm(lib, c, tol_of(c, 23), f"tall body, {variant}")


@pytest.mark.parametrize("split", [0, 1])
def test_gemm_weight_stationary_body(lib, split):
    """Geometry 30 at K = 384: the two smallest M >= 32 that are no multiple of 32 (33, 34), N = 128 (eight waves) and 192
    (twelve); plain + bias, GELU and the two training hooks; the fp32 MFMA form and the three-way bf16 split form (which takes
    N = 128 only: fp32's product accuracy, the same tolerance)."""
    L = lib.load()
    try:
        L.mdt_op_set_ws_split(split)
        with geometry(lib, 30):
            for M in (33, 34):
                for N in (128, 192):
                    for variant in ("bias", "gelu", "aux1", "aux2"):
                        c = gemm_case(M, N, 384, variant)
                        check_gemm(lib, c, tol_of(c, 30), f"weight-stationary body (split {split}), {variant}, {M} x {N} x 384")
    finally:
        L.mdt_op_set_ws_split(-1)


def pack_glu(W):
    """Host image of mdt_op_pack_weight_glu: 16-row tile 2t = projected rows [16t, 16t + 16), tile 2t + 1 = gate rows [H + 16t, ..)."""
    H = W.shape[0] // 2
    order = torch.stack([torch.arange(H).view(-1, 16), H + torch.arange(H).view(-1, 16)], dim=1).reshape(-1)
    return torch.from_numpy(expected_pack(W[order].contiguous()))


@pytest.mark.parametrize("M,K,H", [(33, 48, 48), (33, 512, 208)])
@pytest.mark.parametrize("mode", [3, 4])
def test_gemm_swiglu_epilogues(lib, mode, M, K, H):
    """aux_mode 3 (u (M, 2H; 2 ldo) and projected * silu(gate) (M, H; ldo) from one launch, interleaved weight image) and aux_mode 4
    (out (M, 2H; ldo) = [d silu(gate) | d projected silu'(gate)] with u (M, 2H; ldo) read beside it)."""
    g = seeded(mode, M, K, H)
    A = torch.randn(M, K, generator=g)
    res = {}
    if mode == 3:
        W, b = torch.randn(2 * H, K, generator=g) / math.sqrt(K), torch.randn(2 * H, generator=g) * 0.3
        u = A.double() @ W.double().T + b.double()
        want = {"aux": u, "out": u[:, :H] * F.silu(u[:, H:])}
        image = pack_glu(W)
    else:
        W, u_in = torch.randn(H, K, generator=g) / math.sqrt(K), torch.randn(M, 2 * H, generator=g)
        u64 = u_in.double().requires_grad_()
        (u64[:, :H] * F.silu(u64[:, H:])).backward(A.double() @ W.double().T)
        want = {"out": u64.grad}
        image = torch.from_numpy(expected_pack(W))
    for guarded in (False, True):
        what = f"aux_mode {mode}, {M} x {K} x {H}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        Ad, Wp = L.inp("A", A, pad=4), L.image("Wp", image)
        a = lib.GemmArgs()
        if mode == 3:
            out, aux, bd = L.out("out", M, H, pad=4), L.out("aux", M, 2 * H, pad=8), L.inp("bias", b)
            a.bias, a.N = bd.ptr, 2 * H
        else:
            out, aux = L.out("out", M, 2 * H, pad=4), L.inp("aux", u_in, pad=4)
            a.N = H
        assert aux.ld == (2 if mode == 3 else 1) * out.ld
        a.A, a.lda, a.Wp, a.out, a.ldo, a.M, a.K, a.aux, a.aux_mode = Ad.ptr, Ad.ld, Wp.ptr, out.ptr, out.ld, M, K, aux.ptr, mode
        a.shift_off = a.scale_off = a.gate_off = -1
        a.rows_per_sample = a.gin = a.gout = 1
        lib.check(lib.load().mdt_op_gemm(C.byref(a), stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        res[guarded] = {"out": out.host()}
        if mode == 3:
            aux.check(what + ": aux", written=True)
            res[guarded]["aux"] = aux.host()
    for name, w in want.items():
        assert_close(res[True][name], w, what=f"aux_mode {mode}: {name}", **TOL_AUX2)
        assert same_bits(res[True][name], res[False][name]), f"aux_mode {mode}: {name} differs from the dense call's bits"


def test_gemm_batched_launch(lib):
    """batch = 3 members bs_a / bs_w / bs_out apart, a guard-pattern gap between neighbours, at 17 x 80 x 48; the bias is shared."""
    M, N, K, Z = 17, 80, 48, 3
    g = seeded("batched")
    A, W, b = torch.randn(Z, M, K, generator=g), torch.randn(Z, N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    images = torch.stack([torch.from_numpy(expected_pack(W[z])) for z in range(Z)]).reshape(Z, -1, 256)
    res = {}
    for guarded in (False, True):
        what = "batched launch" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        Ad, Wp, bd = L.inp("A", A, pad=4, gap=64), L.inp("Wp", images, gap=64), L.inp("bias", b)
        out = L.out("out", M, N, pad=4, slabs=Z, gap=64)
        a = lib.GemmArgs()
        a.A, a.lda, a.Wp, a.bias, a.out, a.ldo, a.M, a.N, a.K = Ad.ptr, Ad.ld, Wp.ptr, bd.ptr, out.ptr, out.ld, M, N, K
        a.batch, a.bs_a, a.bs_w, a.bs_out = Z, Ad.slab_stride, Wp.slab_stride, out.slab_stride
        a.shift_off = a.scale_off = a.gate_off = -1
        a.rows_per_sample = a.gin = a.gout = 1
        lib.check(lib.load().mdt_op_gemm(C.byref(a), stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        res[guarded] = out.host()
    assert_close(res[True], A.double() @ W.double().transpose(1, 2) + b.double(), what="batched launch", **TOL_GEMM)
    assert same_bits(res[True], res[False]), "batched launch differs from the dense call's bits"


@functools.lru_cache(maxsize=None)
def ln_weight(N, K):
    """A (N, K) weight and its three images (host tensors; the byte images as float32 words)."""
    g = seeded("ln_weight", N, K)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    return (W, torch.from_numpy(expected_pack(W)), expected_pack_split(W).view(torch.float32),
            expected_pack_pair(W)[0].view(torch.float32))


MERGE_FORMS = {"fp32": 33, "pair": 33, "split": 801}   # rows: the bf16 split form applies from 768 rows on (mdt_op_gemm's rule)


@pytest.mark.parametrize("K", [384, 512])
@pytest.mark.parametrize("form,XP", [(f, x) for f in sorted(MERGE_FORMS) for x in (1, 2, 3, 4) if not (f == "fp32" and x == 1)])
def test_gemm_reads_the_sum_of_gapped_slabs(lib, form, XP, K):
    """a_parts slabs a_part_stride apart (a guard-pattern gap between them, lda = K + 4) through the fp32 merge kernel, the fp16
    pair form (mdt_op_gemm_ln_pair, any row count) and the bf16 split form (Wp_split; from 768 rows on, so 801 here), N = 384:
    a_merged (a Guarded, row stride lda) is the slab-order fp32 sum bit for bit.  XP = 1: the pair / split form on plain rows
    (the fp32 form of that is test_gemm_layernorm_prologue_every_row_tile_body's)."""
    M, N = MERGE_FORMS[form], 384
    g = seeded("merge", form, XP, K)
    slabs = torch.randn(XP, M, K, generator=g)
    W, image, split, pair = ln_weight(N, K)
    b, lw, lb = torch.randn(N, generator=g), torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.2
    summed = slabs[0].clone()
    for s in range(1, XP):
        summed = summed + slabs[s]
    want = F.layer_norm(summed.double(), (K,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()
    res = {}
    Lh = lib.load()
    try:
        if form == "split":
            Lh.mdt_op_set_mlp_split(1)
        for guarded in (False, True):
            what = f"{form} form, {XP} slab(s), K = {K}" + ("" if guarded else " (dense)")
            L = Lay(guarded)
            Ad = L.inp("A", slabs if XP > 1 else slabs[0], pad=4, gap=1024)
            out, bd, lwd, lbd = L.out("out", M, N, pad=4), L.inp("bias", b), L.inp("ln_w", lw), L.inp("ln_b", lb)
            a = lib.GemmArgs()
            a.A, a.lda, a.bias, a.out, a.ldo, a.M, a.N, a.K = Ad.ptr, Ad.ld, bd.ptr, out.ptr, out.ld, M, N, K
            a.ln, a.ln_w, a.ln_b = 1, lwd.ptr, lbd.ptr
            a.shift_off = a.scale_off = a.gate_off = -1
            a.rows_per_sample = a.gin = a.gout = 1
            merged = None
            if XP > 1:
                merged = L.out("a_merged", M, K, pad=4)
                a.a_parts, a.a_part_stride, a.a_merged = XP, Ad.slab_stride, merged.ptr
            if form == "pair":
                a.Wp_pair = L.image("Wp_pair", pair).ptr
                lib.check(Lh.mdt_op_gemm_ln_pair(C.byref(a), stream()))
            else:
                a.Wp = L.image("Wp", image).ptr
                if form == "split":
                    a.Wp_split = L.image("Wp_split", split).ptr
                lib.check(Lh.mdt_op_gemm(C.byref(a), stream()))
            L.check(what)
            out.check(what + ": out", written=True)
            if merged is not None:
                merged.check(what + ": a_merged", written=True)
                assert same_bits(merged.host(), summed), f"{what}: a_merged is not the slab-order sum"
            res[guarded] = out.host()
    finally:
        Lh.mdt_op_set_mlp_split(-1)
    assert_close(res[True], want, what=f"{form} form", **(TOL_LN if form == "fp32" else TOL_GEMM))
    assert same_bits(res[True], res[False]), f"{form} form: differs from the dense call's bits"


@functools.lru_cache(maxsize=None)
def mlp_weights(D):
    g = seeded("mlp", D)
    W1, W2 = torch.randn(4 * D, D, generator=g) / math.sqrt(D), torch.randn(D, 4 * D, generator=g) / math.sqrt(4 * D)
    im = {"fp32": (torch.from_numpy(expected_pack(W1)), torch.from_numpy(expected_pack(W2))),
          "split": (expected_pack_split(W1).view(torch.float32), expected_pack_split(W2).view(torch.float32)),
          "pair": (expected_pack_pair(W1)[0].view(torch.float32), expected_pack_pair(W2)[0].view(torch.float32))}
    return W1, W2, im


def run_mlp(lib, form, guarded, x, im, lw, lb, b1, b2, modulate, gate, mod, T, in_place, what):
    """One fused-MLP launch -> the slabs summed in slab order (fp32, on the host).  mod: None, one row (broadcast) or one row
    per sample of T rows, [shift | scale | gate]."""
    M, D = x.shape
    S = 4 * D // 512
    L = Lay(guarded)
    xd = L.out("x", M, D, pad=4, fill=x) if in_place else L.inp("x", x, pad=4)
    parts = xd if in_place else L.out("parts", M, D, pad=4, slabs=S, gap=1024 - 4 * M)   # part_stride = M D + 1024
    I1, I2 = L.image("W1", im[0]), L.image("W2", im[1])
    o = {k: L.inp(k, v) for k, v in dict(ln_w=lw, ln_b=lb, b1=b1, b2=b2).items()}
    md = L.inp("mod", mod, pad=4) if mod is not None else None
    f, p = lib.GemmArgs(), lib.GemmArgs()
    for a in (f, p):
        a.shift_off = a.scale_off = a.gate_off = -1
        a.rows_per_sample = a.gin = a.gout = 1
        a.M = M
    f.A, f.lda, f.N, f.K, f.bias, f.ln, f.ln_w, f.ln_b, f.act = xd.ptr, xd.ld, 4 * D, D, o["b1"].ptr, 1, o["ln_w"].ptr, o["ln_b"].ptr, 1
    p.N, p.K, p.bias, p.ldo = D, 4 * D, o["b2"].ptr, parts.ld
    if form == "fp32":
        f.Wp, p.Wp = I1.ptr, I2.ptr
    stride = 0 if (mod is None or mod.shape[0] == 1) else md.ld
    if modulate:
        f.mod, f.mod_stride, f.shift_off, f.scale_off, f.rows_per_sample = md.ptr, stride, 0, D, T
    if gate:
        p.mod, p.mod_stride, p.gate_off, p.rows_per_sample = md.ptr, stride, 2 * D, T
    part_stride = parts.slab_stride if S > 1 else M * parts.ld
    if guarded and S > 1:
        assert part_stride == M * D + 1024
    n = C.c_int32(0)
    Lh = lib.load()
    if form == "fp32":
        lib.check(Lh.mdt_op_mlp(C.byref(f), C.byref(p), parts.ptr, part_stride, C.byref(n), stream()))
    else:
        fn = Lh.mdt_op_mlp_split if form == "split" else Lh.mdt_op_mlp_pair
        lib.check(fn(C.byref(f), C.byref(p), I1.ptr, I2.ptr, parts.ptr, part_stride, C.byref(n), stream()))
    L.check(what)
    parts.check(what + ": slabs", written=True)
    assert n.value == S
    slabs = parts.host().reshape(S, M, D)
    got = slabs[0].clone()
    for s in range(1, S):
        got += slabs[s]
    return got


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("pro", ["plain", "bcast", "rows"])
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("D", [128, 384, 512])
def test_fused_mlp_forms_with_gapped_slabs(lib, D, M, pro, gate):
    """mdt_op_mlp, mdt_op_mlp_split and mdt_op_mlp_pair: lda = ldo = D + 4, slabs part_stride = M D + 1024 apart with guard
    pattern between them; every prologue (plain, broadcast modulation, modulation by rows of three-row samples: a sample straddles
    the 32-row tile), gate on and off (beside a plain prologue: a per-sample gate); D = 128 (one slab) also in place, parts == x.
    At 33 rows the split forms are held to the project's gate for them as well -- their error against float64 within 1.5x the
    fp32 launch's + 1e-6 (a statement about the largest of many errors: not asserted on the 128 .. 512 outputs of one row)."""
    g = seeded("mlp case", D, M, pro, gate)
    W1, W2, images = mlp_weights(D)
    T = 3
    x = torch.randn(M, D, generator=g) * 1.5 + 0.2
    lw, lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    b1, b2 = torch.randn(4 * D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    mod, ref = None, {}
    if pro != "plain" or gate:
        by_rows = pro != "bcast"
        mod = torch.randn((M + T - 1) // T if by_rows else 1, 3 * D, generator=g) * 0.5
        pick = (lambda o: mod[torch.arange(M) // T, o:o + D]) if by_rows else (lambda o: mod[:, o:o + D])
        if pro != "plain":
            ref.update(shift=pick(0), scale=pick(D))
        if gate:
            ref.update(gate=pick(2 * D))
    want = ref_mlp(x, W1, W2, lw, lb, b1, b2, **ref)
    err = {}
    for form in ("fp32", "split", "pair"):
        for in_place in ([False, True] if D == 128 else [False]):
            what = f"mdt_op_mlp {form}, D = {D}, M = {M}, {pro}, gate {gate}" + (", in place" if in_place else "")
            kw = dict(x=x, im=images[form], lw=lw, lb=lb, b1=b1, b2=b2, modulate=pro != "plain", gate=gate, mod=mod, T=T,
                      in_place=in_place)
            dense = run_mlp(lib, form, False, what=what + " (dense)", **kw)
            got = run_mlp(lib, form, True, what=what, **kw)
            assert_close(got, want, what=what, **TOL_MLP)
            assert same_bits(got, dense), f"{what}: differs from the dense call's bits"
            err[form] = (got.double() - want).abs().max().item()
    if M >= 33:
        for form in ("split", "pair"):
            assert err[form] <= 1.5 * err["fp32"] + 1e-6, f"{form} form: max error {err[form]:.3g} against the fp32 launch's {err['fp32']:.3g}"


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Tq,Tk", [(1, 1), (10, 4), (16, 16), (5, 11)])
@pytest.mark.parametrize("hd", [16, 32, 48, 64])
def test_attention_on_column_blocks_of_one_strided_row(lib, hd, Tq, Tk, causal, B):
    """mdt_op_attention with q | k | v as column blocks of ONE buffer of row stride 3 H hd + 4 (q on its first B Tq rows, k / v on
    its first B Tk; what neither uses holds NaN), ldo = H hd + 4; B = 64 takes the head split; RoPE as well where hd >= 32."""
    H = 4
    D = H * hd
    g = seeded("attention", hd, Tq, Tk, B)
    q, k, v = (torch.randn(B, T, D, generator=g) for T in (Tq, Tk, Tk))
    rows = B * max(Tq, Tk)
    qkv = torch.full((rows, 3 * D), NAN)
    qkv[:B * Tq, :D], qkv[:B * Tk, D:2 * D], qkv[:B * Tk, 2 * D:] = q.reshape(-1, D), k.reshape(-1, D), v.reshape(-1, D)
    for rope in ([False, True] if hd >= 32 else [False]):
        res = {}
        for guarded in (False, True):
            what = f"attention hd {hd}, {Tq} x {Tk}, causal {causal}, rope {rope}, B {B}" + ("" if guarded else " (dense)")
            L = Lay(guarded)
            x, out = L.inp("qkv", qkv, pad=4), L.out("out", B * Tq, D, pad=4)
            a = lib.AttnArgs(q=x.at(0, 0), ldq=x.ld, k=x.at(0, D), v=x.at(0, 2 * D), ldkv=x.ld, out=out.ptr, ldo=out.ld, B=B, H=H,
                             hd=hd, Tq=Tq, Tk=Tk, causal=int(causal), rope=int(rope))
            lib.check(lib.load().mdt_op_attention(C.byref(a), stream()))
            L.check(what)
            out.check(what + ": out", written=True)
            res[guarded] = out.host()
        assert_close(res[True].reshape(B, Tq, D), ref_attn(q, k, v, H, causal, rope=rope), what=what, **TOL_ATTN)
        assert same_bits(res[True], res[False]), f"{what}: differs from the dense call's bits"


def attn_proj_case(hd, T, B, seed):
    """qkv rows, the projection and its gate, and the float64 rows after  y += gate * (attention @ W^T + b)  (causal, 8 heads)."""
    g = seeded("attn_proj", hd, T, B, seed)
    H, D = 8, 8 * hd
    c = types.SimpleNamespace(H=H, D=D, hd=hd, T=T, B=B)
    c.qkv = torch.randn(B * T, 3 * D, generator=g)
    c.W, c.b = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    c.gate, c.y0 = torch.randn(B, D, generator=g), torch.randn(B * T, D, generator=g)
    q3 = c.qkv.view(B, T, 3 * D)
    att = ref_attn(q3[..., :D], q3[..., D:2 * D], q3[..., 2 * D:], H, True).double().reshape(B * T, D)
    c.want = c.y0.double() + c.gate.double().repeat_interleave(T, 0) * (att @ c.W.double().T + c.b.double())
    c.image = torch.from_numpy(expected_pack(c.W))
    return c


def proj_args(lib, L, c, out, pad_ldo=True):
    Wp, bd, gd = L.image("Wp", c.image), L.inp("bias", c.b), L.inp("gate", c.gate, pad=4)
    a = lib.GemmArgs()
    a.lda, a.Wp, a.bias, a.out, a.ldo, a.M, a.N, a.K = c.D, Wp.ptr, bd.ptr, out.ptr, out.ld, c.B * c.T, c.D, c.D
    a.shift_off = a.scale_off = -1
    a.gate_off, a.mod, a.mod_stride = 0, gd.ptr, gd.ld
    a.residual, a.rows_per_sample, a.gin, a.gout = 1, c.T, 1, 1
    return a


# the per-sample kernel (at most 64 samples), and the tiled form at the smallest batch above 64 samples
@pytest.mark.parametrize("hd,T,B", [(hd, T, 3) for hd in (16, 48, 64) for T in (1, 10, 16)] + [(16, 7, 65)])
def test_attention_fused_into_its_projection(lib, hd, T, B):
    """mdt_op_attn_proj with ldq = 3 K + 4, ldo = N + 4 and a padded gate row: the per-sample kernel, and k_attn_proj_wide (whose
    32-row tiles reach back into the previous tile's keys) at 65 samples of 7 rows."""
    c = attn_proj_case(hd, T, B, 0)
    res = {}
    for guarded in (False, True):
        what = f"attn_proj hd {hd}, T {T}, B {B}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        qd, out = L.inp("qkv", c.qkv, pad=4), L.out("out", B * T, c.D, pad=4, fill=c.y0)
        a = proj_args(lib, L, c, out)
        lib.check(lib.load().mdt_op_attn_proj(C.byref(a), qd.ptr, qd.ld, hd, T, 1, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        res[guarded] = out.host()
    assert_close(res[True], c.want, what=what, **TOL_ATTN_PROJ)
    assert same_bits(res[True], res[False]), f"{what}: differs from the dense call's bits"


def xattn_case(D, H, Te, Ta, B, seed, y=None):
    """Operands of the collapsed cross-attention and the float64 rows  y + c_proj(softmax_causal(q K^T / sqrt(hd)) V) + bo."""
    g = seeded("xattn", D, H, Te, Ta, B, seed)
    c = types.SimpleNamespace(D=D, H=H, hd=D // H, Te=Te, Ta=Ta, B=B, NP=4 * H)
    c.y = torch.randn(B * Ta, D, generator=g) * 2 if y is None else y
    c.kv = torch.randn(B * Te, 2 * D, generator=g)
    c.Wq, c.bq = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.3
    c.Wo, c.bo = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.3
    c.lw, c.lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    c.WqT_p, c.Wo_p = torch.from_numpy(expected_pack(c.Wq.T.contiguous())), torch.from_numpy(expected_pack(c.Wo))
    return c


def ref_xattn(c, y):
    B, Ta, Te, D, H, hd = c.B, c.Ta, c.Te, c.D, c.H, c.hd
    yd, kd = y.double().view(B, Ta, D), c.kv.double()
    K, V = kd[:, :D].view(B, Te, D), kd[:, D:].view(B, Te, D)
    q = F.layer_norm(yd, (D,), c.lw.double(), c.lb.double(), 1e-5) @ c.Wq.double().T + c.bq.double()
    qh, kh, vh = (x.view(B, -1, H, hd).transpose(1, 2) for x in (q, K, V))
    att = (qh @ kh.transpose(-2, -1) / math.sqrt(hd)).masked_fill(~torch.ones(Ta, Te, dtype=torch.bool).tril(), float("-inf"))
    return (yd + (att.softmax(-1) @ vh).transpose(1, 2).reshape(B, Ta, D) @ c.Wo.double().T + c.bo.double()).reshape(B * Ta, D)


def fold(lib, L, c, what, refused=False):
    """mdt_op_xattn_fold with ldkv = 2 D + 4 into guarded U / Wf / c -> (U, Wf, c) operands.  refused: the call has to return
    MDT_ERR_UNSUPPORTED and leave the three outputs, which then start as the canary, as they are."""
    kv, WqT, bq, Wo = L.inp("kv", c.kv, pad=4), L.image("WqT_p", c.WqT_p), L.inp("bq", c.bq), L.image("Wo_p", c.Wo_p)
    start = (lambda *shape: canary(*shape)) if refused else (lambda *shape: None)
    U, Wf, cc = (L.out(k, c.B, n, fill=start(c.B, n)) for k, n in (("U", c.NP * c.D), ("Wf", c.NP * c.D), ("c", c.NP)))
    f = lib.XFoldArgs(kv=kv.ptr, ldkv=kv.ld, WqT_p=WqT.ptr, bq=bq.ptr, Wo_p=Wo.ptr, U=U.ptr, Wf=Wf.ptr, c=cc.ptr, B=c.B, H=c.H,
                      hd=c.hd, D=c.D, Te=c.Te)
    status = lib.load().mdt_op_xattn_fold(C.byref(f), stream())
    if refused:
        L.check(what + ": refused fold")
        assert status == 2, f"{what}: status {status}, not MDT_ERR_UNSUPPORTED"
        for o in (U, Wf, cc):
            assert o.keeps(), f"{what}: a refused fold wrote into its outputs"
        return None
    lib.check(status)
    L.check(what + ": fold")
    U.check(what + ": U", written=True)
    cc.check(what + ": c", written=True)
    return U, Wf, cc


def apply_args(lib, L, c, y, U, Wf, cc, y_out=None):
    lw, lb, bo = L.inp("ln_w", c.lw), L.inp("ln_b", c.lb), L.inp("bo", c.bo)
    return lib.XApplyArgs(y=y.ptr, ln_w=lw.ptr, ln_b=lb.ptr, U=U.ptr, Wf=Wf.ptr, c=cc.ptr, bo=bo.ptr, B=c.B, H=c.H, D=c.D, Te=c.Te,
                          Ta=c.Ta, y_out=ptr(y_out))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Ta", [1, 16])
@pytest.mark.parametrize("Te", [1, 3, 4])
@pytest.mark.parametrize("D,H", [(128, 4), (128, 8), (512, 4), (512, 8)])
def test_collapsed_cross_attention_fold_apply_and_the_linear_behind_it(lib, D, H, Te, Ta, B):
    """mdt_op_xattn_fold (ldkv = 2 D + 4; U, Wf, c guarded), mdt_op_xattn_apply in place (y_out NULL) and into a separate y_out
    (y then keeps its bits), and mdt_op_xattn_gemm (the cross-attention inside a 48-column LayerNorm + GELU Linear) on the same
    folded operands.  Heads of 128 (D = 512 in 4 heads) are beyond what the fold kernel holds in registers: that combination has to
    be refused as unsupported before anything is launched."""
    c = xattn_case(D, H, Te, Ta, B, 0)
    if c.hd > 64:
        fold(lib, Lay(True), c, f"xattn D {D}, H {H}", refused=True)
        return
    want = ref_xattn(c, c.y)
    g = seeded("xattn fc", D, H)
    N = 48
    W, b = torch.randn(N, D, generator=g) / math.sqrt(D), torch.randn(N, generator=g) * 0.1
    lw2, lb2 = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    want_fc = F.gelu(F.layer_norm(want, (D,), lw2.double(), lb2.double(), 1e-5) @ W.double().T + b.double())
    res = {}
    for guarded in (False, True):
        what = f"xattn D {D}, H {H}, Te {Te}, Ta {Ta}, B {B}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        U, Wf, cc = fold(lib, L, c, what)
        folded = {k: bits(o.region) for k, o in dict(U=U, Wf=Wf, c=cc).items()}
        r = {}
        # in place
        y = L.out("y", B * Ta, D, fill=c.y)
        lib.check(lib.load().mdt_op_xattn_apply(C.byref(apply_args(lib, L, c, y, U, Wf, cc)), stream()))
        L.check(what + ": apply in place")
        y.check(what + ": y", written=True)
        r["in place"] = y.host()
        # separate output
        y2, yo = L.inp("y2", c.y), L.out("y_out", B * Ta, D)
        lib.check(lib.load().mdt_op_xattn_apply(C.byref(apply_args(lib, L, c, y2, U, Wf, cc, yo)), stream()))
        L.check(what + ": apply into y_out")
        yo.check(what + ": y_out", written=True)
        r["y_out"] = yo.host()
        # inside the Linear that follows
        y3, yo3, o3 = L.inp("y3", c.y), L.out("y_out3", B * Ta, D), L.out("fc", B * Ta, N, pad=4)
        Wp, bd, l2, b2 = L.image("Wp", torch.from_numpy(expected_pack(W))), L.inp("b", b), L.inp("ln_w2", lw2), L.inp("ln_b2", lb2)
        x = apply_args(lib, L, c, y3, U, Wf, cc, yo3)
        a = lib.GemmArgs()
        a.A, a.lda, a.Wp, a.bias, a.out, a.ldo, a.M, a.N, a.K = y3.ptr, D, Wp.ptr, bd.ptr, o3.ptr, o3.ld, B * Ta, N, D
        a.ln, a.ln_w, a.ln_b, a.act = 1, l2.ptr, b2.ptr, 1
        a.shift_off = a.scale_off = a.gate_off = -1
        a.rows_per_sample, a.gin, a.gout = Ta, 1, 1
        lib.check(lib.load().mdt_op_xattn_gemm(C.byref(x), C.byref(a), stream()))
        L.check(what + ": xattn_gemm")
        yo3.check(what + ": y_out of xattn_gemm", written=True)
        o3.check(what + ": c_fc rows", written=True)
        r["gemm y_out"], r["fc"] = yo3.host(), o3.host()
        for k, o in dict(U=U, Wf=Wf, c=cc).items():
            assert torch.equal(bits(o.region), folded[k]), f"{what}: {k} changed after the fold"
        res[guarded] = r
    for k in ("in place", "y_out", "gemm y_out"):
        assert_close(res[True][k], want, what=f"{what}: {k}", **TOL_XATTN)
    assert_close(res[True]["fc"], want_fc, what=f"{what}: c_fc", **TOL_XATTN_FC)
    for k in res[True]:
        assert same_bits(res[True][k], res[False][k]), f"{what}: {k} differs from the dense call's bits"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [10, 16])
def test_attention_projection_and_cross_attention_in_one_launch(lib, T, B):
    """mdt_op_attn_xattn (one workgroup per sample; 8 heads of 48): its contract fixes ldq = 3 K and ldo = N, so these operands
    get guards and no pad; Te = 3."""
    hd, Te = 48, 3
    p = attn_proj_case(hd, T, B, 1)
    want1 = p.want.float()
    c = xattn_case(p.D, 8, Te, T, B, 1, y=want1)
    want = ref_xattn(c, p.want)
    res = {}
    for guarded in (False, True):
        what = f"attn_xattn T {T}, B {B}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        U, Wf, cc = fold(lib, L, c, what)
        qd, out = L.inp("qkv", p.qkv), L.out("out", B * T, p.D, fill=p.y0)
        a = proj_args(lib, L, p, out)
        x = apply_args(lib, L, c, out, U, Wf, cc)
        lib.check(lib.load().mdt_op_attn_xattn(C.byref(a), qd.ptr, qd.ld, C.byref(x), hd, T, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        res[guarded] = out.host()
    assert_close(res[True], want, what=what, **TOL_XATTN)
    assert same_bits(res[True], res[False]), f"{what}: differs from the dense call's bits"


# ------------------------------------------------------------------------------------------------
# LayerNorm, the action head, the action embedding
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("D", [16, 128, 500, 512])
def test_layernorm_rows(lib, D, M, with_bias):
    """mdt_op_layernorm (dense rows: the op has no stride): D below one float4 per lane, ragged (500) and at the limit; M = 5 is
    one row into a second workgroup."""
    g = seeded("layernorm", D, M)
    x, w, b = torch.randn(M, D, generator=g) * 4 - 1, torch.randn(D, generator=g), torch.randn(D, generator=g)
    res = {}
    for guarded in (False, True):
        what = f"layernorm {M} x {D}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        xd, wd, bd, out = L.inp("x", x), L.inp("w", w), L.inp("b", b), L.out("out", M, D)
        lib.check(lib.load().mdt_op_layernorm(xd.ptr, wd.ptr, bd.ptr if with_bias else None, out.ptr, M, D, stream()))
        L.check(what)
        out.check(what + ": out", written=True)
        res[guarded] = out.host()
    assert_close(res[True], F.layer_norm(x.double(), (D,), w.double(), b.double() if with_bias else None, 1e-5), what=what, **TOL_LAYERNORM)
    assert same_bits(res[True], res[False]), f"{what}: differs from the dense call's bits"


def run_head(lib, guarded, mode, A, D, M, sigma_stride=1, alias=False, no_ln=0, parts=1, what=""):
    """One mdt_op_head call -> {"out": ..., "y_next": ...} on the host, and the float64 values."""
    g = seeded("head", mode, A, D, M, sigma_stride, no_ln, parts)
    T, sd = 3, 0.5
    nb = (M + T - 1) // T
    slabs = torch.randn(parts, M, D, generator=g) * 2
    y = slabs[0].clone()
    for s in range(1, parts):
        y = y + slabs[s]
    lw, lb = torch.randn(D, generator=g) * 0.1 + 1, torch.randn(D, generator=g) * 0.1
    Wp, bp = torch.randn(A, D, generator=g) / 20, torch.randn(A, generator=g)
    WaT, ba = torch.randn(A, D, generator=g), torch.randn(D, generator=g)
    x = torch.randn(M, A, generator=g) * 10
    sigma = torch.rand(nb if sigma_stride else 1, generator=g) * 20 + 0.05
    step = torch.tensor([0.3, 0.7, 2.5])
    ddim = mode == "ddim"
    L = Lay(guarded)
    if alias:
        yd = L.out("y", M, D, fill=y)
    else:
        yd = L.inp("y", slabs if parts > 1 else y, gap=1024)
    o = {k: L.inp(k, v) for k, v in dict(ln_w=lw, ln_b=lb, Wp=Wp, bp=bp, x=x, step=step, Wa=WaT, ba=ba).items()}
    sg = L.inp("sigma", sigma.reshape(-1, 1), pad=max(sigma_stride, 1) - 1, fixed=True)
    out = L.out("out", M, A)
    yn = yd if alias else (L.out("y_next", M, D) if ddim else None)
    a = lib.HeadArgs()
    a.y, a.ln_w, a.ln_b, a.Wp, a.bp, a.x = yd.ptr, o["ln_w"].ptr, o["ln_b"].ptr, o["Wp"].ptr, o["bp"].ptr, o["x"].ptr
    a.sigma, a.sigma_stride, a.out = sg.ptr, sigma_stride, out.ptr
    a.M, a.D, a.A, a.rows_per_sample, a.mode, a.sigma_data, a.step = M, D, A, T, lib.HEAD[mode], sd, o["step"].ptr
    a.no_ln = no_ln
    if yn is not None:
        a.y_next, a.Wa, a.ba = yn.ptr, o["Wa"].ptr, o["ba"].ptr
    if parts > 1:
        a.y_parts, a.y_part_stride = parts, yd.slab_stride
    lib.check(lib.load().mdt_op_head(C.byref(a), stream()))
    L.check(what)
    out.check(what + ": out", written=True)
    got = {"out": out.host()}
    if yn is not None:
        yn.check(what + ": y_next", written=True)
        got["y_next"] = yn.host()
    h = y.double() if no_ln else F.layer_norm(y.double(), (D,), lw.double(), lb.double(), 1e-5)
    Fv = h @ Wp.double().T + bp.double()
    s = (sigma.double()[torch.arange(M) // T] if sigma_stride else sigma.double().expand(M))[:, None]
    den = Fv * (s * sd / (s ** 2 + sd ** 2).sqrt()) + x.double() * (sd ** 2 / (s ** 2 + sd ** 2))
    want = {"out": {"raw": Fv, "denoised": den, "ddim": 0.3 * x.double() + 0.7 * den}[mode]}
    if yn is not None:
        want["y_next"] = (want["out"] / math.sqrt(2.5 ** 2 + sd ** 2)) @ WaT.double() + ba.double()
    return got, want


def check_head(lib, what, **kw):
    dense, _ = run_head(lib, False, what=what + " (dense)", **kw)
    got, want = run_head(lib, True, what=what, **kw)
    for k, w in want.items():
        assert_close(got[k], w, what=f"{what}: {k}", **TOL_HEAD)
        assert same_bits(got[k], dense[k]), f"{what}: {k} differs from the dense call's bits"


@pytest.mark.parametrize("mode", ["denoised", "ddim", "raw"])
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("D", [64, 384])
@pytest.mark.parametrize("A", [1, 8, 9, 16])
def test_action_head(lib, A, D, M, mode):
    """mdt_op_head in its three modes (DDIM with the next step's embedding into a separate y_next), both instantiations (A <= 8,
    A > 8), D below and above one float4 per lane, a last workgroup of one row."""
    check_head(lib, f"head {mode}, A {A}, D {D}, M {M}", mode=mode, A=A, D=D, M=M)


@pytest.mark.parametrize("option", ["sigma_stride 0", "sigma_stride 3", "y_next == y", "no_ln", "y_parts 2", "y_parts 4"])
@pytest.mark.parametrize("A,D,M", [(8, 384, 33), (1, 64, 1)])
def test_action_head_options(lib, option, A, D, M):
    """One sigma for the batch and sigma at a stride of 3 floats (the floats between hold the guard NaN), y_next aliasing y, the
    MLP head's no_ln rows, and rows read as the sum of 2 / 4 slabs y_part_stride apart with a guard-pattern gap."""
    kw = dict(mode="ddim", A=A, D=D, M=M)
    if option.startswith("sigma_stride"):
        kw["sigma_stride"] = int(option[-1])
    elif option == "y_next == y":
        kw["alias"] = True
    elif option == "no_ln":
        kw["no_ln"] = 1
    else:
        kw["parts"] = int(option[-1])
    check_head(lib, f"head, {option}, A {A}, D {D}, M {M}", **kw)


@pytest.mark.parametrize("with_sigma", [False, True])
@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("D", [64, 384])
@pytest.mark.parametrize("A", [1, 9, 16])
def test_action_embed(lib, A, D, M, with_sigma):
    """mdt_op_action_embed with and without c_in(sigma); sigma at a stride of 3 floats."""
    g = seeded("embed", A, D, M)
    T, sd = 3, 0.5
    x, WaT, ba = torch.randn(M, A, generator=g) * 30, torch.randn(A, D, generator=g), torch.randn(D, generator=g)
    sigma = torch.rand((M + T - 1) // T, generator=g) * 50 + 0.01
    res = {}
    for guarded in (False, True):
        what = f"action_embed A {A}, D {D}, M {M}, sigma {with_sigma}" + ("" if guarded else " (dense)")
        L = Lay(guarded)
        xd, Wd, bd, sg, y = L.inp("x", x), L.inp("WaT", WaT), L.inp("ba", ba), L.inp("sigma", sigma.reshape(-1, 1), pad=2, fixed=True), L.out("y", M, D)
        lib.check(lib.load().mdt_op_action_embed(xd.ptr, sg.ptr if with_sigma else None, sg.ld, sd, Wd.ptr, bd.ptr, y.ptr, M, A, D,
                                                 T, stream()))
        L.check(what)
        y.check(what + ": y", written=True)
        res[guarded] = y.host()
    cin = (1 / (sigma.double() ** 2 + sd ** 2).sqrt())[torch.arange(M) // T][:, None] if with_sigma else 1.0
    assert_close(res[True], (x.double() * cin) @ WaT.double() + ba.double(), what=what, **TOL_EMBED)
    assert same_bits(res[True], res[False]), f"{what}: differs from the dense call's bits"


# ------------------------------------------------------------------------------------------------
# the packers: bit-exact against the host packers of the tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(16, 32), (48, 96)])
def test_packers_write_their_image_and_nothing_else(lib, N, K):
    """mdt_op_pack_weight with n_off > 0 into a taller image (the tiles outside [n_off, n_off + n_rows) keep the canary),
    mdt_op_pack_weight_glu, mdt_op_pack_weight_split_rows and mdt_op_pack_weight_pair with n_off (tiles outside keep the canary),
    mdt_op_pair_from_packed: each image bit for bit the host packer's, source and image between guards."""
    Lh = lib.load()
    g = seeded("packers", N, K)
    W = torch.randn(N, K, generator=g) * torch.exp(2.0 * torch.randn(N, 1, generator=g))
    off, total = 16, N + 32
    words = lambda t: t.contiguous().view(torch.float32).reshape(-1)

    # fp32 fragment image, rows [off, off + N) of a (N + 32)-row image
    L = GuardedSet()
    src, img = L.inp("w", W), L.out("image", total * K // 256, 256, fill=canary(total * K // 256, 256))
    lib.check(Lh.mdt_op_pack_weight(src.ptr, N, K, img.ptr, off, total, stream()))
    torch.cuda.synchronize()
    L.check("pack_weight")
    want = canary(total * K)
    want[off * K:(off + N) * K] = torch.from_numpy(expected_pack(W))
    assert same_bits(img.host().reshape(-1), want), "pack_weight: image differs from the host packer's, or a tile outside the rows was touched"

    # SwishGLU image of a (2H = 2N, K) weight
    W2 = torch.randn(2 * N, K, generator=g)
    L = GuardedSet()
    src, img = L.inp("w", W2), L.out("image", 2 * N * K // 256, 256)
    lib.check(Lh.mdt_op_pack_weight_glu(src.ptr, 2 * N, K, img.ptr, stream()))
    torch.cuda.synchronize()
    L.check("pack_weight_glu")
    assert same_bits(img.host().reshape(-1), pack_glu(W2)), "pack_weight_glu: image differs from the host packer's"

    # bf16 split image, rows [off, off + N) of a taller one: 6 bytes per weight
    tall = torch.cat([torch.zeros(off, K), W, torch.zeros(16, K)])
    want = words(expected_pack_split(tall))
    lo, hi = off * K * 6 // 4, (off + N) * K * 6 // 4
    start = canary(want.numel())
    L = GuardedSet()
    src, img = L.inp("w", W), L.out("image", want.numel() // 64, 64, fill=start)
    lib.check(Lh.mdt_op_pack_weight_split_rows(src.ptr, N, K, img.ptr, off, stream()))
    torch.cuda.synchronize()
    L.check("pack_weight_split_rows")
    start[lo:hi] = want[lo:hi]
    assert same_bits(img.host().reshape(-1), start), "pack_weight_split_rows: image differs, or rows outside the range were touched"

    # fp16 pair image, column tiles off / 16 .. of a taller one (4 K + 1 bytes per row: K + 1 / 4 words)
    want = words(expected_pack_pair(tall)[0])
    per = 16 * K + 4                                           # words of one 16-row tile: its fragments and the trailer
    lo, hi = off // 16 * per, (off + N) // 16 * per
    start = canary(want.numel())
    L = GuardedSet()
    src, img = L.inp("w", W), L.out("image", want.numel() // 4, 4, fill=start)
    lib.check(Lh.mdt_op_pack_weight_pair(src.ptr, N, K, img.ptr, off, stream()))
    torch.cuda.synchronize()
    L.check("pack_weight_pair")
    start[lo:hi] = want[lo:hi]
    assert same_bits(img.host().reshape(-1), start), "pack_weight_pair: image differs, or tiles outside the range were touched"

    # ... and the same image from the fp32 fragment image
    want = words(expected_pack_pair(W)[0])
    L = GuardedSet()
    src, img = L.inp("packed", torch.from_numpy(expected_pack(W)).reshape(-1, 256)), L.out("image", want.numel() // 4, 4)
    lib.check(Lh.mdt_op_pair_from_packed(src.ptr, N, K, img.ptr, stream()))
    torch.cuda.synchronize()
    L.check("pair_from_packed")
    assert same_bits(img.host().reshape(-1), want), "pair_from_packed: image differs from the host packer's"
