"""The two-way fp16 pair split (include/mdt_hip_ops.h, mdt_op_pack_weight_pair ff.): the arithmetic emulated on the CPU, then the
pack kernels, the fused MLP launch, the LayerNorm GEMM, their range behaviour and the model-level calls on the MI355X."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import assert_close, cfg_of, inputs_of, load_fixture, params_of


# ------------------------------------------------------------------------------------------------
# the reference split, written out here
# ------------------------------------------------------------------------------------------------
def group_scale(mx):
    """Power-of-two scale of a group whose largest |x| is mx (fp32 tensor): mx * s in [2^14, 2^15) for normal maxima, exponent
    clamped to +-126 (zero / subnormal groups: 2^126)."""
    ex = (mx.contiguous().view(torch.int32) >> 23) & 255
    e = torch.clamp(141 - ex, -126, 126)
    return torch.ldexp(torch.ones_like(mx), e)


def pair_split(x, s):
    """x s = h1 + h2: h1 = fp16(x s), h2 = fp16(x s - h1), round to nearest both."""
    v = (x * s).float()
    h1 = v.half()
    h2 = (v - h1.float()).half()
    return h1, h2


# ------------------------------------------------------------------------------------------------
# CPU: the arithmetic (no GPU, no library)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [384, 512, 1536])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pair_split_arithmetic_is_no_worse_than_the_fp32_mfma_chain(K, seed):
    """Emulation of one contraction, 32 rows x 64 columns: rows scaled over e^+-4, weights N(0, 0.02^2).  Pair form: one scale per
    row and per 16-column tile, three exact products per k32 step (x2 w1, x1 w2, x1 w1), each added to the fp32 accumulator with one
    rounding.  fp32 form: the v_mfma_f32_16x16x4_f32 chain, one fp32 rounding per k4 step.  Against float64 the pair form's largest
    error must not exceed the chain's."""
    g = torch.Generator().manual_seed(1000 * K + seed)
    M, N = 32, 64
    x = torch.randn(M, K, generator=g) * torch.exp(8.0 * torch.rand(M, 1, generator=g) - 4.0)
    w = torch.randn(N, K, generator=g) * 0.02
    want = x.double() @ w.double().T

    acc = torch.zeros(M, N)
    for k in range(0, K, 4):
        acc = (acc.double() + x[:, k:k + 4].double() @ w[:, k:k + 4].double().T).float()
    err_chain = (acc.double() - want).abs().max().item()

    sx = group_scale(x.abs().amax(1, keepdim=True))
    sw = group_scale(w.reshape(N // 16, 16 * K).abs().amax(1)).repeat_interleave(16).reshape(N, 1)
    x1, x2 = pair_split(x, sx)
    w1, w2 = pair_split(w, sw)
    acc = torch.zeros(M, N)
    for k in range(0, K, 32):
        sl = slice(k, k + 32)
        for a, b in ((x2, w1), (x1, w2), (x1, w1)):
            acc = (acc.double() + a[:, sl].double() @ b[:, sl].double().T).float()
    got = acc.double() / (sx.double() * sw.double().T)
    err_pair = (got - want).abs().max().item()
    print(f"K={K} seed={seed}: pair {err_pair:.3e}  fp32 chain {err_chain:.3e}  ratio {err_pair / err_chain:.3f}")
    assert err_pair <= err_chain


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def dev(t):
    return t.to("cuda", torch.float32).contiguous()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(lib, W):
    N, K = W.shape
    Wd = dev(W)
    P = torch.zeros(N * K, device="cuda")
    lib.check(lib.load().mdt_op_pack_weight(Wd.data_ptr(), N, K, P.data_ptr(), 0, N, stream()))
    return P


def image_bytes(lib, N, K):
    n = lib.load().mdt_op_pair_image_bytes(N, K)
    assert n == 4 * N * K + N
    return n


def pack_pair(lib, W, ranges=None):
    """fp16 pair image of a (N, K) weight through the library, in one piece or row range by row range."""
    N, K = W.shape
    Wd = dev(W)
    P = torch.zeros(image_bytes(lib, N, K), dtype=torch.uint8, device="cuda")
    for lo, hi in (ranges or ((0, N),)):
        lib.check(lib.load().mdt_op_pack_weight_pair(Wd[lo:hi].contiguous().data_ptr(), hi - lo, K, P.data_ptr(), lo, stream()))
    torch.cuda.synchronize()
    return P


def expected_pack_pair(W):
    """The documented image: column tile nt = K / 32 steps x 2 parts x 1 KiB (lane l's eight fp16 = the part of
    W[16 nt + l % 16][32 kk + 16 h + 4 (l / 16) + e] at slot 4 h + e), then the trailer {fp32 scale, 0, 0, 0}."""
    N, K = W.shape
    s = group_scale(W.reshape(N // 16, 16 * K).abs().amax(1))
    h = pair_split(W, s.repeat_interleave(16).reshape(N, 1))
    frag = torch.zeros(N // 16, K // 32, 2, 64, 8, dtype=torch.float16)
    for pi, P in enumerate(h):
        t = P.reshape(N // 16, 16, K // 32, 2, 4, 4)                                       # nt, ni, kk, h, g, e
        frag[:, :, pi] = t.permute(0, 2, 4, 1, 3, 5).reshape(N // 16, K // 32, 64, 8)      # lane = ni + 16 g, slot = 4 h + e
    body = frag.reshape(N // 16, -1).contiguous().view(torch.uint8)
    tail = torch.zeros(N // 16, 4)
    tail[:, 0] = s
    return torch.cat([body, tail.view(torch.uint8)], dim=1).reshape(-1), s


def unpack_pair(image, N, K):
    """-> (h1 + h2 as float64 (N, K), scales (N / 16,))"""
    rows = image.cpu().reshape(N // 16, -1)
    body = rows[:, :-16].contiguous().view(torch.float16).reshape(N // 16, K // 32, 2, 64, 8)
    s = rows[:, -16:].contiguous().view(torch.float32)[:, 0]
    parts = body.double()
    assert torch.isfinite(parts).all() and torch.isfinite(s).all(), "a part or a scale is not finite"
    v = parts.sum(dim=2)                                                                    # nt, kk, lane, slot
    return v.reshape(N // 16, K // 32, 4, 16, 2, 4).permute(0, 3, 1, 4, 2, 5).reshape(N, K), s


@gpu
@pytest.mark.parametrize("N,K", [(16, 32), (48, 96), (1152, 384)])
def test_pack_weight_pair_layout_error_bound_and_edges(lib, N, K):
    """mdt_op_pack_weight_pair: the documented layout bit for bit against the host packer; every element within 2^-21 of its tile's
    largest |W|; a zero tile, a tile reaching 3e38 and a tile of fp32 subnormals all give finite parts and scales; packing by row
    ranges and from the fp32 fragment image give the one-piece image."""
    g = torch.Generator().manual_seed(N + K)
    W = torch.randn(N, K, generator=g) * torch.exp(3.0 * torch.randn(N, 1, generator=g))
    sub = torch.zeros(16, K)
    if N >= 48:
        W[0:16] = 0.0
        W[16:32] *= 3e38 / W[16:32].abs().max()
        sub = (torch.randint(1, 1 << 22, (16, K), generator=g, dtype=torch.int32).view(torch.float32)
               * (1 - 2 * torch.randint(0, 2, (16, K), generator=g)).float())
        W[32:48] = sub
        assert sub.abs().max() < 1.1754944e-38 and torch.equal(W[32:48], sub)
    got = pack_pair(lib, W)
    want, s_want = expected_pack_pair(W)
    v, s = unpack_pair(got, N, K)
    assert torch.equal(s, s_want), "tile scales differ from the documented rule"
    tile_max = W.reshape(N // 16, 16 * K).abs().amax(1).double().repeat_interleave(16).reshape(N, 1)
    back = v / s.double().repeat_interleave(16).reshape(N, 1)
    err = (W.double() - back).abs()
    print(f"N={N} K={K}: largest error / tile max = {(err / tile_max.clamp_min(1e-300)).max().item():.3e} (bound {2.0 ** -21:.3e})")
    assert (err <= 2.0 ** -21 * tile_max).all(), "an element is further than 2^-21 of its tile's maximum from the weight"
    assert torch.equal(got.cpu(), want), "pair image differs from the documented layout"
    third = max(16, (N // 3) // 16 * 16)
    ranges = ((0, N),) if N == 16 else ((0, third), (third, 2 * third), (2 * third, N)) if N > 2 * third else ((0, third), (third, N))
    assert torch.equal(pack_pair(lib, W, ranges), got), "row-range packs differ from the one-piece image"
    Q = torch.zeros_like(got)
    lib.check(lib.load().mdt_op_pair_from_packed(pack(lib, W).data_ptr(), N, K, Q.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert torch.equal(Q, got), "the image made from the fp32 fragment image differs"


def _gemm_args(lib, keep, A, lda, N, K, M, out=None, ldo=0, bias=None, Wp=None):
    a = lib.GemmArgs()
    a.A, a.lda, a.M, a.N, a.K = A.data_ptr(), lda, M, N, K
    if Wp is not None:
        a.Wp = Wp.data_ptr()
    if out is not None:
        a.out, a.ldo = out.data_ptr(), ldo
    if bias is not None:
        bd = dev(bias); keep.append(bd); a.bias = bd.data_ptr()
    a.shift_off = a.scale_off = a.gate_off = -1
    a.rows_per_sample, a.gin, a.gout, a.goff = 1, 1, 1, 0
    return a


def run_mlp(lib, x, W1, W2, ln_w, ln_b, b1, b2, pro, gate, mod, T, pair, images=None):
    """-> the sublayer's output (slabs summed in order, on the host).  pro: 'plain' | 'bcast' | 'rows'; mod rows hold
    shift | scale | gate at 0, D, 2 D."""
    M, D = x.shape
    keep = []
    xd = dev(x)
    S = 4 * D // 512
    parts = torch.full((S, M, D), float("nan"), device="cuda")
    P1, P2 = (None, None) if pair else (pack(lib, W1), pack(lib, W2))
    f = _gemm_args(lib, keep, xd, D, 4 * D, D, M, bias=b1, Wp=P1)
    p = _gemm_args(lib, keep, xd, D, D, 4 * D, M, bias=b2, Wp=P2)
    p.ldo = D
    f.ln, f.act = 1, lib.ACT["gelu"]
    lw = dev(ln_w); keep.append(lw); f.ln_w = lw.data_ptr()
    if ln_b is not None:
        lb = dev(ln_b); keep.append(lb); f.ln_b = lb.data_ptr()
    md = dev(mod); keep.append(md)
    stride = 3 * D if pro == "rows" else 0
    if pro != "plain":
        f.mod, f.mod_stride, f.shift_off, f.scale_off, f.rows_per_sample = md.data_ptr(), stride, 0, D, T
    if gate:
        p.mod, p.mod_stride, p.gate_off, p.rows_per_sample = md.data_ptr(), stride, 2 * D, T
    n = C.c_int32(0)
    if pair:
        S1, S2 = images if images else (pack_pair(lib, W1), pack_pair(lib, W2))
        lib.check(lib.load().mdt_op_mlp_pair(C.byref(f), C.byref(p), S1.data_ptr(), S2.data_ptr(), parts.data_ptr(), M * D, C.byref(n), stream()))
    else:
        lib.check(lib.load().mdt_op_mlp(C.byref(f), C.byref(p), parts.data_ptr(), M * D, C.byref(n), stream()))
    torch.cuda.synchronize()
    assert n.value == S
    got = parts[0].clone()
    for s in range(1, S):
        got += parts[s]
    return got.cpu()


def ref_mlp(x, W1, W2, ln_w, ln_b, b1, b2, shift=None, scale=None, gate=None):
    x = x.double()
    h = F.layer_norm(x, (x.shape[1],), ln_w.double(), None if ln_b is None else ln_b.double(), 1e-5)
    if shift is not None:
        h = shift.double() + h * scale.double()
    u = h @ W1.double().T + (0 if b1 is None else b1.double())
    v = F.gelu(u) @ W2.double().T + (0 if b2 is None else b2.double())
    return x + (v if gate is None else gate.double() * v)


def mlp_case(M, D, pro, seed):
    g = torch.Generator().manual_seed(seed)
    T = 10 if M % 10 == 0 else 11
    x = torch.randn(M, D, generator=g) * 1.5 + 0.2
    W1 = torch.randn(4 * D, D, generator=g) / math.sqrt(D)
    W2 = torch.randn(D, 4 * D, generator=g) / math.sqrt(4 * D)
    lw, lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    b1, b2 = torch.randn(4 * D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    nb = M // T if pro == "rows" else 1
    mod = torch.randn(nb, 3 * D, generator=g) * 0.5
    pick = (lambda o: mod[:, o:o + D].repeat_interleave(T, 0)) if pro == "rows" else (lambda o: mod[:, o:o + D])
    return T, x, W1, W2, lw, lb, b1, b2, mod, pick


def check_gate(err_pair, err_fp32, what):
    """the project's gate for split forms: the error against float64 within 1.5x the fp32 launch's on the same inputs + 1e-6"""
    print(f"{what}: pair {err_pair:.3e}  fp32 {err_fp32:.3e}  ratio {err_pair / max(err_fp32, 1e-30):.3f}")
    assert err_pair <= 1.5 * err_fp32 + 1e-6, f"{what}: max error {err_pair:.3g} against the fp32 launch's {err_fp32:.3g}"


@gpu
@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("pro", ["plain", "bcast", "rows"])
@pytest.mark.parametrize("M", [33, 70])
@pytest.mark.parametrize("D", [384, 512])
def test_fused_mlp_in_its_fp16_pair_form_keeps_fp32_accuracy(lib, D, M, pro, gate):
    """mdt_op_mlp_pair: ragged second row tile (33 rows), samples of 10 rows straddling the 32-row tiles (70 rows); every prologue,
    gate on and off.  Against float64 within 1.5x the fp32 launch's error + 1e-6, not the fp32 launch's bits, the same bits twice."""
    T, x, W1, W2, lw, lb, b1, b2, mod, pick = mlp_case(M, D, pro, 7 * M + D + len(pro) + gate)
    ref = {}
    if pro != "plain":
        ref.update(shift=pick(0), scale=pick(D))
    if gate:
        ref.update(gate=pick(2 * D))
    want = ref_mlp(x, W1, W2, lw, lb, b1, b2, **ref)
    fp32 = run_mlp(lib, x, W1, W2, lw, lb, b1, b2, pro, gate, mod, T, pair=False)
    images = (pack_pair(lib, W1), pack_pair(lib, W2))
    got = run_mlp(lib, x, W1, W2, lw, lb, b1, b2, pro, gate, mod, T, pair=True, images=images)
    again = run_mlp(lib, x, W1, W2, lw, lb, b1, b2, pro, gate, mod, T, pair=True, images=images)
    assert torch.isfinite(got).all()
    check_gate((got.double() - want).abs().max().item(), (fp32.double() - want).abs().max().item(), f"pair mlp {M}x{D} {pro} gate={gate}")
    assert not torch.equal(got, fp32), "the pair form did not run"
    assert torch.equal(got, again), "two launches on the same inputs differ"


def run_ln_gemm(lib, slabs, W, b, lw, lb, pair, image=None):
    XP, M, D = slabs.shape
    N = W.shape[0]
    keep = []
    sd = dev(slabs)
    out = torch.full((M, N), float("nan"), device="cuda")
    merged = torch.full((M, D), float("nan"), device="cuda")
    a = _gemm_args(lib, keep, sd, D, N, D, M, out=out, ldo=N, bias=b, Wp=pack(lib, W))
    a.ln = 1
    for name, t in (("ln_w", lw), ("ln_b", lb)):
        td = dev(t); keep.append(td); setattr(a, name, td.data_ptr())
    if XP > 1:
        a.a_parts, a.a_part_stride, a.a_merged = XP, M * D, merged.data_ptr()
    if pair:
        a.Wp_pair = image.data_ptr()
        lib.check(lib.load().mdt_op_gemm_ln_pair(C.byref(a), stream()))
    else:
        lib.check(lib.load().mdt_op_gemm(C.byref(a), stream()))
    torch.cuda.synchronize()
    return out.cpu(), merged.cpu()


@gpu
@pytest.mark.parametrize("XP", [1, 3])
def test_layernorm_gemm_in_its_fp16_pair_form_keeps_fp32_accuracy(lib, XP):
    """mdt_op_gemm_ln_pair at N = 1152, K = 384, M = 70 (the decoder's qkv product), rows from one array and from three slabs, the image
    packed in three row ranges like the stacked query | key | value: the gate of the fused MLP test; a_merged is the slab-order sum."""
    M, N, D = 70, 1152, 384
    g = torch.Generator().manual_seed(M + N + XP)
    slabs = torch.randn(XP, M, D, generator=g)
    W, b = torch.randn(N, D, generator=g) / math.sqrt(D), torch.randn(N, generator=g)
    lw, lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    summed = slabs[0].clone()
    for s in range(1, XP):
        summed = summed + slabs[s]
    want = F.layer_norm(summed.double(), (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()
    image = pack_pair(lib, W, ((0, D), (D, 2 * D), (2 * D, N)))
    fp32, m0 = run_ln_gemm(lib, slabs, W, b, lw, lb, pair=False)
    got, m1 = run_ln_gemm(lib, slabs, W, b, lw, lb, pair=True, image=image)
    again, _ = run_ln_gemm(lib, slabs, W, b, lw, lb, pair=True, image=image)
    if XP > 1:
        assert torch.equal(m1, summed), "a_merged is not the slab-order sum"
    check_gate((got.double() - want).abs().max().item(), (fp32.double() - want).abs().max().item(), f"pair LayerNorm GEMM, {XP} slab(s)")
    assert not torch.equal(got, fp32), "the pair form did not run"
    assert torch.equal(got, again), "two launches on the same inputs differ"


@gpu
def test_fp16_pair_forms_over_the_fp32_range(lib):
    """Rows scaled by 1e4 and 1e-4 and one zero row in the same 32-row tile; c_fc weights scaled so that hidden activations exceed 1e6
    (far beyond fp16's 65504): finite results inside the gate.  One row holding Inf makes that row non-finite, and no other.
    The LayerNorm GEMM takes the same rows among 70 -- the row count at which its gate is set above: below ~60 column tiles
    mdt_op_gemm's fp32 form is the split-K small-M kernel, whose eight 12-step chains are more accurate than any full-K form (at
    33 rows the pair form's error measured 2.1-2.8x that kernel's, and 0.6x the wide tiles' it replaces)."""
    M, D = 33, 384
    T, x, W1, W2, lw, lb, b1, b2, mod, pick = mlp_case(M, D, "plain", 99)
    x[3] *= 1e4
    x[4] *= 1e-4
    x[5] = 0.0
    W1 = W1 * 1e6
    want = ref_mlp(x, W1, W2, lw, lb, b1, b2)
    hidden = F.gelu(F.layer_norm(x.double(), (D,), lw.double(), lb.double(), 1e-5) @ W1.double().T + b1.double())
    assert hidden.abs().max() > 1e6
    fp32 = run_mlp(lib, x, W1, W2, lw, lb, b1, b2, "plain", False, mod, T, pair=False)
    got = run_mlp(lib, x, W1, W2, lw, lb, b1, b2, "plain", False, mod, T, pair=True)
    assert torch.isfinite(got).all(), "a finite input gave a non-finite output"
    check_gate((got.double() - want).abs().max().item(), (fp32.double() - want).abs().max().item(), "pair mlp over the range")
    xi = x.clone()
    xi[7, 11] = float("inf")
    bad = run_mlp(lib, xi, W1, W2, lw, lb, b1, b2, "plain", False, mod, T, pair=True)
    fin = torch.isfinite(bad).all(dim=1)
    assert not torch.isfinite(bad[7]).any() and fin[:7].all() and fin[8:].all(), "an Inf in row 7 must reach row 7 and no other row"
    keep = torch.arange(M) != 7
    assert torch.equal(bad[keep], got[keep]), "the other rows changed"

    # the LayerNorm GEMM on the same rows (LayerNorm takes the row scales out: its range case is the weight's)
    N = 1152
    g = torch.Generator().manual_seed(5)
    W, b = torch.randn(N, D, generator=g) * 1e5, torch.randn(N, generator=g)
    W[16:32] *= 1e-9
    M = 70
    x = torch.cat([x, torch.randn(M - x.shape[0], D, generator=g) * 1.5 + 0.2])
    xi = torch.cat([xi, x[xi.shape[0]:]])
    slabs = x.reshape(1, M, D)
    want = F.layer_norm(x.double(), (D,), lw.double(), lb.double(), 1e-5) @ W.double().T + b.double()
    fp32, _ = run_ln_gemm(lib, slabs, W, b, lw, lb, pair=False)
    got, _ = run_ln_gemm(lib, slabs, W, b, lw, lb, pair=True, image=pack_pair(lib, W))
    assert torch.isfinite(got).all()
    check_gate((got.double() - want).abs().max().item(), (fp32.double() - want).abs().max().item(), "pair LayerNorm GEMM over the range")
    bad, _ = run_ln_gemm(lib, xi.reshape(1, M, D), W, b, lw, lb, pair=True, image=pack_pair(lib, W))
    fin = torch.isfinite(bad).all(dim=1)
    assert not torch.isfinite(bad[7]).any() and fin[:7].all() and fin[8:].all(), "an Inf in row 7 must reach row 7 and no other row"


# ------------------------------------------------------------------------------------------------
# model level: B = 80 (800 decoder rows: the first launches from 768 rows on), 3 DDIM steps
# ------------------------------------------------------------------------------------------------
_ORACLE = {}


def model_case(fixture):
    """(meta, model, state, goal, noise, sigmas, oracle actions): built once per configuration and shared, unchanged, by the tests"""
    if fixture not in _ORACLE:
        from oracle import mdt_oracle as O
        from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
        meta, _ = load_fixture(fixture)
        meta = dict(meta, B=80, input_seed=4242)
        cfg, P = cfg_of(meta), params_of(meta)
        model = GCDenoiser(cfg, sigma_data=0.5)
        model.load_state_dict(P, strict=True)
        model = model.cuda().eval()
        state, goal, noise = inputs_of(meta)
        sig = O.get_sigmas_exponential(3, 0.01, 80.0)
        want = O.sample_ddim(P, cfg, state, noise * 80.0, goal, sig, arch=meta["arch"], hoist=True)
        state = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
        _ORACLE[fixture] = (meta, model, state, goal.cuda(), noise.cuda(), sig, want)
    return _ORACLE[fixture]


@gpu
@pytest.mark.parametrize("fixture", ["g3_b256_lang.npz", "g3_b8_mdt.npz"], ids=["mdtv_default", "mdt_default"])
def test_model_level_calls_run_the_pair_form(lib, fixture):
    """sample_ddim at B = 80 against the oracle at the parity gate (rtol 1e-3, atol 1e-4); against the same call with the fp32 launches
    (mdt_op_set_mlp_split(0)) at 1e-4 / 1e-4 and not its bits; the same bits call after call; and after two optimizer steps the bits
    of a freshly loaded model, so no stale image is read."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd import synthetic
    meta, model, state, goal, noise, sig, want = model_case(fixture)
    L = lib.load()
    L.mdt_op_set_mlp_split(1)
    try:
        with torch.no_grad():
            got = gs.sample_ddim(model, state, noise * 80.0, goal, sig).clone()
            again = gs.sample_ddim(model, state, noise * 80.0, goal, sig).clone()
            L.mdt_op_set_mlp_split(0)
            fp32 = gs.sample_ddim(model, state, noise * 80.0, goal, sig).clone()
            L.mdt_op_set_mlp_split(1)
        assert_close(got.cpu(), want, what="pair form against the oracle")
        assert torch.equal(got, again), "two calls differ"
        assert not torch.equal(got, fp32), "the pair launches did not run at B = 80"
        print(f"{fixture}: largest |pair - fp32| = {(got - fp32).abs().max().item():.3e}")
        assert_close(got.cpu(), fp32.cpu(), rtol=1e-4, atol=1e-4, what="pair against fp32 launches")

        cfg = cfg_of(meta)
        trained = GCDenoiser(cfg, sigma_data=0.5).cuda()
        trained.load_state_dict(model.state_dict())
        with torch.no_grad():
            trained.eval()
            before = gs.sample_ddim(trained, state, noise * 80.0, goal, sig).clone()   # images of the initial weights in use
        assert torch.equal(before, got)
        trained.train()
        opt = torch.optim.SGD(trained.parameters(), lr=0.05)
        tstate, tgoal, _ = inputs_of(dict(meta, B=16, input_seed=1))
        tstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in tstate.items()}
        li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(16, cfg, 2).items()}
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, _ = trained.loss(tstate, li["actions"], tgoal.cuda(), li["noise_train"], li["sigma"])
            loss.backward()
            opt.step()
        trained.eval()
        with torch.no_grad():
            after = gs.sample_ddim(trained, state, noise * 80.0, goal, sig).clone()
            fresh = GCDenoiser(cfg, sigma_data=0.5).cuda().eval()
            fresh.load_state_dict(trained.state_dict())
            ref = gs.sample_ddim(fresh, state, noise * 80.0, goal, sig).clone()
    finally:
        L.mdt_op_set_mlp_split(-1)
    assert not torch.equal(after, before), "the optimizer steps did not change the sampler's output"
    assert torch.equal(after, ref), "sampling after optimizer steps read stale pair images"
