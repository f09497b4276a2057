"""Shared by tests/test_gpu_score_ops.py and tests/test_cpu_score_ops_reference.py: the three kernels of mdt_denoising_score
(mdt_policy_amd/csrc/mdt_score.hip: k_score_prep, k_score_repeat, k_score_reduce; hooks mdt_op_score_* of
include/mdt_hip_debug.h) restated in numpy from the header's formulas, an fp32 emulation of the two that compute, their cases and
their error bounds.

Indices.  B observations, K chunks each, S levels, M noise rows per level; decoder sample j = ((b S + s) K + k) M + m is chunk
r = b K + k at level s with noise row i = s M + m.  ``*_ref`` are float64 and take ``defect``, one planted mistake of DEFECTS;
``*_emulate`` run the kernel's own operation order in fp32 (numpy float32 arithmetic is IEEE, one rounding per operation; a fused
multiply-add is the float64 product -- exact, 48 bits -- plus the addend, rounded to fp32).

Bounds.  u = 2^-24, g(n) = n u / (1 - n u) (n roundings compose to at most g(n), Higham's gamma), magnitudes in float64, the counts
of tests/steer_ops_cases.py for the EDM scalings: den2 = sigma^2 + sd^2 has 2 roundings (two squares, then a sum of positives).
  prep   noised = x0 + sigma n: product 1 + sum 1 = 2 on X = |x0| + |sigma n| (the sum may cancel: X, not |noised|)
         c_in = 1 / sqrt(den2): 2 / 2 + 1 of the root + 1 of the division = 3;  xv = noised c_in: 2 + 3 + 1 = 6
         y[d] = ba[d] + sum_c xv[c] WaT[c, d] as A fused multiply-adds from the bias: a term sees its own fma and the later ones, at
         most A                                                          g(A + 6) (|ba[d]| + sum_c X[c] c_in |WaT[c, d]|)
  reduce the three level constants: c_x = sigma / den2: 2 + 1 = 3;  c_n = sd^2 / den2: 1 + 2 + 1 = 4;  c_f = sd / sqrt(den2):
         2 / 2 + 1 + 1 = 3;  c_w = w / M: 1 (M is exact)
         q = c_x x0 - c_n n - c_f F: a product adds 1 (4, 5, 4), the two subtractions 1 each on what they see: at most 5 + 2 = 7 on
         Q = |c_x x0| + |c_n n| + |c_f F| (q may cancel: Q, not |q|);  the square: |q'^2 - q^2| <= ((1 + g(7))^2 - 1) Q^2 <= g(14) Q^2,
         + 1 where the square is rounded on its own (inside an fma it is not: the count holds either way)
         the lane sum over e = lane, lane + 64, ..: ceil(E / 64) fused adds, a term sees at most that many;  the sample's sum times
         c_w (1) in one fma (1) and the later fmas of its wave: ceil(S M / 4) in all;  the xor butterfly: 6 sums;  the tree
         (p0 + p1) + (p2 + p3): 2
                                        g(24 + ceil(E / 64) + ceil(S M / 4)) sum_s (w_s / M) sum_m sum_e Q^2
         (sum |terms| with Q for |q|: no smaller than -score).  All-zero weights: bound 0, the score compares equal to 0.
  noised, the rows' and contexts' sigma, every row k_score_repeat copies: bits.
A contracted multiply-add has one rounding fewer: the counts hold with or without it.  Nothing here was fitted to a device result."""
import math

import numpy as np

from tests.steer_ops_cases import U, as_f32, draw, f64, g, outside, ratio, rng_of, same_bits32  # noqa: F401  (re-exported)

SD = 0.5
SMIN, SMAX = 0.001, 80.0
THREADS, MAX_BLOCKS, SCORE_MAX = 256, 4096, 64
CAP = THREADS * MAX_BLOCKS     # the indices of one trip of the grid-stride loops of k_score_prep and k_score_repeat
EXTREME = (1e4, 1e-6)          # descending like the others: 1 / c_in spans ten decades

# name -> what the planted mistake is
DEFECTS = {
    "a_cn": "c_n formed as sigma^2 / (sigma^2 + sd^2)",
    "b_no_m": "the weight not divided by M",
    "c_swap_ks": "K and S swapped when a sample's index is decomposed",
    "d_noise_m": "the noise row taken as m, not s M + m",
    "e_tail": "the E mod 64 tail elements dropped",
    "f_wave3": "the fourth wave's partial left out (the samples i % 4 == 3)",
    "g_cin": "c_in from sigma alone",
    "h_ctx_k": "ctx_sig written at b S + k: under the writer's own selection k == 0 every level of an observation lands in slot b S "
               "(the last level wins) and the other S - 1 slots stay unwritten",
}
PREP_DEFECTS = ("c_swap_ks", "d_noise_m", "g_cin", "h_ctx_k")
REDUCE_DEFECTS = ("a_cn", "b_no_m", "c_swap_ks", "d_noise_m", "e_tail", "f_wave3")


def levels_of(S, extreme=False):
    """fp32 levels: log-uniform from 80 down to 0.001, both included (one level: 0.001); ``extreme``: 1e4 and 1e-6."""
    if extreme:
        assert S == 2
        return np.array(EXTREME, dtype=np.float32)
    if S == 1:
        return np.array([SMIN], dtype=np.float32)
    return np.exp(np.linspace(math.log(SMAX), math.log(SMIN), S)).astype(np.float32)


def trapezoid(levels):
    """Half the distance in ln sigma to each neighbour (one level: 1), rounded to fp32."""
    ln = np.log(np.asarray(levels, dtype=np.float64))
    if ln.size == 1:
        return np.ones(1, dtype=np.float32)
    d = np.abs(np.diff(ln))
    return (0.5 * (np.concatenate([[0.0], d]) + np.concatenate([d, [0.0]]))).astype(np.float32)


def weights_of(kind, levels):
    w = trapezoid(levels)
    if kind == "some_zero":      # every odd level weighs nothing
        w[1::2] = 0
    elif kind == "all_zero":
        w[:] = 0
    elif kind == "one_1e6":      # an odd level: with M = 2 one of its samples is the fourth wave's
        w[min(len(w) // 2 | 1, len(w) - 1)] = 1e6
    else:
        assert kind == "trapezoid"
    return w


def sample_index(B, S, K, M, defect=None):
    """(b, s, k, m) of every decoder sample j."""
    j = np.arange(B * S * K * M)
    m, j = j % M, j // M
    if defect == "c_swap_ks":
        s, j = j % S, j // S
        return j // K, s, j % K, m
    k, j = j % K, j // K
    return j // S, j % S, k, m


# ---- k_score_prep ---------------------------------------------------------------------------------------------------------------
def prep_case(B, S, K, M, Ta, A, D, ctx=True, extreme=False):
    return dict(B=B, S=S, K=K, M=M, Ta=Ta, A=A, D=D, ctx=ctx, extreme=extreme)


PREP_CASES = {
    "ones": prep_case(1, 1, 1, 1, 1, 1, 16),
    "distinct": prep_case(2, 3, 5, 7, 3, 7, 64),                 # four distinct extents: every index swap shows
    "distinct_no_ctx": prep_case(2, 3, 5, 7, 3, 7, 64, ctx=False),
    **{f"a{A}_d{D}": prep_case(2, 3, 2, 2, 3, A, D, ctx=(A + D) % 3 != 0) for A in (1, 7, 17, 64) for D in (16, 144, 384, 512)},
    "ta64": prep_case(1, 2, 2, 1, 64, 7, 64),
    "s64_m1": prep_case(1, 64, 2, 1, 2, 3, 16),
    "s1_m64": prep_case(1, 1, 2, 64, 2, 3, 16),
    "extreme_levels": prep_case(2, 2, 3, 2, 3, 7, 64, extreme=True),
    "past_grid_cap": prep_case(2, 5, 41, 2, 10, 3, 512),         # 8200 rows x 128 threads a row > 4096 x 256
}


def prep_operands(c, key="prep"):
    r = rng_of(key, sorted(c.items()))
    return {"x0": draw(r, c["B"] * c["K"], c["Ta"], c["A"]), "noise": draw(r, c["S"] * c["M"], c["Ta"], c["A"]),
            "WaT": draw(r, c["A"], c["D"]), "ba": draw(r, c["D"]), "levels": levels_of(c["S"], c["extreme"])}


def _prep_rows(c, op, defect, dtype):
    """x0 row, noise row and sigma of every decoder sample, in ``dtype``."""
    b, s, k, m = sample_index(c["B"], c["S"], c["K"], c["M"], defect)
    x = op["x0"].astype(dtype)[b * c["K"] + k]
    n = op["noise"].astype(dtype)[m if defect == "d_noise_m" else s * c["M"] + m]
    return (b, s, k, m), x, n, op["levels"].astype(dtype)[s]


def _ctx_sig(c, idx, sg, defect):
    """(B S) values, NaN where nothing is written: the (k, m) = (0, 0) sample of (b, s) writes its sigma.  The defect keeps that
    selection and only indexes with k, so it is k == 0 always: slot b S takes every level in turn, no other slot is written."""
    b, s, k, m = idx
    out = np.full(c["B"] * c["S"], np.nan)
    sel = (k == 0) & (m == 0)
    out[(b * c["S"] + (k if defect == "h_ctx_k" else s))[sel]] = sg[sel]
    return out


def prep_ref(c, op, defect=None, sd=SD):
    """float64: {"noised" (rows, A), "y" (rows, D), "sig_rows" (B S K M), "ctx_sig" (B S), "S_y" the magnitudes of y's sum}."""
    idx, x, n, sg = _prep_rows(c, op, defect, np.float64)
    sgb = sg[:, None, None]
    noised = x + sgb * n
    cin = 1.0 / sgb if defect == "g_cin" else 1.0 / np.sqrt(sgb * sgb + np.float64(np.float32(sd)) ** 2)
    W, ba = f64(op["WaT"]), f64(op["ba"])
    y = ba + np.einsum("jta,ad->jtd", noised * cin, W)
    S_y = np.abs(ba) + np.einsum("jta,ad->jtd", (np.abs(x) + np.abs(sgb * n)) * cin, np.abs(W))
    return {"noised": noised.reshape(-1, c["A"]), "y": y.reshape(-1, c["D"]), "sig_rows": sg, "ctx_sig": _ctx_sig(c, idx, sg, defect),
            "S_y": S_y.reshape(-1, c["D"])}


def prep_bound(c, op):
    return g(c["A"] + 6) * prep_ref(c, op)["S_y"]


def fma32(a, b, acc):
    """fmaf on fp32 arrays: the product is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def prep_emulate(c, op, sd=SD):
    """fp32 in the kernel's order: {"noised", "y", "sig_rows", "ctx_sig"} as fp32 arrays."""
    idx, x, n, sg = _prep_rows(c, op, None, np.float32)
    sgb, sd = sg[:, None, None], np.float32(sd)
    xin = x + sgb * n                                    # two roundings
    cin = np.float32(1) / np.sqrt(sgb * sgb + sd * sd)
    xv = xin * cin
    acc = np.broadcast_to(op["ba"], xv.shape[:2] + (c["D"],)).astype(np.float32)
    for a in range(c["A"]):                              # the fma chain over A from the bias
        acc = fma32(xv[:, :, a, None], op["WaT"][a], acc)
    return {"noised": xin.reshape(-1, c["A"]), "y": acc.reshape(-1, c["D"]), "sig_rows": sg,
            "ctx_sig": _ctx_sig(c, idx, sg, None).astype(np.float32)}


def prep_shows(c):
    """The planted defects a prep case can show, from its features alone."""
    out = {"g_cin"}
    if c["S"] > 1 and c["K"] > 1:
        out.add("c_swap_ks")
    if c["S"] > 1:
        out.add("d_noise_m")
        if c["ctx"]:
            out.add("h_ctx_k")
    return out


def prep_check(c, op, got, what=""):
    """Hold ``got`` = {"noised", "y", "sig_rows", "ctx_sig" (or None)} to the float64 restatement: (None or a text, largest y error /
    bound).  noised, the rows' and the contexts' sigma are the host's fp32 bits."""
    ref, host = prep_ref(c, op), prep_emulate(c, op)
    b = g(c["A"] + 6) * ref["S_y"]
    texts = []
    for k in ("noised", "sig_rows") + (("ctx_sig",) if c["ctx"] else ()):
        if not same_bits32(np.asarray(got[k]).reshape(host[k].shape), host[k]):
            bad = int(np.flatnonzero(np.asarray(got[k], dtype=np.float32).reshape(-1).view(np.int32) != host[k].reshape(-1).view(np.int32))[0])
            texts.append(f"{what}: {k} element {bad} is {np.asarray(got[k]).reshape(-1)[bad]!r}, the host's {host[k].reshape(-1)[bad]!r}")
    bad = outside(got["y"], ref["y"], b)
    if bad is not None:
        texts.append(f"{what}: y element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}")
    return (texts[0] if texts else None), ratio(got["y"], ref["y"], b)


# ---- k_score_repeat -------------------------------------------------------------------------------------------------------------
WIDTHS = ((5, 3, 7), (5, 0, 7), (1152, 384, 512))
REPEAT_CASES = {**{f"w{w[0]}_{w[1]}_{w[2]}_s{S}_b{B}": dict(B=B, S=S, w=w) for w in WIDTHS for S in (1, 3, 64) for B in (1, 3)},
                "past_grid_cap": dict(B=10, S=64, w=(1152, 0, 512))}     # 640 x 1664 > 4096 x 256


def repeat_operands(c, key="repeat"):
    r = rng_of(key, c["B"], c["S"], c["w"])
    w1, w2, wg = c["w"]
    return {"tok": draw(r, c["B"], w1), "tok2": draw(r, c["B"], w2) if w2 else None, "goal": draw(r, c["B"], wg)}


def repeat_ref(c, op):
    """Row i of (B S) is row i / S of the input, for each operand given."""
    return {k + "_o": None if v is None else np.repeat(v, c["S"], axis=0) for k, v in op.items()}


# ---- k_score_reduce -------------------------------------------------------------------------------------------------------------
def reduce_case(B, K, S, M, E, weights="trapezoid", extreme=False):
    return dict(B=B, K=K, S=S, M=M, E=E, weights=weights, extreme=extreme)


ES = (1, 63, 64, 65, 70, 448, 4096)
SMS = ((1, 1), (1, 2), (3, 1), (2, 2), (5, 1), (16, 2), (64, 1), (1, 64))
BKS = ((1, 1), (3, 1), (1, 3), (2, 5))
REDUCE_CASES = {
    **{f"e{E}": reduce_case(2, 5, 2, 2, E) for E in ES},
    **{f"s{S}_m{M}": reduce_case(1, 3, S, M, 70) for S, M in SMS},
    "s64_m64_e3": reduce_case(1, 3, 64, 64, 3),
    **{f"b{B}_k{K}": reduce_case(B, K, 5, 1, 65) for B, K in BKS},
    **{f"w_{kind}": reduce_case(2, 5, 16, 2, 70, weights=kind) for kind in ("some_zero", "all_zero", "one_1e6")},
    "extreme_levels": reduce_case(1, 3, 2, 2, 70, extreme=True),
}


def reduce_operands(c, key="reduce"):
    r = rng_of(key, sorted(c.items()))
    lv = levels_of(c["S"], c["extreme"])
    return {"F": draw(r, c["B"] * c["S"] * c["K"] * c["M"], c["E"]), "x0": draw(r, c["B"] * c["K"], c["E"]),
            "noise": draw(r, c["S"] * c["M"], c["E"]), "levels": lv, "weights": weights_of(c["weights"], lv)}


def _grids(c, op, defect, dtype):
    """F, x0 and noise as (B, S, K, M, E) broadcastable arrays in ``dtype``."""
    B, K, S, M, E = (c[k] for k in "BKSME")
    F = op["F"].astype(dtype)
    F = F.reshape(B, K, S, M, E).transpose(0, 2, 1, 3, 4) if defect == "c_swap_ks" else F.reshape(B, S, K, M, E)
    n = op["noise"].astype(dtype).reshape(1, S, 1, M, E)
    if defect == "d_noise_m":
        n = np.broadcast_to(n[:, :1], n.shape)
    return F, op["x0"].astype(dtype).reshape(B, 1, K, 1, E), n


def reduce_ref(c, op, defect=None, sd=SD):
    """float64: (score (B K), sum of the terms' magnitudes (B K))."""
    B, K, S, M, E = (c[k] for k in "BKSME")
    F, x, n = _grids(c, op, defect, np.float64)
    sg, sd = f64(op["levels"]).reshape(1, S, 1, 1, 1), np.float64(np.float32(sd))
    den2 = sg * sg + sd * sd
    c_x, c_n, c_f = sg / den2, (sg * sg if defect == "a_cn" else sd * sd) / den2, sd / np.sqrt(den2)
    q = c_x * x - c_n * n - c_f * F
    Q = np.abs(c_x * x) + np.abs(c_n * n) + np.abs(c_f * F)
    keep = np.ones((1, S, 1, M, E))
    if defect == "e_tail":
        keep[..., E // 64 * 64:] = 0
    if defect == "f_wave3":
        keep.reshape(S * M, E)[3::4] = 0
    w = f64(op["weights"]).reshape(1, S, 1, 1, 1) / (1 if defect == "b_no_m" else M)
    return -(w * keep * q * q).sum(axis=(1, 3, 4)).reshape(-1), (w * Q * Q).sum(axis=(1, 3, 4)).reshape(-1)


def reduce_depth(c):
    return 24 + -(-c["E"] // 64) + -(-c["S"] * c["M"] // 4)


def reduce_bound(c, op):
    return g(reduce_depth(c)) * reduce_ref(c, op)[1]


def reduce_emulate(c, op, sd=SD):
    """fp32 in the kernel's order: the score (B K) as an fp32 array."""
    B, K, S, M, E = (c[k] for k in "BKSME")
    F, x, n = _grids(c, op, None, np.float32)
    sg, sd = op["levels"].astype(np.float32).reshape(1, S, 1, 1, 1), np.float32(sd)
    den2 = sg * sg + sd * sd
    c_x, c_n, c_f = sg / den2, sd * sd / den2, sd / np.sqrt(den2)
    c_w = op["weights"].astype(np.float32) / np.float32(M)
    q = c_x * x - c_n * n - c_f * F                                  # three products, two subtractions
    pad = -E % 64
    q = np.concatenate([q, np.zeros(q.shape[:-1] + (pad,), dtype=np.float32)], axis=-1).reshape(B, S, K, M, -1, 64)
    lane = np.zeros((B, S, K, M, 64), dtype=np.float32)
    for t in range(q.shape[4]):                                       # the lane's strided sum (a padded q adds +0 to a sum >= 0)
        lane = fma32(q[..., t, :], q[..., t, :], lane)
    lane = lane.transpose(0, 2, 1, 3, 4).reshape(B * K, S * M, 64)    # (chunk, sample i = s M + m, lane)
    part = np.zeros((B * K, 4), dtype=np.float32)
    other = np.arange(64)
    for wave in range(4):
        acc = np.zeros((B * K, 64), dtype=np.float32)
        for i in range(wave, S * M, 4):
            acc = fma32(np.broadcast_to(c_w[i // M], acc.shape), lane[:, i], acc)
        for off in (32, 16, 8, 4, 2, 1):                              # the xor butterfly
            acc = acc + acc[:, other ^ off]
        part[:, wave] = acc[:, 0]
    return -((part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3]))


def reduce_shows(c, op):
    """The planted defects a reduce case can show, from its features alone."""
    S, M, K, E = c["S"], c["M"], c["K"], c["E"]
    w = np.repeat(op["weights"], M)                  # per sample i
    out = set()
    if (w > 0).any():
        out.add("a_cn")
        if M > 1:
            out.add("b_no_m")
        if S > 1 and K > 1:
            out.add("c_swap_ks")
        if E % 64:
            out.add("e_tail")
    if (w[M:] > 0).any():
        out.add("d_noise_m")
    if (w[3::4] > 0).any():
        out.add("f_wave3")
    return out
