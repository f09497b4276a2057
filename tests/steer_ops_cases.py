"""Shared by tests/test_gpu_steer_ops.py, tests/test_cpu_steer_ops_reference.py and tests/test_native_sampler_plan.py: the four
element-wise kernels of the steered samplers (mdt_policy_amd/csrc/mdt_steer.hip: k_steer_seed, k_steer_step, k_steer_first,
k_steer_plan; hooks mdt_op_steer_* of include/mdt_hip_debug.h) restated in numpy, their cases, and their error bounds.

One restatement, two precisions.  Every function takes ``q``, applied to the result of every operation in the kernel's order:
``exact`` (identity) makes it the float64 reference, ``rounded`` (to fp32 and back) a correctly rounded fp32 execution of the same
order.  ``defect`` plants one mistake in the plan restatement (DEFECTS); tests/test_cpu_steer_ops_reference.py shows that the
rounded execution is inside every bound and every defect a case can show is outside.

Bounds.  u = 2^-24, g(n) = n u / (1 - n u) (n roundings compose to at most g(n), Higham's gamma), magnitudes in float64.
  EDM scalings from fp32 sigma, sd: den2 = sigma^2 + sd^2 has 2 roundings (two squares, then a sum of positives: max + 1);
    c_skip = sd^2 / den2: 1 + 2 + 1 = 4;  c_out = sigma sd / sqrt(den2): 1 + (2 / 2 + 1) + 1 = 4;  c_in = 1 / sqrt(den2): 2 + 1 = 3.
  seed   D  = fma(F, c_out, x c_skip): c_skip 4 + product 1 + fma 1 = 6 on S_D = |F c_out| + |x c_skip|         g(6) S_D
         e  = w (known - D): 6 of D + subtraction 1 + product 1 = 8                                             g(8) |w| (|known| + S_D)
         dF = c_out e: 8 + c_out 4 + product 1 = 13                                                             g(13) c_out |w| (|known| + S_D)
  D'     g = fma(small, c_in, e c_skip): 6 on S_g = |small c_in| + |e c_skip|;  D' = D + scale g: product 1 + sum 1 = 8 on
         S_D' = |D| + |scale| S_g                                                                               g(8) S_D'
  step   x_out = ratio x_in + coef D': 8 of D' + product 1 + sum 1 = 10; the clamp is 1-Lipschitz               g(10) (|ratio x_in| + |coef| S_D')
  first  Y = x_T + n0 cn: product 1 + sum 1                                                                     g(2) (|x_T| + |n0 cn|)
  plan   d = (Y - D') / sigma: 8 of D' + subtraction 1 + division 1 = 10 on S_d = (|Y| + S_D') / sigma          g(10) S_d
         X' = sum_q cx_q R_q from 0: a term sees its product and at most 9 sums = 10 on S_X = sum |cx_q R_q|; the roundings of D'
         enter through cx_D (8 + 10) and cx_d (10 + 10)                       g(10) S_X + g(18) |cx_D| S_D' + g(20) |cx_d| S_d
         Y' = cy_X' X' + sum_q cy_q R_q: a term sees its product and at most 10 sums = 11 on S_Y = |cy_X' X'| + sum |cy_q R_q|
                              g(11) S_Y + (1 + g(11)) |cy_X'| bound(X') + g(19) |cy_D| S_D' + g(21) |cy_d| S_d
         record: Y's bits, D' to g(8) S_D';  history: H0..H2 move as bits, the new H0 is D' or d to its bound
  the rows' sigma, X of `first`, the zeroed history, untouched rows: bits.
A contracted multiply-add has one rounding fewer: the counts hold with or without it.

Layout.  Every buffer is a tests/guarded.Guarded of dense rows of ``cols_of(N, A)`` columns: A where it divides N, else N's
smallest divisor above 1 (N = 262141 = 11 x 23831, 262438 = 2 x 131219) -- the guard bands stay at 1024 floats."""
import zlib

import numpy as np

from mdt_policy_amd import _lib

U = 2.0 ** -24
NREG = _lib.SAMPLER_NREG
R_X, R_Y, R_D, R_DD, R_H0, R_N0, R_N1 = 0, 1, 2, 3, 4, 8, 9
PUSH_NONE, PUSH_D, PUSH_DD = 0, 1, 2
CAP = 1024 * 256                  # STEER_MAX_BLOCKS * STEER_THREADS: the indices of one trip of the grid-stride loop
SD, BETA = 0.5, 5.0
DEFECTS = ("rec_D", "hist_order", "scale_next", "y_unclamped", "noise_row0")

# (N, R, A)
SIZES = {
    "one_block": (70, 1, 7),              # one partly filled block
    "ragged": (1050, 15, 7),              # ragged last block
    "capacity": (CAP - 3, 3, 7),          # N + R exactly the grid's capacity
    "sigma_past_cap": (CAP - 2, 3, 2),    # the one index of the second trip is a sigma row
    "second_trip": (CAP + 294, 5, 7),     # second-trip elements and sigma rows
    "chunk64": (4096, 1, 64),             # one 64 x 64 chunk
}
SIGMA_ONLY = (0, 5, 1)                    # k_steer_step as fill_sigma calls it


def g(n):
    return n * U / (1.0 - n * U)


def exact(v):
    return v


def rounded(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def cols_of(N, A):
    if N % A == 0:
        return A
    return next((d for d in range(2, 1025) if N % d == 0), N)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def draw(rng, *shape):
    """fp32 magnitudes in [0.5, 1.5], random signs: every term of every sum is far above its bound."""
    return ((0.5 + rng.random(shape)) * (rng.integers(0, 2, shape) * 2 - 1)).astype(np.float32)


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def host_scale(beta, sigma, sd):
    """s(sigma) = min(beta, 1 + sigma^2 / sd^2) in fp32, as the entry points form it on the host."""
    s, d = np.float32(sigma), np.float32(sd)
    return np.float32(min(np.float32(beta), np.float32(1) + (s * s) / (d * d)))


def edm(sigma, sd, q):
    sg, sd = np.float64(np.float32(sigma)), np.float64(np.float32(sd))
    den2 = q(q(sg * sg) + q(sd * sd))
    root = q(np.sqrt(den2))
    return q(q(sd * sd) / den2), q(q(sg * sd) / root), q(1.0 / root)   # c_skip, c_out, c_in


# ---- k_steer_seed ---------------------------------------------------------------------------------------------------------------
def seed_operands(N, key="seed"):
    r = rng_of(key, N)
    return {k: draw(r, N) for k in ("F", "x", "known", "weight")}


def seed_ref(op, sigma, sd, q=exact):
    c_skip, c_out, _ = edm(sigma, sd, q)
    F, x, known, w = (f64(op[k]) for k in ("F", "x", "known", "weight"))
    D = q(F * c_out + q(x * c_skip))
    e = q(w * q(known - D))
    return {"D": D, "e": e, "dF": q(c_out * e)}


def seed_bounds(op, sigma, sd):
    c_skip, c_out, _ = edm(sigma, sd, exact)
    F, x, known, w = (f64(op[k]) for k in ("F", "x", "known", "weight"))
    S_D = np.abs(F * c_out) + np.abs(x * c_skip)
    S_e = np.abs(w) * (np.abs(known) + S_D)
    return {"D": g(6) * S_D, "e": g(8) * S_e, "dF": g(13) * c_out * S_e}


# ---- D' = D + scale (c_in small + c_skip e), shared by k_steer_step and k_steer_plan ---------------------------------------------
def dprime(op, sigma, sd, scale, q=exact):
    """(D', S_D')."""
    c_skip, _, c_in = edm(sigma, sd, q)
    small, e, D = (f64(op[k]) for k in ("small", "e", "D"))
    gg = q(small * c_in + q(e * c_skip))
    with np.errstate(invalid="ignore"):
        dp = q(D + q(np.float64(scale) * gg))
        S = np.abs(D) + abs(np.float64(scale)) * (np.abs(small * c_in) + np.abs(e * c_skip))
    return dp, S


def clamp(v, lo, hi, A):
    """torch.clamp per column i % A: ordered compares keep a NaN, lo > hi gives hi."""
    col = np.arange(v.shape[0]) % A
    l, h = f64(lo)[col], f64(hi)[col]
    with np.errstate(invalid="ignore"):
        v = np.where(v < l, l, v)
        return np.where(v > h, h, v)


def bounds_of(rng, A, inverted=False):
    """(lo, hi) inside the spread of the values they clamp; ``inverted``: column 1 % A has lo > hi."""
    lo, hi = (-0.4 - 0.2 * rng.random(A)).astype(np.float32), (0.4 + 0.2 * rng.random(A)).astype(np.float32)
    if inverted:
        c = 1 % A
        lo[c], hi[c] = hi[c], lo[c]
    return lo, hi


# ---- k_steer_step ---------------------------------------------------------------------------------------------------------------
STEP = dict(sigma=2.0, scale=float(host_scale(BETA, 2.0, SD)), ratio=0.25, coef=0.75, sigma_next=0.5)


def step_operands(N, A, bounded, key="step"):
    r = rng_of(key, N, A, bounded)
    op = {k: draw(r, N) for k in ("small", "e", "D", "x_in")}
    op["lo"], op["hi"] = bounds_of(r, A, inverted=True) if bounded else (None, None)
    return op


def step_ref(op, A, q=exact, sd=SD, **kw):
    p = dict(STEP, **kw)
    dp, _ = dprime(op, p["sigma"], sd, p["scale"], q)
    v = q(q(np.float64(np.float32(p["ratio"])) * f64(op["x_in"])) + q(np.float64(np.float32(p["coef"])) * dp))
    return clamp(v, op["lo"], op["hi"], A) if op["lo"] is not None else v


def step_bound(op, sd=SD, **kw):
    p = dict(STEP, **kw)
    _, S = dprime(op, p["sigma"], sd, p["scale"], exact)
    return g(10) * (np.abs(np.float64(np.float32(p["ratio"])) * f64(op["x_in"])) + abs(np.float64(np.float32(p["coef"]))) * S)


# ---- k_steer_first --------------------------------------------------------------------------------------------------------------
def first_operands(N, key="first"):
    r = rng_of(key, N)
    return {"x_T": draw(r, N), "n0": draw(r, N)}


def first_ref(op, cn, with_row, q=exact):
    """Y; with a null row or cn == 0 the kernel copies x_T (bits)."""
    x = f64(op["x_T"])
    if not with_row or np.float32(cn) == 0:
        return x
    return q(x + q(f64(op["n0"]) * np.float64(np.float32(cn))))


def first_bound(op, cn, with_row):
    if not with_row or np.float32(cn) == 0:
        return np.zeros(op["x_T"].shape[0])
    return g(2) * (np.abs(f64(op["x_T"])) + np.abs(f64(op["n0"]) * np.float64(np.float32(cn))))


# ---- k_steer_plan ---------------------------------------------------------------------------------------------------------------
def plan_registers(X, Y, Dv, sigma, H, noise, n_noise, slots, defect=None, q=exact):
    """The ten registers of one evaluation: X, Y, D, d = (Y - D) / sigma, H0..H3, N0, N1.  A noise slot outside [0, n_noise), or
    any slot of a null ``noise``, reads as 0."""
    zero = np.zeros_like(X)

    def row(idx):
        if noise is None:
            return zero
        if 0 <= idx < n_noise:
            return noise[idx]
        return noise[0] if defect == "noise_row0" and idx >= n_noise else zero
    with np.errstate(invalid="ignore"):
        d = q(q(Y - Dv) / np.float64(sigma))
    return [X, Y, Dv, d, H[0], H[1], H[2], H[3], row(slots[0]), row(slots[1])]


def plan_update(cx, cy, R, clip=None, q=exact, defect=None):
    """(X', Y'): X' = sum_q cx_q R_q from 0, clamped by ``clip`` (a function, or None), Y' = cy[NREG] X' + sum_q cy_q R_q -- the
    order of head_plan_elem (mdt_tiles.h)."""
    with np.errstate(invalid="ignore"):
        xn = q(np.float64(cx[0]) * R[0])
        for k in range(1, NREG):
            xn = q(xn + q(np.float64(cx[k]) * R[k]))
        raw = xn
        if clip is not None:
            xn = clip(xn)
        yn = q(np.float64(cy[NREG]) * (raw if defect == "y_unclamped" else xn))
        for k in range(NREG):
            yn = q(yn + q(np.float64(cy[k]) * R[k]))
    return xn, yn


def push_history(H, push, R, defect=None):
    """The history slots after the evaluation."""
    if push == PUSH_NONE:
        return H
    new = R[R_D] if push == PUSH_D else R[R_DD]
    if defect == "hist_order":   # slot 1 written before slot 2 reads it, and so on: H0 everywhere
        return np.stack([new, H[0], H[0], H[0]])
    return np.stack([new, H[0], H[1], H[2]])


def apply_plan(plan, x_T, noise, denoiser):
    """A whole plan in float64 with ``denoiser(Y, sigma, k)`` as D at evaluation k: the per-element update every plan kernel
    runs (MDT_HEAD_PLAN in mdt_tiles.h, k_steer_plan).  Returns (X, [(Y, D) of every evaluation])."""
    X = x_T.copy()
    Y = X + (plan.y0_cn * noise[plan.y0_noise] if plan.y0_noise >= 0 else 0.0)
    H = np.zeros((4,) + X.shape)
    seen = []
    for k in range(plan.n_evals):
        e = plan.e[k]
        D = denoiser(Y, np.float64(e.sigma), k)
        seen.append((Y, D))
        R = plan_registers(X, Y, D, e.sigma, H, noise, noise.shape[0], list(e.noise))
        Xn, Yn = plan_update(list(e.cx), list(e.cy), R)
        H = push_history(H, e.push, R)
        X, Y = Xn, Yn
    return X, seen


def copy_eval(ev, **over):
    out = _lib.SamplerEval.from_buffer_copy(ev)
    for k, v in over.items():
        if k == "noise":
            out.noise[0], out.noise[1] = v
        else:
            setattr(out, k, v)
    return out


def _schedule(n):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    return gs.get_sigmas_exponential(n, 1.0, 80.0).tolist()


def plan_rows():
    """name -> an evaluation row of a real plan (exponential schedule 80 -> 1), and one synthetic row."""
    sde = _lib.sampler_plan("dpmpp_sde", _schedule(4), eta=1.0)
    anc = _lib.sampler_plan("dpm_2_ancestral", _schedule(4))
    rows = {
        "heun_second": _lib.sampler_plan("heun", _schedule(4)).e[1],
        "dpmpp_2m_third": _lib.sampler_plan("dpmpp_2m", _schedule(4)).e[2],
        "lms4_fifth": _lib.sampler_plan("lms", _schedule(6), order=4).e[4],
        "dpmpp_sde_eta1": next(sde.e[k] for k in range(sde.n_evals) if max(sde.e[k].noise) >= 0),
        "dpm_2_ancestral": next(anc.e[k] for k in range(anc.n_evals) if max(anc.e[k].noise) >= 0),
    }
    syn = _lib.SamplerEval()
    syn.sigma, syn.sigma_next = 2.0, 0.5
    for k in range(NREG):
        syn.cx[k] = (-1) ** k * (0.3 + 0.07 * k)
        syn.cy[k] = (-1) ** (k + 1) * (0.9 - 0.06 * k)
    syn.cy[NREG] = 0.8
    syn.push, syn.ends_step, syn.begins_step = PUSH_D, 1, 1
    syn.noise[0], syn.noise[1] = 0, 1
    rows["synthetic"] = syn
    return {k: copy_eval(v) for k, v in rows.items()}


def feature(row, size="one_block", **kw):
    """A plan-kernel case.  ``inplace``: x_out == X and y_out == Y, else x_out distinct and y_out null (the last evaluation);
    ``sigma`` / ``sigma_next`` / ``push`` / ``slots`` / ``ends_step`` / ``begins_step``: put over the row's (None: the row's);
    ``n_noise`` rows of noise, ``noise_null``: the pointer is null all the same; ``bounds``: None, "plain" or "inverted";
    ``rec``: a record is given; ``nan``: D[3] is NaN."""
    c = dict(row=row, size=size, inplace=True, sigma=None, sigma_next=None, push=None, slots=None, n_noise=3, noise_null=False,
             bounds=None, ends_step=None, begins_step=None, rec=False, nan=False)
    assert set(kw) <= set(c)
    c.update(kw)
    return c


def case_id(c):
    d = feature(c["row"])
    return "-".join([c["row"], c["size"]] + [f"{k}={v}" for k, v in c.items() if k not in ("row", "size") and v != d[k]])


# A small cross product: every feature of the issue at least once, every row, every size.
PLAN_CASES = [
    feature("heun_second", bounds="plain", ends_step=1, rec=True, begins_step=0),               # clamp, Y' from the clamped X'
    feature("heun_second", "ragged", inplace=False, bounds="inverted", ends_step=1, sigma=0.5, sigma_next=0.1),
    feature("heun_second", bounds="plain", ends_step=0),                                           # bounds given, no clamp
    feature("dpmpp_2m_third", "ragged", push=PUSH_D, rec=True, begins_step=1),
    feature("dpmpp_2m_third", sigma=0.001, sigma_next=0.0, push=PUSH_DD, inplace=False),
    feature("lms4_fifth", push=PUSH_D, sigma=80.0, sigma_next=0.5, rec=True, begins_step=1),
    feature("lms4_fifth", "chunk64", push=PUSH_NONE, nan=True, bounds="plain", ends_step=1, rec=True, begins_step=1),
    feature("dpmpp_sde_eta1", slots=(2, -1)),
    feature("dpmpp_sde_eta1", "ragged", slots=(3, 0), n_noise=3),                                  # an index >= n_noise reads as 0
    feature("dpm_2_ancestral", slots=(1, 2), noise_null=True),                                     # null noise, n_noise > 0
    feature("dpm_2_ancestral", "chunk64", slots=(0, 5), n_noise=2, sigma=0.5, sigma_next=2.0, inplace=False),
    feature("synthetic", "ragged", bounds="inverted", rec=True, nan=True),
    feature("synthetic", "chunk64", sigma=0.001, sigma_next=0.5, push=PUSH_DD, slots=(-1, 1)),
    feature("synthetic", "capacity", rec=True),
    feature("synthetic", "sigma_past_cap", bounds="plain", rec=True, push=PUSH_DD, slots=(2, 7)),
    feature("synthetic", "second_trip", inplace=False, rec=True, sigma=0.5, sigma_next=0.001),
    feature("heun_second", "second_trip", push=PUSH_D),
]


def plan_case(c, rows=None):
    """(ev, operands, N, R, A) of a case: fp32 numpy operands; hist holds four distinct non-zero rows."""
    N, R, A = SIZES[c["size"]]
    row = (rows or plan_rows())[c["row"]]
    over = {k: c[k] for k in ("sigma", "sigma_next", "push", "ends_step", "begins_step") if c[k] is not None}
    if c["slots"] is not None:
        over["noise"] = c["slots"]
    ev = copy_eval(row, **over)
    r = rng_of("plan", case_id(c))
    op = {k: draw(r, N) for k in ("small", "e", "D", "Y", "X")}
    op["hist"] = np.stack([draw(r, N) * np.float32(1 + h) for h in range(4)])
    op["noise_rows"] = np.stack([draw(r, N) for _ in range(c["n_noise"])]) if c["n_noise"] else None
    op["noise"] = None if c["noise_null"] else op["noise_rows"]
    op["n_noise"] = c["n_noise"]
    op["lo"], op["hi"] = None, None
    op["rec"] = c["rec"]
    if c["bounds"]:   # the 0.3 / 0.7 quantiles of the unclamped float64 X', per column: the clamp acts on part of every column
        free = plan_ref(ev, op, A)["x"].reshape(-1, A)
        op["lo"], op["hi"] = (np.quantile(free, p, axis=0).astype(np.float32) for p in (0.3, 0.7))
        if c["bounds"] == "inverted":
            k = 1 % A
            op["lo"][k], op["hi"][k] = op["hi"][k], op["lo"][k]
    if c["nan"]:
        op["D"][3] = np.float32("nan")
    return ev, op, N, R, A


def plan_ref(ev, op, A, q=exact, defect=None, sd=SD, beta=BETA):
    """One evaluation: {"x", "y", "hist", "rec" (None: rows untouched), "sig", "scale", and the exact-mode magnitudes}."""
    scale = host_scale(beta, ev.sigma_next if defect == "scale_next" else ev.sigma, sd)
    dp, S_dp = dprime(op, ev.sigma, sd, scale, q)
    X, Y, H = f64(op["X"]), f64(op["Y"]), f64(op["hist"])
    R = plan_registers(X, Y, dp, np.float32(ev.sigma), H, f64(op["noise"]), op["n_noise"], list(ev.noise), defect, q)
    clip = (lambda v: clamp(v, op["lo"], op["hi"], A)) if op["lo"] is not None and ev.ends_step else None
    cx, cy = [np.float32(v) for v in ev.cx], [np.float32(v) for v in ev.cy]
    xn, yn = plan_update(cx, cy, R, clip, q, defect)
    rec = None
    if op["rec"] and ev.begins_step:
        rec = np.stack([Y, f64(op["D"]) if defect == "rec_D" else dp])
    return {"x": xn, "y": yn, "hist": push_history(H, ev.push, R, defect), "rec": rec, "sig": np.float32(ev.sigma_next),
            "scale": scale, "dp": dp, "S_dp": S_dp, "R": R}


def plan_bounds(ev, op, A):
    """Per element: {"x", "y", "dp" (the record's D' and a pushed D'), "d" (a pushed d)} from the float64 run."""
    ref = plan_ref(ev, op, A)
    R, S_dp = ref["R"], ref["S_dp"]
    cx, cy = [abs(np.float64(v)) for v in ev.cx], [abs(np.float64(v)) for v in ev.cy]
    with np.errstate(invalid="ignore"):
        S_d = (np.abs(R[R_Y]) + S_dp) / np.float64(np.float32(ev.sigma))
        S_X = sum(cx[k] * np.abs(R[k]) for k in range(NREG))
        bx = g(10) * S_X + g(18) * cx[R_D] * S_dp + g(20) * cx[R_DD] * S_d
        S_Y = cy[NREG] * np.abs(ref["x"]) + sum(cy[k] * np.abs(R[k]) for k in range(NREG))
        by = g(11) * S_Y + (1 + g(11)) * cy[NREG] * bx + g(19) * cy[R_D] * S_dp + g(21) * cy[R_DD] * S_d
    return {"x": bx, "y": by, "dp": g(8) * S_dp, "d": g(10) * S_d}


def shows(c, ev, op, sd=SD, beta=BETA):
    """The planted defects this case can show, from its features alone."""
    out = set()
    if op["rec"] and ev.begins_step:
        out.add("rec_D")
    if ev.push != PUSH_NONE:
        out.add("hist_order")
    if host_scale(beta, ev.sigma, sd) != host_scale(beta, ev.sigma_next, sd):
        out.add("scale_next")
    if op["lo"] is not None and ev.ends_step and ev.cy[NREG] != 0 and c["inplace"]:
        out.add("y_unclamped")
    if op["noise"] is not None and any(ev.noise[j] >= op["n_noise"] and (ev.cx[R_N0 + j] != 0 or (ev.cy[R_N0 + j] != 0 and c["inplace"]))
                                       for j in range(2)):
        out.add("noise_row0")
    return out


def outside(got, want, bound):
    """None, or (index, got, want, bound) of the element furthest outside its bound.  A NaN of the reference asks for a NaN (any
    payload); a NaN anywhere else is outside."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    with np.errstate(invalid="ignore"):
        excess = np.abs(got - want) - bound
    excess = np.where(np.isnan(want), np.where(np.isnan(got), -1.0, np.inf), np.where(np.isnan(got), np.inf, excess))
    if not (excess > 0).any():
        return None
    i = np.unravel_index(int(excess.argmax()), want.shape)
    return tuple(int(v) for v in i), float(got[i]), float(want[i]), float(bound[i])


def ratio(got, want, bound):
    """Largest |got - want| / bound over the finite elements with a positive bound."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    ok = np.isfinite(want) & (bound > 0)
    return float((np.abs(got - want)[ok] / bound[ok]).max()) if ok.any() else 0.0


def plan_check(ev, op, A, got, what="", y_given=True):
    """Hold a plan evaluation's outputs ``got`` = {"x", "y" (or None), "hist", "rec" (or None), "sig"} to the float64 reference:
    None, or a text naming the first output outside.  Returns (text, largest error / bound)."""
    ref, b = plan_ref(ev, op, A), plan_bounds(ev, op, A)
    worst = 0.0

    def hold(name, g_, w_, bd):
        nonlocal worst
        bad = outside(g_, w_, bd)
        worst = max(worst, ratio(g_, w_, bd))
        return None if bad is None else f"{what}: {name} element {bad[0]} is {bad[1]!r}, float64 {bad[2]!r}, bound {bad[3]:.3e}"
    texts = [hold("x_out", got["x"], ref["x"], b["x"])]
    if y_given:
        texts.append(hold("y_out", got["y"], ref["y"], b["y"]))
    if ev.push == PUSH_NONE:
        texts.append(None if same_bits32(got["hist"], op["hist"]) else f"{what}: the history changed without a push")
    else:
        texts.append(hold("hist[0]", got["hist"][0], ref["hist"][0], b["dp"] if ev.push == PUSH_D else b["d"]))
        for h in (1, 2, 3):
            texts.append(None if same_bits32(got["hist"][h], op["hist"][h - 1]) else f"{what}: hist[{h}] is not the old hist[{h - 1}]'s bits")
    if ref["rec"] is not None:
        texts.append(None if same_bits32(got["rec"][0], op["Y"]) else f"{what}: the record's x is not Y's bits")
        texts.append(hold("the record's denoised", got["rec"][1], ref["rec"][1], b["dp"]))
    return next((t for t in texts if t), None), worst


def same_bits32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def as_f32(ref_out):
    """A rounded-mode output as the fp32 array a kernel would have stored."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(ref_out, dtype=np.float64).astype(np.float32)
