"""The InfoNCE op's test cases and the rules its results are held to -- shared by tests/test_cpu_infonce_abi.py (the float32
oracle against the float64 one: the rules leave a correct float32 implementation room) and tests/test_gpu_infonce.py (the HIP
op).  A plain module: no fixtures, nothing collected.

Inputs are the recipe of tests/test_cla.py (img ~ N(0, 1); lang = mix * img + N(0, 1), mix = 0.5), the reference is
oracle.cla_oracle.clip_auxiliary_loss in float64 with torch autograd, the tolerances are those of
test_hip_infonce_large_batches_against_float64 with ONE change: the absolute floor of a gradient is 1e-3 of the largest
reference magnitude of its own ROW, not of the whole tensor.  Rows of one gradient differ by twelve orders of magnitude here (a
zero row's gradient is 1e12 times its neighbours', the row-scale case spans 1e-6 .. 1e6), and a floor taken over the tensor
would pass anything in the small rows.

Shape cases (logit_scale = log(1 / 0.07), every mode): the smallest batches that cross each block edge of
csrc/mdt_infonce.hip -- 4 rows per workgroup (k_row_lse, k_infonce_grad, the row norms), 64 columns and 4 row groups
(k_col_lse), the padding to 16 rows, 256 threads of k_pair_sum, the step from the few-row GEMM to the tiled one near 400 padded
rows -- at widths that leave most of a 64-lane row stride idle (16), or its last pass partial (48, 80).
Input cases (B = 65, D = 48, every mode; row 64 is alone in the last 4-row group, in the second 64-column block and in a
padded 16-row tile): the letters of CASE_NOTES."""
import collections
import functools
import math

import numpy as np
import torch

from mdt_policy_amd import synthetic
from oracle import cla_oracle as O

MODES = ("symmetric", "img_to_text", "text_to_img")
# One seed for every case, chosen among 21 tried by the float32 oracle on the CPU and by nothing else (tests/test_cpu_infonce_abi.py):
# with one to four negatives at D = 16 a batch can come out saturated (p_ii within 1e-3 of 1), and the gradient of such a row is
# the rounding error of p_ii - 1 in any float32 implementation.  With this seed no case is: the float32 oracle stays below 0.03
# of every tolerance.
SEED = 314
LS_DEFAULT = math.log(1 / 0.07)
LS_CEILING = math.log(100.0)          # where the reference clamps its temperature
SHAPE_B = (2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)
SHAPE_D = (16, 48, 80)
SHAPES = tuple((B, SHAPE_D[i % 3]) for i, B in enumerate(SHAPE_B)) + ((1024, 16), (400, 48))
INPUT_B, INPUT_D = 65, 48
# The ceiling-temperature case draws lang independently of img.  At mix = 0.5 its logits are 45 +- 14 on the diagonal against
# 0 +- 14 elsewhere: in the one-sided modes some rows saturate (1 - p_ii down to 1e-16) and their float64 gradient, 1e-10 and
# less, is lost in ANY float32 run (the float32 oracle misses the per-row tolerance there by factors of 600 to 800, at every seed
# and at every mix from 0.1 to 0.3 tried).  Unaligned, the logits still span +-50 and every row keeps a gradient of order one.
CEILING_MIX = 0.0

CASE_NOTES = {
    "a_ceiling": "logit_scale = log 100, mix = 0 (see CEILING_MIX)",
    "b_cold_m3": "logit_scale = -3 (temperature below 1)",
    "b_cold_0": "logit_scale = 0",
    "c_duplicates": "img[7] = img[3], lang[7] = lang[3], img[64] = img[0]: ties in the running max",
    "d_zero_rows": "img[5] = 0, lang[64] = 0: the 1e-12 clamp of the norm",
    "e_row_scales": "img row i times 10^(-6 + 12 i / 64), lang by the same vector reversed",
    "f_upstream": "upstream gradient -2.5 through backward",
    "g_saturated": "mix = 2.0 at logit_scale = log 100: the loss underflows to 0",
}

Case = collections.namedtuple("Case", "id img lang logit_scale mode upstream")
Result = collections.namedtuple("Result", "loss d_img d_lang d_scale")   # float, (B, D) float64, (B, D) float64, float

LOSS_RTOL, LOSS_ATOL = 1e-4, 1e-6
SCALE_RTOL, SCALE_ATOL = 1e-3, 1e-6
GRAD_RTOL, GRAD_ROW_FLOOR = 1e-3, 1e-3
ZERO_ROW_ATOL = 1e-7


def f32(x):
    """The float32 nearest to x as a Python float: reference and kernel are handed the same temperature."""
    return float(np.float32(x))


def _ids():
    out = [f"B{B}_D{D}_{m}" for B, D in SHAPES for m in MODES]
    return out + [f"{k}_{m}" for k in CASE_NOTES for m in MODES]


IDS = tuple(_ids())
# (B, D, mode) of the direct calls of the C entry (tests/test_gpu_infonce.py): ids of the same form, inputs of the same recipe
DIRECT = ((5, 16, "symmetric"), (17, 48, "symmetric"), (65, 80, "symmetric"), (257, 48, "symmetric"), (15, 80, "img_to_text"),
          (63, 16, "text_to_img"))
DIRECT_IDS = tuple(f"B{B}_D{D}_{m}" for B, D, m in DIRECT)


def inputs(B, D, mix=0.5, seed=None):
    """Fresh (img, lang) float32 CPU tensors of the test_cla.py recipe."""
    seed = SEED if seed is None else seed
    base = synthetic.normal("img", (B, D), seed)
    img = torch.from_numpy(base.copy())
    lang = torch.from_numpy((mix * base + synthetic.normal("lang", (B, D), seed + 1)).astype(np.float32))
    return img, lang


@functools.lru_cache(maxsize=None)
def case(cid):
    """The Case of an id of IDS, or of any other B<batch>_D<dim>_<mode> (shared between tests: never written to)."""
    kind, mode = next((cid[:-len(m) - 1], m) for m in MODES if cid.endswith("_" + m))
    ls, upstream = LS_DEFAULT, 1.0
    if kind not in CASE_NOTES:
        B, D = (int(p[1:]) for p in kind.split("_"))
        img, lang = inputs(B, D)
    else:
        img, lang = inputs(INPUT_B, INPUT_D, mix={"g_saturated": 2.0, "a_ceiling": CEILING_MIX}.get(kind, 0.5))
        if kind in ("a_ceiling", "g_saturated"):
            ls = LS_CEILING
        elif kind == "b_cold_m3":
            ls = -3.0
        elif kind == "b_cold_0":
            ls = 0.0
        elif kind == "c_duplicates":
            img[7], lang[7], img[64] = img[3].clone(), lang[3].clone(), img[0].clone()
        elif kind == "d_zero_rows":
            img[5], lang[64] = 0.0, 0.0
        elif kind == "e_row_scales":
            s = torch.from_numpy((10.0 ** (-6.0 + 12.0 * np.arange(INPUT_B) / 64.0)).astype(np.float32))
            img, lang = img * s[:, None], lang * s.flip(0)[:, None]
        elif kind == "f_upstream":
            upstream = -2.5
    return Case(cid, img, lang, f32(ls), mode, upstream)


def cases():
    """(id, img, lang, logit_scale, mode, upstream) of every case."""
    for cid in IDS:
        yield case(cid)


def run(fn, c, device="cpu", dtype=torch.float32):
    """loss = fn(img, lang, logit_scale, mode=...) and its gradients under the case's upstream gradient -> Result on the CPU."""
    img = c.img.to(device=device, dtype=dtype, copy=True).requires_grad_()   # (a copy: the case's tensors are shared)
    lang = c.lang.to(device=device, dtype=dtype, copy=True).requires_grad_()
    ls = torch.tensor(c.logit_scale, device=device, dtype=dtype, requires_grad=True)
    loss = fn(img, lang, ls, mode=c.mode)
    loss.backward(torch.tensor(c.upstream, device=device, dtype=loss.dtype))
    return Result(float(loss.item()), img.grad.detach().double().cpu(), lang.grad.detach().double().cpu(), float(ls.grad.item()))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The float64 oracle's Result for an id (computed once, shared, never written to)."""
    return run(O.clip_auxiliary_loss, case(cid), dtype=torch.float64)


def reference_of(img, lang, logit_scale, mode):
    """The float64 oracle's Result for inputs that are not in the list (upstream gradient 1)."""
    return run(O.clip_auxiliary_loss, Case("", img.detach().cpu(), lang.detach().cpu(), float(logit_scale), mode, 1.0),
               dtype=torch.float64)


WORST = {}   # quantity -> (largest error / tolerance seen by check() in this process, the id it came from)


def _note(quantity, ratio, cid):
    if ratio > WORST.get(quantity, (-1.0, ""))[0]:
        WORST[quantity] = (float(ratio), cid)


def _check_rows(got, want, what, cid, fraction):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, f"{cid} {what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    assert bool(torch.isfinite(got).all()), f"{cid} {what}: not finite"
    row_max = want.abs().amax(dim=1, keepdim=True)
    tol = GRAD_RTOL * want.abs() + GRAD_ROW_FLOOR * row_max
    tol = torch.where(row_max > 0, tol, torch.full_like(tol, ZERO_ROW_ATOL))   # an all-zero reference row (B = 1 only)
    ratio = (got - want).abs() / tol
    _note(what, ratio.max(), cid)
    bad = ratio > fraction
    if bool(bad.any()):
        r, col = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{cid} {what}: {int(bad.sum())}/{bad.numel()} entries outside {fraction} x the per-row tolerance; worst "
                             f"at [{r}, {col}]: got {got[r, col]:.9e}, want {want[r, col]:.9e}, row max {row_max[r, 0]:.3e}, "
                             f"error / tolerance {ratio[r, col]:.3f}")


def check(result, ref, cid, fraction=1.0):
    """Hold a Result to the module's rules against the float64 Result `ref`.  `fraction` scales every bound (the CPU
    self-check asks for a tenth).  A saturated case (id g_saturated_<mode>) is held to its own rules: see _check_saturated."""
    if cid.startswith("g_saturated"):
        return _check_saturated(result, cid, fraction)
    assert math.isfinite(result.loss) and math.isfinite(result.d_scale), f"{cid}: loss {result.loss}, d_logit_scale {result.d_scale}"
    tol = LOSS_RTOL * abs(ref.loss) + LOSS_ATOL
    _note("loss", abs(result.loss - ref.loss) / tol, cid)
    assert abs(result.loss - ref.loss) <= fraction * tol, f"{cid} loss: got {result.loss:.9e}, want {ref.loss:.9e}"
    tol = SCALE_RTOL * abs(ref.d_scale) + SCALE_ATOL
    _note("d_logit_scale", abs(result.d_scale - ref.d_scale) / tol, cid)
    assert abs(result.d_scale - ref.d_scale) <= fraction * tol, f"{cid} d_logit_scale: got {result.d_scale:.9e}, want {ref.d_scale:.9e}"
    _check_rows(result.d_img, ref.d_img, "d_image", cid, fraction)
    _check_rows(result.d_lang, ref.d_lang, "d_lang", cid, fraction)


def _check_saturated(result, cid, fraction):
    """The float64 loss is below 1e-16 and its gradients near 1e-18: a relative comparison would measure float32 rounding of
    nothing.  Instead: everything finite; |loss| within 16 ulp of the largest logit, exp(logit_scale), which is where lse - s is
    formed; every gradient entry at most 1e-3 of the largest float64 magnitude of the same gradient in case (a) of the same
    mode -- the same temperature and shapes, unsaturated."""
    c = case(cid)
    assert math.isfinite(result.loss) and math.isfinite(result.d_scale), f"{cid}: loss {result.loss}, d_logit_scale {result.d_scale}"
    bound = 16 * 2.0 ** -23 * math.exp(c.logit_scale)
    _note("saturated loss", abs(result.loss) / bound, cid)
    assert abs(result.loss) <= fraction * bound, f"{cid} loss: {result.loss:.3e} above {fraction} x {bound:.3e}"
    a = reference("a_ceiling_" + c.mode)
    for what, got, big in (("d_image", result.d_img, float(a.d_img.abs().max())), ("d_lang", result.d_lang, float(a.d_lang.abs().max())),
                           ("d_logit_scale", torch.tensor([[result.d_scale]], dtype=torch.float64), abs(a.d_scale))):
        assert bool(torch.isfinite(got).all()), f"{cid} {what}: not finite"
        worst = float(got.abs().max())
        _note("saturated " + what, worst / (1e-3 * big), cid)
        assert worst <= fraction * 1e-3 * big, f"{cid} {what}: largest entry {worst:.3e} above {fraction} x 1e-3 x {big:.3e}"
