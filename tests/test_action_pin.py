"""Pinned actions (chunk inpainting), CPU tier: ActionPin's shapes, broadcasting and refusals, ActionPin.overlap against a
hand-written table, and the package's host loops -- DDIM and every kind of test_gpu_sampler_bounds.KINDS -- over a float64
oracle denoiser that takes ``pin=`` and applies D' = keep * known + (1 - keep) * D the way GCDenoiser.forward does.

The inputs, shared with tests/test_gpu_action_pin.py: the g7_samplers model, 4 steps of 80 -> 1 -> 0 (dpm_fast: 7 evaluations
from 80 to 1); ``known`` is the unpinned host-loop result of another noise seed, negated; ``keep`` is 1 on tokens 0..2, 0.5 on
token 3 and 0 elsewhere.  The conditions that keep the comparisons from being vacuous (``conditions``) are asserted on the
host loop alone: the pinned and the unpinned result differ by more than 100 x the tolerance on the pinned elements and by more
than 10 x the tolerance on the keep == 0 elements, the tolerance of a set of elements being atol + rtol max |pinned| over that
set (the largest tolerance any of its elements is compared with).  Measured with this float64 loop at B = 2 (B = 1): on the
keep == 0 elements the gaps are 0.043 .. 0.11 (0.022 .. 0.040) against 10 x tol = 0.014 .. 0.017 (0.010 .. 0.013), except
dpm_fast -- it stops at sigma = 1, where the chunk is still mostly noise: 0.010 against 0.024.  For that kind ``known`` is
scaled by 64 (KNOWN_SCALE: 0.077 against 0.024, at B = 1 0.043 against 0.030; the effect saturates, 16 gives 0.055 and 0.035),
the condition stays.  On the pinned elements every kind is above 2.1 against 100 x tol <= 0.2 (dpm_fast, scaled: 168 against
17).

dpm_fast stops at sigma_min: on an element with keep == 1 the denoiser is the constant ``known``, eps = (x - known) / sigma, and
DPM-Solver is exact for it at every order (its corrections are differences of equal eps values), so
x_end - known = (x_T - known) sigma_min / sigma_max -- the bound asserted for it."""
import pytest
import torch

from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from oracle import mdt_oracle as O
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, inputs_of, load_fixture, params_of

N, SMIN, SMAX, NFE = 4, 1.0, 80.0, 7  # test_gpu_sampler_bounds' schedule
KINDS = {"euler": dict(s_churn=1.0), "euler_ancestral": {}, "heun": dict(s_churn=1.0), "dpm_2": dict(s_churn=1.0),
         "dpm_2_ancestral": {}, "lms": {}, "dpmpp_2s": {}, "dpmpp_2s_ancestral": {}, "dpmpp_2m": {}, "dpmpp_sde": {},
         "dpm_fast": {}}  # test_gpu_sampler_bounds.KINDS (that module is GPU-only: restated, and compared in the GPU tier)
NAMES = ["ddim"] + sorted(KINDS)
HARD, HALF = 3, 3  # keep == 1 on tokens [0, HARD), 0.5 on token HALF
KNOWN_SCALE = {"dpm_fast": 64.0}  # see the module docstring


def sched():
    return gs.get_sigmas_exponential(N, SMIN, SMAX)


def keep_of(Ta):
    keep = torch.zeros(Ta)
    keep[:HARD], keep[HALF] = 1.0, 0.5
    return keep


def run(name, model, state, x, goal, seed=11, **kw):
    """One seeded sampler call through gc_sampling (test_gpu_sampler_bounds.run, DDIM added)."""
    torch.manual_seed(seed)
    kw = dict(KINDS.get(name, {}), **kw)
    if name == "dpmpp_sde" and "noise_sampler" not in kw:
        rows = iter(torch.randn(2 * N, *x.shape, device=x.device, dtype=x.dtype))
        kw["noise_sampler"] = lambda s0, s1: next(rows)
    with torch.no_grad():
        if name == "dpm_fast":
            return gs.sample_dpm_fast(model, state, x, goal, SMIN, SMAX, NFE, **kw)
        return getattr(gs, "sample_" + name)(model, state, x, goal, sched(), **kw)


def conditions(name, free, pinned, known, keep, x_T, atol=ATOL, rtol=RTOL):
    """What makes a comparison against ``pinned`` mean something, asserted on host-loop results alone; ``keep`` is (Ta,)."""
    free, pinned, known, x_T = (t.detach().double().cpu() for t in (free, pinned, known, x_T))
    hard, rest = keep == 1, keep == 0
    tol_pin, tol_rest = (atol + rtol * float(pinned[:, sel].abs().max()) for sel in (hard, rest))
    gap_pin = float((pinned - free)[:, hard].abs().max())
    gap_rest = float((pinned - free)[:, rest].abs().max())
    print(f"{name}: |pinned - unpinned| max {gap_pin:.4f} on keep == 1 (100 tol {100 * tol_pin:.4f}), {gap_rest:.4f} on keep == 0 "
          f"(10 tol {10 * tol_rest:.4f})")
    assert gap_pin > 100 * tol_pin, f"{name}: pinned and unpinned differ by {gap_pin:.3e} only on the pinned elements"
    assert gap_rest > 10 * tol_rest, f"{name}: pinned and unpinned differ by {gap_rest:.3e} only on the keep == 0 elements"
    # where the pinned elements arrive
    if name.startswith("dpm_fast"):
        bound = (SMIN / SMAX) * (x_T - known)[:, hard].abs() + atol + rtol * known[:, hard].abs()
        assert bool(((pinned - known)[:, hard].abs() <= bound).all()), "dpm_fast: a pinned element is outside its sigma_min bound"
    else:
        assert_close(pinned[:, hard], known[:, hard], rtol=rtol, atol=atol, what=f"{name}: pinned elements")


class OracleModel:
    """model(state, x, goal, sigma, pin=None) over the float64 oracle (tests/test_log_likelihood.py's, with the pin)."""

    def __init__(self, meta):
        self.P = O.to_dtype(params_of(meta), torch.float64)
        self.cfg, self.arch = cfg_of(meta), meta["arch"]

    def __call__(self, state, x, goal, sigma, pin=None):
        st = {k: (v.double() if torch.is_tensor(v) else v) for k, v in state.items()}
        sigma = sigma.double().reshape(-1)
        den = O.denoise(self.P, self.cfg, st, x.double(), goal.double(), sigma.expand(x.shape[0]), 0.5, self.arch)
        if pin is None:
            return den
        known, keep = (t.double() for t in pin.on(den.device, den.shape))
        return torch.where(keep == 0, den, torch.where(keep == 1, known, den + keep * (known - den)))


_ORACLE = {}


def oracle_case(B=2):
    """(model, state, goal, x_T, x_T of the other seed) of the float64 oracle loops, built once."""
    if B not in _ORACLE:
        meta, _ = load_fixture("g7_samplers.npz")
        state, goal, noise = inputs_of(dict(meta, B=B, input_seed=700 + B), dtype=torch.float64)
        _, _, other = inputs_of(dict(meta, B=B, input_seed=900 + B), dtype=torch.float64)
        _ORACLE[B] = (OracleModel(meta), state, goal, noise * SMAX, other * SMAX)
    return _ORACLE[B]


_LOOPS = {}


def oracle_loops(name, B=2):
    """(unpinned, known, pin, pinned) of the float64 oracle host loop of a kind, computed once and left unchanged."""
    if (name, B) not in _LOOPS:
        model, state, goal, x, x_other = oracle_case(B)
        free = run(name, model, state, x, goal)
        known = -KNOWN_SCALE.get(name, 1.0) * run(name, model, state, x_other, goal)
        pin = ActionPin(known, keep_of(x.shape[1]))
        pinned = run(name, model, state, x, goal, extra_args={"pin": pin})
        _LOOPS[(name, B)] = (free, known, pin, pinned)
    return _LOOPS[(name, B)]


# ---- ActionPin ---------------------------------------------------------------------------------------------------------------
def test_keep_shapes_broadcast_to_the_chunk():
    B, Ta, A = 2, 10, 7
    known = torch.arange(B * Ta * A, dtype=torch.float32).reshape(B, Ta, A)
    row = torch.linspace(0, 1, Ta)
    for keep in (row, row.expand(B, Ta), row.reshape(1, Ta, 1).expand(B, Ta, 1), row.reshape(1, Ta, 1).expand(B, Ta, A)):
        k, q = ActionPin(known, keep).on("cpu", (B, Ta, A))
        assert k.shape == q.shape == (B, Ta, A) and k.is_contiguous() and q.is_contiguous()
        assert k.dtype == q.dtype == torch.float32
        assert torch.equal(k, known) and torch.equal(q, row.reshape(1, Ta, 1).expand(B, Ta, A))
    # known broadcasts: one pose for every token, one chunk for every sample, float64 and lists
    k, _ = ActionPin(torch.ones(A, dtype=torch.float64) * 3, row).on("cpu", (B, Ta, A))
    assert torch.equal(k, torch.full((B, Ta, A), 3.0))
    k, _ = ActionPin(known[:1], row).on("cpu", (B, Ta, A))
    assert torch.equal(k[1], known[0])
    k, q = ActionPin([[0.5] * A], [0.0] * Ta).on("cpu", (B, Ta, A))
    assert torch.equal(k, torch.full((B, Ta, A), 0.5)) and not q.any()


def test_bad_pins_are_refused():
    B, Ta, A = 2, 10, 7
    known = torch.zeros(B, Ta, A)
    for bad in (1.5, -0.1, float("nan"), float("inf")):
        keep = torch.zeros(Ta)
        keep[4] = bad
        with pytest.raises(ValueError):
            ActionPin(known, keep)
    with pytest.raises(ValueError):
        ActionPin(torch.full((B, Ta, A), float("nan")), torch.zeros(Ta))
    with pytest.raises(ValueError):
        ActionPin(known, torch.zeros(B, Ta, A, 1))
    with pytest.raises(ValueError):
        ActionPin(known, torch.zeros(Ta)).on("cpu", (B, Ta + 1, A))  # a chunk of another length
    with pytest.raises(ValueError):
        ActionPin(known, torch.zeros(B + 1, Ta)).on("cpu", (B, Ta, A))
    with pytest.raises(ValueError):
        ActionPin.overlap(known, -1, 2)
    with pytest.raises(ValueError):
        ActionPin.overlap(known[0], 1, 2)


def test_apply_selects_at_both_ends():
    den = torch.tensor([[[float("inf"), -0.0, 2.0, 4.0]]])
    known = torch.tensor([[[1.0, 5.0, float(3), 8.0]]])
    keep = torch.tensor([[[0.0, 0.0, 1.0, 0.25]]])
    out = ActionPin(known, keep).apply(den)
    assert out[0, 0, 0] == float("inf")                                  # keep == 0: no 0 * inf
    assert out[0, 0, 1] == 0 and torch.signbit(out[0, 0, 1])             # ... and the sign of zero stays
    assert out[0, 0, 2] == 3.0 and out[0, 0, 3] == 4.0 + 0.25 * (8.0 - 4.0)


def test_overlap_against_a_hand_written_table():
    B, Ta, A = 2, 10, 3
    prev = torch.arange(B * Ta * A, dtype=torch.float32).reshape(B, Ta, A)
    pin = ActionPin.overlap(prev, executed=4, hard=2, soft=3)
    known, keep = pin.on("cpu", (B, Ta, A))
    table = [1.0, 1.0, 0.75, 0.5, 0.25, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert torch.equal(keep, torch.tensor(table).reshape(1, Ta, 1).expand(B, Ta, A))
    for j in range(Ta):
        want = prev[:, j + 4] if j + 4 < Ta else torch.zeros(B, A)
        assert torch.equal(known[:, j], want), j
    # the ramp is cut where the previous chunk ends: executed = 7 leaves three tokens
    _, keep = ActionPin.overlap(prev, executed=7, hard=2, soft=3).on("cpu", (B, Ta, A))
    assert keep[0, :, 0].tolist() == [1.0, 1.0, 0.75] + [0.0] * 7
    _, keep = ActionPin.overlap(prev, executed=0, hard=Ta + 5).on("cpu", (B, Ta, A))
    assert bool((keep == 1).all())
    _, keep = ActionPin.overlap(prev, executed=Ta, hard=2, soft=2).on("cpu", (B, Ta, A))
    assert not keep.any()


# ---- routing (no device) -------------------------------------------------------------------------------------------------------
def test_a_pin_alone_keeps_the_native_call_and_other_keys_do_not(monkeypatch):
    from mdt_policy_amd import configs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.models.networks._engine import rollout_controls
    calls = []
    monkeypatch.setattr(GCDenoiser, "sample_native", lambda self, kind, state, action, *a, **kw: calls.append((kind, kw)) or action)
    monkeypatch.setattr(GCDenoiser, "sample_ddim", lambda self, state, action, *a, **kw: calls.append(("ddim", kw)) or action)
    torch.manual_seed(0)
    model = GCDenoiser(configs.mdtv_default(), 0.5).eval()
    B, Ta, A = 2, 10, 7
    state, x, goal = {"state_images": torch.zeros(B, 3, 512), "modality": "lang"}, torch.randn(B, Ta, A), torch.zeros(B, 1, 512)
    pin = ActionPin(torch.ones(B, Ta, A), keep_of(Ta))
    assert rollout_controls(pin=pin) == (True, None, pin) and rollout_controls(pin=pin, cond_lambda=2.0)[:2] == (True, 2.0)
    assert rollout_controls(pin=pin, s_churn=0)[0] is False
    for name in NAMES:
        calls.clear()
        run(name, model, state, x, goal, extra_args={"pin": pin, "cond_lambda": 2.0})
        assert len(calls) == 1 and calls[0][0] == name, (name, calls)
        known, keep = calls[0][1]["pin"]
        assert torch.equal(known, torch.ones(B, Ta, A)) and torch.equal(keep[0, :, 0], keep_of(Ta))
        assert calls[0][1]["cond_lambda"] == 2.0


def test_forward_applies_the_pin_after_the_guidance(monkeypatch):
    from mdt_policy_amd import configs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    B, Ta, A = 2, 10, 7
    vals = {False: torch.full((B, Ta, A), 3.0), True: torch.full((B, Ta, A), 1.0)}
    orig = GCDenoiser.forward

    def base(self, state, action, goal, sigma, cond_lambda=1.0, pin=None, **kw):
        if pin is not None or float(cond_lambda) != 1.0:
            return orig(self, state, action, goal, sigma, cond_lambda=cond_lambda, pin=pin, **kw)
        return vals[bool(kw.get("uncond", False))]
    monkeypatch.setattr(GCDenoiser, "forward", base)
    torch.manual_seed(0)
    model = GCDenoiser(configs.mdtv_default(), 0.5).eval()
    known = torch.full((B, Ta, A), -2.0)
    out = model({}, torch.zeros(B, Ta, A), None, torch.ones(1), cond_lambda=2.5, pin=ActionPin(known, keep_of(Ta)))
    d_lam = 1.0 + 2.5 * 2.0
    assert torch.equal(out[:, :HARD], known[:, :HARD])
    assert torch.equal(out[:, HALF], torch.full((B, A), d_lam + 0.5 * (-2.0 - d_lam)))
    assert torch.equal(out[:, HALF + 1:], torch.full((B, Ta - HALF - 1, A), d_lam))


# ---- the host loops over the float64 oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_loop_with_a_pin_over_the_oracle(name):
    model, state, goal, x, _ = oracle_case()
    free, known, pin, pinned = oracle_loops(name)
    # (a) keep == 0 everywhere: the unpinned result, bit for bit
    none = run(name, model, state, x, goal, extra_args={"pin": ActionPin(known, torch.zeros(x.shape[1]))})
    assert torch.equal(none, free), f"{name}: an all-zero keep changed the result"
    # (b) the pinned elements end at known (dpm_fast: inside its sigma_min bound); (c) the others change
    conditions(name, free, pinned, known, keep_of(x.shape[1]), x)
    assert bool(torch.isfinite(pinned).all())
