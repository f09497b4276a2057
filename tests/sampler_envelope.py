"""Shared by tests/test_sampler_envelope.py (CPU), tests/test_gpu_sampler_envelope.py and tests/test_gpu_steer_plan_envelope.py:
the sampler options -- pin, bounds and record, guidance, candidates, steer (DDIM's and, at the end of the file, every plan
sampler's), denoise_vjp, log-likelihood -- on the configurations of tests/envelope_configs.ENVELOPE.

The reference of every comparison is the package's own host loop in gc_sampling run on the CPU over ``EnvelopeOracle``, a float64
denoiser built from oracle/mdt_oracle.py that composes the options the way GCDenoiser.forward does; it shares no kernel with the
native calls.  Weights and inputs are those of tests/test_gpu_config_envelope.py ("rich" synthetic weights, seed 5).

Schedule: get_sigmas_exponential(4, 1, 80), the one of test_action_pin and test_gpu_sampler_bounds.  No churn and no ancestral
noise (the generator streams of the two devices differ); dpmpp_sde gets its noise as one fixed tensor.  ``pattern`` gives the
per-element weights (1, 0.5, 0)[(b + t + c) % 3]: every lane of the action head, all three values from three samples on even at
Ta = A = 1.  ``known`` is the unpinned float64 result of another noise seed, negated."""
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.utils.action_pin import ActionPin
from mdt_policy_amd.utils.action_steer import ActionSteer
from oracle import mdt_oracle as O
from tests.envelope_configs import ENVELOPE
from tests.helpers import ATOL, RTOL, assert_close, observation, rich_model

NAMES = sorted(ENVELOPE)
GUIDED_NAMES = [n for n in NAMES if ENVELOPE[n]["cfg"].get("goal_conditioned", True)]
SD, LAM, BETA = 0.5, 2.5, 5.0
N, SMIN, SMAX = 4, 1.0, 80.0
STEER_SMIN = 0.01  # the steered trajectory's last level (see steered_ddim)
# the quantiles of the float64 unclamped result the bounds are taken at, per column (see tests/test_sampler_envelope.py)
Q_LO, Q_HI = 0.3, 0.7
KINDS = {"ddim": {}, "heun": dict(s_churn=0.), "dpmpp_2m": {}, "lms": {}, "dpmpp_sde": dict(eta=1.)}
SEED, OTHER_SEED = 31, 32  # of the inputs; of the noise behind ``known``
LL_NAMES = ["h1_d64_min", "a16_ctx16", "rope_ta16", "mdt_h6_a12", "proprio_ctx16", "plain_ta16"]
LL_SMIN, LL_SMAX = 0.001, 80.0

_PARAMS, _ORACLES, _LOOPS = {}, {}, {}


def sched():
    return gs.get_sigmas_exponential(N, SMIN, SMAX)


def shape_of(name):
    cfg = ENVELOPE[name]["cfg"]
    return cfg["action_seq_len"], cfg["action_dim"]


def params(name):
    """{state_dict name: float32 tensor}: test_gpu_config_envelope.model_of's weights, without a device."""
    if name not in _PARAMS:
        _PARAMS[name] = rich_model(ENVELOPE[name]["cfg"])[1]
    return _PARAMS[name]


def pattern(B, Ta, A, values=(1.0, 0.5, 0.0)):
    """(B, Ta, A) weights values[(b + t + c) % 3]."""
    b, t, c = torch.meshgrid(torch.arange(B), torch.arange(Ta), torch.arange(A), indexing="ij")
    return torch.tensor(values, dtype=torch.float32)[(b + t + c) % 3]


class EnvelopeOracle:
    """model(state, x, goal, sigma, cond_lambda=1.0, pin=None, steer=None, uncond=False) in float64 over O.denoise, composed as
    GCDenoiser.forward composes it: D_u + lambda (D_g - D_u) with D_u on the zeroed goal, then the pin (selects at keep == 0 and
    keep == 1) or the steer D + s(sigma) J^T (w (known - D)) by torch.autograd.  Differentiable in ``x``.  With adaLN
    conditioning the context does not depend on sigma or x: the one of the last (state, goal) pair is kept."""
    sigma_data = SD

    def __init__(self, name, case=None, P=None):
        """``case`` / ``P``: a configuration (cfg, arch) and weights from outside the envelope, for the cross-checks."""
        e = ENVELOPE[name] if case is None else case
        self.name, self.cfg, self.arch = name, e["cfg"], e["arch"]
        self.P = O.to_dtype(params(name) if P is None else P, torch.float64)
        self._held = None

    def _denoise(self, state, x, goal, sigma, uncond):
        ctx = None
        if self.cfg.get("use_ada_conditioning", False):
            if self._held is None or self._held[0] is not state or self._held[1] is not goal:
                self._held = (state, goal, {})
            ctxs = self._held[2]
            if uncond not in ctxs:
                st = {k: (v.double() if torch.is_tensor(v) else v) for k, v in state.items()}
                g = goal.double()
                with torch.no_grad():
                    ctxs[uncond] = O.encode(self.P, self.cfg, st, torch.zeros_like(g) if uncond else g, self.arch)
            ctx = ctxs[uncond]
            st, g = state, goal  # not read
        else:
            st = {k: (v.double() if torch.is_tensor(v) else v) for k, v in state.items()}
            g = torch.zeros_like(goal.double()) if uncond else goal.double()
        return O.denoise(self.P, self.cfg, st, x, g, sigma, SD, self.arch, ctx)

    def base(self, state, x, goal, sigma, cond_lambda=1.0, uncond=False):
        lam = float(cond_lambda)
        if lam == 1.0:
            return self._denoise(state, x, goal, sigma, bool(uncond))
        assert not uncond
        d_u = self._denoise(state, x, goal, sigma, True)
        return d_u + lam * (self._denoise(state, x, goal, sigma, False) - d_u)

    def __call__(self, state, x, goal, sigma, cond_lambda=1.0, pin=None, steer=None, uncond=False):
        x = x.double()
        sigma = torch.as_tensor(sigma).double().reshape(-1).expand(x.shape[0])
        if steer is not None:
            assert pin is None and float(cond_lambda) == 1.0
            return self.steered(state, x, goal, sigma, steer)[0]
        den = self.base(state, x, goal, sigma, cond_lambda, uncond)
        if pin is None:
            return den
        known, keep = (t.double() for t in pin.on(den.device, den.shape))
        return torch.where(keep == 0, den, torch.where(keep == 1, known, den + keep * (known - den)))

    def steered(self, state, x, goal, sigma, steer):
        """(D', D, J^T e), e = w (known - D) a constant of the evaluation (tests/test_gpu_steer.oracle_steered)."""
        with torch.enable_grad():
            xg = x.detach().double().requires_grad_()
            d = self.base(state, xg, goal, sigma)
            known, w = steer.on("cpu", tuple(x.shape))
            e = w.double() * (known.double() - d.detach())
            j, = torch.autograd.grad((d * e).sum(), xg)
        s = steer.scale(sigma, SD).reshape(-1, 1, 1)
        return d.detach() + s * j, d.detach(), j

    def vjp(self, state, x, goal, sigma, v):
        """(D, (dD/dx)^T v) by float64 autograd."""
        xg = x.detach().double().requires_grad_()
        with torch.enable_grad():
            d = self(state, xg, goal, sigma)
            j, = torch.autograd.grad((d * v.double()).sum(), xg)
        return d.detach(), j


def oracle_of(name):
    if name not in _ORACLES:
        _ORACLES[name] = EnvelopeOracle(name)
    return _ORACLES[name]


def case(name, B, seed=SEED):
    """(state, goal, x_T, fixed noise) in float32 on the host; x_T = 80 noise."""
    e = ENVELOPE[name]
    state, goal, noise = observation(e["cfg"], e["arch"], e["proprio"], B, seed)
    fixed = torch.from_numpy(synthetic.normal("sde_noise", tuple(noise.shape), seed + 100))
    return state, goal, noise * SMAX, fixed


def run(kind, model, state, x, goal, fixed, sig=None, **kw):
    """One sampler call through gc_sampling: the host loop for an EnvelopeOracle, the native call for a GCDenoiser."""
    kw = dict(KINDS[kind], **kw)
    if kind == "dpmpp_sde":
        kw["noise_sampler"] = lambda s0, s1: fixed.to(device=x.device, dtype=x.dtype)
    with torch.no_grad():
        return getattr(gs, "sample_" + kind)(model, state, x, goal, sched() if sig is None else sig, **kw)


def wide(t):
    return {k: (v.double() if torch.is_tensor(v) else v) for k, v in t.items()} if isinstance(t, dict) else t.double()


def loops(name, kind, B, lam=1.0, repeat=1):
    """(free, known, pinned) float64 host-loop results of a configuration, kind and batch, computed once and left unchanged:
    unpinned; the unpinned result of the other noise seed, negated; pinned with keep = pattern (over the B * repeat rows).
    ``lam``: the guidance weight of all three.  ``repeat`` = K: the B observations are repeated K times (repeat_interleave) and
    every one of the B * K rows has its own noise -- what a candidates call computes."""
    key = (name, kind, B, lam, repeat)
    if key not in _LOOPS:
        model = oracle_of(name)
        state, goal, x, fixed, x_other = chunk_case(name, B, repeat)
        if repeat != 1:
            state = {k: (v.repeat_interleave(repeat, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
            goal = goal.repeat_interleave(repeat, 0)
        state, goal, x, fixed, x_other = wide(state), wide(goal), wide(x), wide(fixed), wide(x_other)
        ea = {} if lam == 1.0 else {"cond_lambda": lam}
        free = run(kind, model, state, x, goal, fixed, extra_args=dict(ea))
        known = -run(kind, model, state, x_other, goal, fixed, extra_args=dict(ea))
        pin = ActionPin(known, pattern(*x.shape))
        pinned = run(kind, model, state, x, goal, fixed, extra_args=dict(ea, pin=pin))
        _LOOPS[key] = (free, known, pinned)
    return _LOOPS[key]


def chunk_case(name, B, repeat=1):
    """(state, goal of the B observations; x_T, fixed noise, x_T of the other seed of the B * repeat rows), float32."""
    state, goal, _, _ = case(name, B)
    _, _, x, fixed = case(name, B * repeat)
    _, _, x_other, _ = case(name, B * repeat, OTHER_SEED)
    return state, goal, x, fixed, x_other


def pin_of(name, kind, B, lam=1.0, repeat=1):
    """The ActionPin of ``loops`` (it holds known and keep in float32, what the native call reads)."""
    _, known, _ = loops(name, kind, B, lam, repeat)
    return ActionPin(known, pattern(*known.shape))


def tol_of(t, atol=ATOL, rtol=RTOL):
    return atol + rtol * float(t.abs().max()) if t.numel() else atol


def conditions(what, free, pinned, known, keep, atol=ATOL, rtol=RTOL, lone=False):
    """test_action_pin.conditions for an element mask ``keep`` (B, Ta, A): pinned and unpinned differ by more than 100 x the
    tolerance on the keep == 1 elements and by more than 10 x on the keep == 0 ones, the tolerance of a set being
    atol + rtol max |pinned| over it; the keep == 1 elements land on ``known``.  ``lone``: every sample is a single element, so a
    keep == 0 sample cannot feel the pin -- there the pinned result must equal the unpinned one."""
    free, pinned, known = (t.detach().double().cpu() for t in (free, pinned, known))
    hard, rest = keep == 1, keep == 0
    assert bool(hard.any()) and bool(rest.any()) and bool(((keep > 0) & (keep < 1)).any()), f"{what}: keep lacks a value"
    gap_pin, gap_rest = float((pinned - free)[hard].abs().max()), float((pinned - free)[rest].abs().max())
    tol_pin, tol_rest = tol_of(pinned[hard], atol, rtol), tol_of(pinned[rest], atol, rtol)
    print(f"{what}: |pinned - unpinned| max {gap_pin:.4f} on keep == 1 (100 tol {100 * tol_pin:.4f}), {gap_rest:.4f} on keep == 0 "
          f"(10 tol {10 * tol_rest:.4f})")
    assert gap_pin > 100 * tol_pin, f"{what}: pinned and unpinned differ by {gap_pin:.3e} only on the pinned elements"
    if lone:
        assert torch.equal(pinned[rest], free[rest]), f"{what}: a keep == 0 sample of one element changed under the pin"
    else:
        assert gap_rest > 10 * tol_rest, f"{what}: pinned and unpinned differ by {gap_rest:.3e} only on the keep == 0 elements"
    assert_close(pinned[hard], known[hard], rtol=rtol, atol=atol, what=f"{what}: pinned elements")
    return gap_pin, gap_rest


def is_lone(name):
    return shape_of(name) == (1, 1)


# ---- bounds -------------------------------------------------------------------------------------------------------------------
class ClampOnly:
    """tests/test_gpu_sampler_bounds.ClampOnly: clip_output alone, counting the share of elements each call changed."""

    def __init__(self, lo, hi):
        self.lo, self.hi, self.changed = lo, hi, []

    def clip_output(self, x):
        y = torch.clamp(x, self.lo.to(x), self.hi.to(x))
        self.changed.append(float((y != x).double().mean()))
        return y


def quantile_bounds(unclamped):
    """Per-column Q_LO / Q_HI quantiles, as float32 (what the native call reads)."""
    rows = unclamped.reshape(-1, unclamped.shape[-1]).double()
    return torch.quantile(rows, Q_LO, dim=0).float(), torch.quantile(rows, Q_HI, dim=0).float()


def bounded(name, kind, B, pinned=False):
    """(lo, hi, clamped float64 result, [(x, denoised)] of every step, share changed per step, unclamped result), computed once:
    the bounds come from the unclamped loop of the same options."""
    key = (name, kind, B, "bounds", pinned)
    if key not in _LOOPS:
        model = oracle_of(name)
        state, goal, x, fixed, _ = chunk_case(name, B)
        state, goal, x, fixed = wide(state), wide(goal), wide(x), wide(fixed)
        free, _, with_pin = loops(name, kind, B)
        ea = {"pin": pin_of(name, kind, B)} if pinned else {}
        plain = with_pin if pinned else free
        lo, hi = quantile_bounds(plain)
        scaler, seen = ClampOnly(lo, hi), []
        want = run(kind, model, state, x, goal, fixed, scaler=scaler, extra_args=ea,
                   callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
        _LOOPS[key] = (lo, hi, want, seen, list(scaler.changed), plain)
    return _LOOPS[key]


# ---- steer --------------------------------------------------------------------------------------------------------------------
def steer_of(name, B):
    """ActionSteer(known, pattern with (1, 0.25, 0), BETA); ``known`` is the DDIM loops'."""
    _, known, _ = loops(name, "ddim", B)
    return ActionSteer(known, pattern(*known.shape, values=(1.0, 0.25, 0.0)), BETA)


def werr(steer, out):
    known, w = steer.on("cpu", tuple(out.shape))
    return float((w.double() * (known.double() - out.double().cpu()) ** 2).sum())


def steered_ddim(name, B, n=3):
    """(steered, unsteered) float64 n-step sample_ddim host loops, computed once.  The schedule ends at STEER_SMIN = 0.01, far
    below sigma_data: there J = dD/dx is c_skip I to O(sigma) and s(sigma) is 1, so the last evaluation's steer is
    D + weight (known - D) and must lower the weighted error -- at a last level of 1 (c_skip = 0.2, s = 5) the sign of the effect
    is the random network's (measured: plain_ta16 111.1 -> 118.4)."""
    key = (name, "steer", B, n)
    if key not in _LOOPS:
        model = oracle_of(name)
        state, goal, x, _, _ = chunk_case(name, B)
        state, goal, x = wide(state), wide(goal), wide(x)
        sig = gs.get_sigmas_exponential(n, STEER_SMIN, SMAX)
        with torch.no_grad():
            plain = gs.sample_ddim(model, state, x, goal, sig)
            steered = gs.sample_ddim(model, state, x, goal, sig, extra_args={"steer": steer_of(name, B)})
        _LOOPS[key] = (steered, plain)
    return _LOOPS[key]


# ---- log-likelihood -----------------------------------------------------------------------------------------------------------
def signs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def loglik_case(name, B=2, K=3):
    """(state, goal of the B observations; the B * K chunks to score -- the DDIM result of another seed plus 0.3 N(0, 1) on all but
    chunk 0 of every observation; one sign probe), float32."""
    Ta, A = shape_of(name)
    state, goal, _, _ = case(name, B)
    base = -loops(name, "ddim", B)[1].float()
    rows = base.repeat_interleave(K, 0).clone()
    jitter = torch.from_numpy(synthetic.normal("ll_chunks", tuple(rows.shape), 33))
    first = (torch.arange(B * K) % K == 0)[:, None, None]
    return state, goal, torch.where(first, rows, rows + 0.3 * jitter), signs((B * K, Ta, A), 34)


def loglik_reference(name, monkeypatch, B=2, K=3):
    """(ll, latent, delta, info) of gs.log_likelihood's autograd branch over the oracle on the expanded observations, in float64,
    computed once.  ``latent`` and ``delta`` are taken from the integrator the branch runs (gs._dopri5, wrapped for the call)."""
    key = (name, "loglik", B, K)
    if key not in _LOOPS:
        state, goal, rows, v = loglik_case(name, B, K)
        st = {k: (t.repeat_interleave(K, 0) if torch.is_tensor(t) else t) for k, t in state.items()}
        kept, inner = {}, gs._dopri5

        def keeping(*a, **kw):
            kept["y"] = inner(*a, **kw)
            return kept["y"]
        with monkeypatch.context() as mp:
            mp.setattr(gs, "_probe_signs", lambda a: v.to(a))
            mp.setattr(gs, "_dopri5", keeping)
            ll, info = gs.log_likelihood(oracle_of(name), wide(st), rows.double(), goal.repeat_interleave(K, 0).double(),
                                         LL_SMIN, LL_SMAX)
        _LOOPS[key] = (ll, kept["y"][0], kept["y"][1], dict(info))
    return _LOOPS[key]


# ---- the steered plan samplers (mdt_sample_steer) --------------------------------------------------------------------------------
# (a) the kinds without noise rows, through gc_sampling's own loop: kind -> (sample_<kind>'s keyword arguments, steps of 80 -> 1)
PLAN_KINDS = {"heun": (dict(s_churn=0.), N), "dpmpp_2m": ({}, N), "lms": (dict(order=4), 6), "dpmpp_sde": (dict(eta=1.), N)}
PLAN_CASES = [(n, k) for k in ("heun", "dpmpp_2m") for n in NAMES] + [(n, k) for k in ("lms", "dpmpp_sde") for n in LL_NAMES]
# (b) the kinds that read noise rows, through the plan interpreter: tag -> (kind, parameters, dpm_fast's evaluation count)
NOISE_NAMES = ["h1_d64_min", "a16_ctx16", "mdt_h6_a12"]
NOISE_KINDS = {"euler_churn": ("euler", dict(s_churn=1.0), None), "heun_churn": ("heun", dict(s_churn=1.0, s_noise=0.9), None),
               "euler_ancestral": ("euler_ancestral", {}, None), "dpm_2_ancestral": ("dpm_2_ancestral", {}, None),
               "dpmpp_2s_ancestral": ("dpmpp_2s_ancestral", {}, None), "dpm_fast_6": ("dpm_fast", {}, 6)}
# (c) bounds: the kinds whose loops clip after every step, and the one that never reads its scaler
CLIP_NAMES = ["a16_ctx16", "mdt_h6_a12"]
CLIP_KINDS = {"heun": dict(s_churn=0.), "dpm_2": dict(s_churn=0.)}


def plan_sched(kind):
    return gs.get_sigmas_exponential(PLAN_KINDS[kind][1] if kind in PLAN_KINDS else N, SMIN, SMAX)


def native_steer(steer):
    """The same steer asking for the native plan call (mdt_sample_steer)."""
    return ActionSteer(steer.known, steer.weight, steer.beta, plan_native=True)


def steer_gate(want):
    """The project's gate for steered trajectories, per element: (1 + beta) (ATOL + RTOL |want|)."""
    return (1 + BETA) * (ATOL + RTOL * want.detach().double().abs())


def werr_bound(steer, want):
    """|E(native) - E(want)| <= sum W (2 |known - want| t + t^2), t the per-element gate (tests/test_gpu_steer_plan.py)."""
    known, w = steer.on("cpu", tuple(want.shape))
    t = steer_gate(want)
    return float((w.double() * (2 * (known.double() - want).abs() * t + t * t)).sum())


def run_plan_loop(kind, model, state, x, goal, fixed, sig, extra_args=None, scaler=None, callback=None, **params):
    """gc_sampling's sample_<kind> (dpmpp_sde: the fixed noise tensor) with the given parameters."""
    kw = dict(params)
    if kind == "dpmpp_sde":
        kw["noise_sampler"] = lambda s0, s1: fixed.to(device=x.device, dtype=x.dtype)
    if scaler is not None:
        kw["scaler"] = scaler
    if callback is not None:
        kw["callback"] = callback
    with torch.no_grad():
        return getattr(gs, "sample_" + kind)(model, state, x, goal, sig, extra_args=dict(extra_args or {}), **kw)


def steered_plan(name, kind, B, x_scale=None):
    """(steered, unsteered) float64 host loops of a noise-free kind under steer_of(name, B), computed once.  ``x_scale``: x_T is
    multiplied by it and nothing is kept (the conditioning check of the CPU tier); only the steered result is returned."""
    key = (name, "steer_plan", kind, B)
    if key in _LOOPS and x_scale is None:
        return _LOOPS[key]
    model = oracle_of(name)
    state, goal, x, fixed, _ = chunk_case(name, B)
    state, goal, x, fixed = wide(state), wide(goal), wide(x), wide(fixed)
    params, sig = (PLAN_KINDS[kind][0] if kind in PLAN_KINDS else CLIP_KINDS[kind]), plan_sched(kind)
    ea = {"steer": steer_of(name, B)}
    if x_scale is not None:
        return run_plan_loop(kind, model, state, x * x_scale, goal, fixed, sig, ea, **params)
    _LOOPS[key] = (run_plan_loop(kind, model, state, x, goal, fixed, sig, ea, **params),
                   run_plan_loop(kind, model, state, x, goal, fixed, sig, **params))
    return _LOOPS[key]


class never_forward_steered:
    """Inside: GCDenoiser._steered counts its calls; the native plan call makes none (tests/test_gpu_steer_plan.both_ways)."""

    def __enter__(self):
        from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
        self.cls, self.kept, self.calls = GCDenoiser, GCDenoiser._steered, []
        kept, calls = self.kept, self.calls
        GCDenoiser._steered = lambda this, *a, **k: calls.append(1) or kept(this, *a, **k)
        return self

    def __exit__(self, *exc):
        self.cls._steered = self.kept
        return False


def noise_rows(tag, shape, n):
    """(n,) + shape explicit noise rows of a case (b)."""
    return torch.from_numpy(synthetic.normal("steer_plan_rows_" + tag, (n,) + tuple(shape), 35))


def noise_plan(tag):
    """(kind, parameters, n_steps for dpm_fast, host schedule, plan) of a kind that reads noise rows."""
    from mdt_policy_amd import _lib
    kind, params, n = NOISE_KINDS[tag]
    sig = [SMAX, SMIN] if kind == "dpm_fast" else sched().tolist()
    return kind, params, n, sig, _lib.sampler_plan(kind, sig, n_steps=n, **params)


def chunk_steer(name, B, K):
    """A per-chunk steer over the B * K rows: steer_of(name, B)'s known of the chunk's observation plus 0.1 N(0, 1) of its own."""
    base = steer_of(name, B)
    known = base.known.repeat_interleave(K, 0)
    known = known + 0.1 * torch.from_numpy(synthetic.normal("steer_plan_chunks", tuple(known.shape), 36))
    return ActionSteer(known, pattern(*known.shape, values=(1.0, 0.25, 0.0)), BETA)


def interpreted(name, tag, B, K=1):
    """(result, [(step, Y, D')] of the evaluations that begin a step, rows, steer) of the float64 plan interpreter
    (tests/steer_ops_cases.apply_plan) with D' from EnvelopeOracle.steered on the expanded observations, computed once."""
    key = (name, "steer_interp", tag, B, K)
    if key not in _LOOPS:
        from tests.steer_ops_cases import apply_plan
        kind, params, n, sig, plan = noise_plan(tag)
        model = oracle_of(name)
        state, goal, x, _, _ = chunk_case(name, B, K)
        if K != 1:
            state = {k: (v.repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
            goal = goal.repeat_interleave(K, 0)
        state, goal = wide(state), wide(goal)
        steer = steer_of(name, B) if K == 1 else chunk_steer(name, B, K)
        rows = noise_rows(tag, x.shape, plan.n_noise)
        R = x.shape[0]

        def dprime(Y, sigma, k):
            return model.steered(state, torch.from_numpy(Y), goal, torch.full((R,), float(sigma), dtype=torch.float64), steer)[0].numpy()
        out, seen = apply_plan(plan, x.double().numpy(), rows.double().numpy(), dprime)
        begins = [(plan.e[k].step, torch.from_numpy(seen[k][0]), torch.from_numpy(seen[k][1])) for k in range(plan.n_evals)
                  if plan.e[k].begins_step]
        _LOOPS[key] = (torch.from_numpy(out), begins, rows, steer)
    return _LOOPS[key]


def steered_bounded(name, kind, B):
    """(lo, hi, clamped float64 steered loop, share changed per step, unclamped steered loop), computed once: the ``bounded``
    pattern under steer_of(name, B), the bounds at the quantiles of the unclamped steered result."""
    key = (name, "steer_bounds", kind, B)
    if key not in _LOOPS:
        model = oracle_of(name)
        state, goal, x, fixed, _ = chunk_case(name, B)
        state, goal, x, fixed = wide(state), wide(goal), wide(x), wide(fixed)
        plain = steered_plan(name, kind, B)[0]
        lo, hi = quantile_bounds(plain)
        scaler = ClampOnly(lo, hi)
        params = PLAN_KINDS[kind][0] if kind in PLAN_KINDS else CLIP_KINDS[kind]
        want = run_plan_loop(kind, model, state, x, goal, fixed, plan_sched(kind), {"steer": steer_of(name, B)}, scaler=scaler, **params)
        _LOOPS[key] = (lo, hi, want, list(scaler.changed), plain)
    return _LOOPS[key]
