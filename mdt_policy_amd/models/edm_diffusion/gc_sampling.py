"""Noise schedules and samplers (reference: mdt/models/edm_diffusion/gc_sampling.py).

``sample_ddim`` -- the sampler MDT ships with (conf/model/mdtv_agent.yaml:14) -- runs as ONE call into
libmdt_hip.so when ``model`` is this package's GCDenoiser and no Python hooks are requested: encoder and
cross-attention K/V once, adaLN vectors of all steps once, the DDIM update fused into the action-head kernel.
The other fixed-step samplers (euler, heun, the ancestral ones, dpm_2, lms, dpmpp_2m / 2s / sde) run the same way --
one call, ``GCDenoiser.sample_native`` -> mdt_sample -- under the same condition and with ``scaler`` None or an object that
exposes its bounds (``clip_bounds``, utils/action_bounds.py ActionBounds: the call clamps inside), and so does
sample_dpm_fast (1..128 evaluations); sample_dpm_adaptive with eta = 0 on the GPU is one blocking call
(``GCDenoiser.sample_dpm_adaptive_native`` -> mdt_sample_dpm_adaptive).  Otherwise they are host loops over
``model(state, x, goal, sigma)`` (the HIP denoiser step) with the sigma-independent encoder hoisted out of the loop.
Every sampler takes ``extra_args={"steer": ActionSteer}`` (utils/action_steer.py: D' = D + s(sigma) J^T (weight (known - D)));
sample_ddim, and sample_euler without churn, then run as one native call (``GCDenoiser.sample_steered`` -> mdt_sample_ddim_steer)
when the only other key is ``candidates``; with ``ActionSteer(..., plan_native=True)`` every other fixed-step sampler does too
(-> mdt_sample_steer, with the noise rows its unsteered native call draws, on a host schedule).  Without that flag, and for
sample_dpm_adaptive, a ``callback`` or a scaler without ``clip_bounds``, they are host loops whose ``model(...)`` calls get the key.
``log_likelihood`` with this package's GCDenoiser is one blocking call too (``GCDenoiser.log_likelihood`` ->
mdt_log_likelihood), for K chunks per observation and P probes; ``best_candidates`` picks from its result.
``denoising_score`` is the forwards-only scorer beside it: the chunks' likelihood-weighted denoising error over a few noise
levels as one enqueue (``GCDenoiser.denoising_score`` -> mdt_denoising_score), no tape, no read-back, capturable.

Signatures follow the reference: ``sample_*(model, state, action, goal, sigmas, scaler=None, extra_args=None,
callback=None, disable=None, ...)``.
"""
from __future__ import annotations

import ctypes
import math
import os
from contextlib import nullcontext

import numpy as np
import torch

from . import utils
from ... import _lib
from ..networks._engine import candidate_count, chunk_rows, rollout_controls, steer_alone, take_candidates, take_steer
from .graphed import GraphedDDIM, GraphedSampler, GraphedSelect
from .score_wrappers import GCDenoiser, draw_score_noise


# ------------------------------------------------------------------------------------------------
# schedules (reference gc_sampling.py:22-88); all return n+1 values ending in 0
# ------------------------------------------------------------------------------------------------
def append_zero(action):
    return torch.cat([action, action.new_zeros([1])])


def get_sigmas_karras(n, sigma_min, sigma_max, rho=7., device='cpu'):
    """Karras et al. (2022) schedule: linear ramp in sigma^(1/rho)."""
    ramp = torch.linspace(0, 1, n)
    lo, hi = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
    return append_zero((hi + ramp * (lo - hi)) ** rho).to(device)


def get_sigmas_exponential(n, sigma_min, sigma_max, device='cpu'):
    """Geometric schedule: linear ramp in log sigma (the MDT default, mdtv_agent.yaml:18)."""
    return append_zero(torch.linspace(math.log(sigma_max), math.log(sigma_min), n, device=device).exp())


def get_sigmas_linear(n, sigma_min, sigma_max, device='cpu'):
    return append_zero(torch.linspace(sigma_max, sigma_min, n, device=device))


def cosine_beta_schedule(n, s=0.008, device='cpu'):
    """Cosine beta schedule, flipped and clipped (reference gc_sampling.py:47-58)."""
    steps = n + 1
    x = np.linspace(0, steps, steps)
    acp = np.cos(((x / steps) + s) / (1 + s) * np.pi * 0.5) ** 2
    acp = acp / acp[0]
    betas = np.clip(1 - (acp[1:] / acp[:-1]), a_min=0, a_max=0.999)
    return append_zero(torch.tensor(np.flip(betas).copy(), device=device, dtype=torch.float32))


def get_sigmas_ve(n, sigma_min=0.02, sigma_max=100, device='cpu'):
    """Variance-exploding schedule incl. the reference's linspace(0, n+1, n) parametrisation (:61-69)."""
    t = torch.linspace(0, n + 1, n, device=device)
    t = (sigma_max ** 2) * ((sigma_min ** 2 / sigma_max ** 2) ** (t / (n - 1)))
    return append_zero(torch.sqrt(t))


def get_iddpm_sigmas(n, sigma_min=0.02, sigma_max=100, M=1000, j_0=0, C_1=0.001, C_2=0.008, device='cpu'):
    """Improved-DDPM schedule (reference gc_sampling.py:71-81): u_{j-1} from the cosine alpha-bar recursion, the
    levels inside [sigma_min, sigma_max] sub-sampled at n evenly spaced (rounded) indices.  As in the reference the
    alpha-bar ratios are float32 (Python float x integer tensor promotes to the default dtype) and only the
    recursion itself runs in float64 -- the ratios near j = M sit within rounding of 1, so this matters at 1e-4."""
    j = torch.arange(0, M + 1, device=device)
    abar = (0.5 * np.pi * j / M / (C_2 + 1)).sin() ** 2              # float32
    ratio = (abar[:-1] / abar[1:]).clip(min=C_1)                     # ratio[j-1] = abar(j-1) / abar(j)
    u = torch.zeros(M + 1, dtype=torch.float64, device=device)
    for jj in range(M, j_0, -1):
        u[jj - 1] = ((u[jj] ** 2 + 1) / ratio[jj - 1] - 1).sqrt()
    kept = u[torch.logical_and(u >= sigma_min, u <= sigma_max)]
    idx = ((len(kept) - 1) / (n - 1) * torch.arange(n, dtype=torch.float64, device=device)).round().to(torch.int64)
    return append_zero(kept[idx]).to(torch.float32)


def get_sigmas_vp(n, beta_d=19.9, beta_min=0.1, eps_s=1e-3, device='cpu'):
    t = torch.linspace(1, eps_s, n, device=device)
    return append_zero(torch.sqrt(torch.exp(beta_d * t ** 2 / 2 + beta_min * t) - 1))


def to_d(action, sigma, denoised):
    """Karras ODE derivative dx/dsigma = (x - D(x; sigma)) / sigma."""
    if torch.is_tensor(sigma) and sigma.ndim > 0:
        return (action - denoised) / utils.append_dims(sigma.to(action.device), action.ndim)
    return (action - denoised) / _f(sigma)


def default_noise_sampler(x):
    return lambda sigma, sigma_next: torch.randn_like(x)


def get_ancestral_step(sigma_from, sigma_to, eta=1.):
    """Split a step into a deterministic part down to sigma_down and fresh noise sigma_up."""
    if not eta:
        return sigma_to, 0.
    sigma_up = min(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


# ------------------------------------------------------------------------------------------------
# samplers
# ------------------------------------------------------------------------------------------------
def _hoist(model, state, goal):
    """Encoder-once context for this package's denoiser; a no-op for any other callable."""
    if isinstance(model, GCDenoiser):
        return model.cached_context(state, goal)
    return nullcontext()


def _t(sigma):
    return sigma.log().neg()


def _sigma(t):
    return t.neg().exp()


def _host(sigmas):
    """Schedules are tiny: keep their scalar arithmetic on the host (fp32 0-dim CPU tensors, exactly the reference's
    expressions) so that no step of a sampler loop waits on the device for a scalar."""
    return sigmas.detach().to("cpu", torch.float32) if torch.is_tensor(sigmas) else torch.tensor(sigmas, dtype=torch.float32)


def _f(x):
    """0-dim fp32 host tensor (or number) -> Python float (exact), usable against tensors on any device."""
    return x.item() if torch.is_tensor(x) else float(x)


def _sig_in(sigma, action, model=None):
    """sigma * s_in of the reference.  This package's denoiser takes the single shared value (one adaLN row for the
    whole batch, broadcast inside the kernels); any other model gets the reference's (B,) vector."""
    n = 1 if isinstance(model, GCDenoiser) else action.shape[0]
    return torch.full((n,), _f(sigma), device=action.device, dtype=action.dtype)


# MDT_HIP_GRAPH: "1" = every fused DDIM call replays a HIP graph, "0" = never, unset = "auto": rollout-sized batches (B <= 8)
# from the third call with the same shapes on -- a rollout repeats one call for hundreds of steps (mdtv_agent.py:721-760) and
# its ~250 launches take the host longer to submit than the GPU to run (B = 1, host-synchronised: 1.56 ms eager, 1.43 ms
# replayed; tools/graph_probe.py), a one-off call is not worth a capture
_GRAPH_MODE = os.environ.get("MDT_HIP_GRAPH", "auto")
_GRAPH_SAMPLER = _GRAPH_MODE not in ("", "0", "auto")
_GRAPH_AUTO_MAX_BATCH, _GRAPH_AUTO_AFTER = 8, 2


def _graph_key(state, action, goal, sigmas):
    """Hashable for any `state` content: tensors by shape, everything else by type and repr (a list or dict value is legal)."""
    return (tuple(action.shape), tuple(goal.shape), len(sigmas),
            tuple(sorted((str(k), tuple(v.shape) if torch.is_tensor(v) else (type(v).__name__, repr(v)))
                         for k, v in state.items())))


def _graph_wanted(model, state, action, goal, sigmas, tag=None) -> bool:
    if action.device.type != "cuda" or model.inner_model.training or torch.cuda.is_current_stream_capturing():
        return False
    if _GRAPH_SAMPLER:
        return True
    if _GRAPH_MODE != "auto" or action.shape[0] > _GRAPH_AUTO_MAX_BATCH:
        return False
    key = _graph_key(state, action, goal, sigmas)
    if tag is not None:
        key = (tag,) + key
    if key in model.__dict__.get("_graph_failed", ()):
        return False  # a capture of this call failed once: it stays eager
    seen = model.__dict__.setdefault("_graph_seen", {})
    seen[key] = seen.get(key, 0) + 1
    if len(seen) > 16:
        seen.clear()
    return seen.get(key, 0) > _GRAPH_AUTO_AFTER


def _graph_route(model, cache, tag, key, state, action, goal, sigmas, make, what, noise=None, bounds=None, pin=None):
    """A native sampler call replayed as a HIP graph, or None: the eager call runs then.  The rule is _graph_wanted's, ``tag``
    joining the call's graph key (None: unguided DDIM).  The graphs live on the model in the list ``cache`` (at most four) and
    are found by GraphedDDIM.matches with ``key``; ``make(sigmas)`` captures a new one.  In auto mode a capture that fails
    (another thread allocating / synchronising while torch's global capture mode is on, ...) must not break a rollout the eager
    path would have served: that call shape stays eager, with a warning naming ``what``.  MDT_HIP_GRAPH=1 re-raises.
    ``bounds``: the call's (lo, hi) action bounds (a graph captured with bounds copies them in before it replays); ``pin``: its
    (known, keep) pinned actions, handled the same way."""
    if not _graph_wanted(model, state, action, goal, sigmas, tag=tag):
        return None
    kw = {} if bounds is None else {"bounds": bounds}
    if pin is not None:
        kw["pin"] = pin
    try:
        graphs = model.__dict__.setdefault(cache, [])
        for gsamp in graphs:
            if gsamp.matches(state, action, goal, sigmas, key=key, noise=noise):
                return gsamp(state, action, goal, sigmas, noise=noise, **kw)
        gsamp = make(sigmas if torch.is_tensor(sigmas) else torch.as_tensor(sigmas))
        graphs.append(gsamp)
        del graphs[:-4]
        return gsamp(state, action, goal, sigmas, noise=noise, **kw)  # the same launches, replayed as a HIP graph
    except Exception as exc:  # noqa: BLE001 -- whatever the capture raised, the eager launches still work
        if _GRAPH_SAMPLER:
            raise
        failed = _graph_key(state, action, goal, sigmas)
        model.__dict__.setdefault("_graph_failed", set()).add(failed if tag is None else (tag,) + failed)
        model.__dict__.pop(cache, None)
        import warnings
        warnings.warn(f"mdt_policy_amd: HIP-graph capture of {what} failed ({exc!r}); this call shape stays eager")
        torch.cuda.synchronize()
        return None


# ------------------------------------------------------------------------------------------------
# The other samplers' native path (GCDenoiser.sample_native -> mdt_sample): the whole loop as one enqueue, under the condition
# sample_ddim uses.  clip_output is not linear, so it cannot ride in the plan's coefficients: a scaler that exposes its bounds
# (a callable ``clip_bounds(device)`` -> (lo, hi), ActionBounds) has them applied by the plan head on the evaluation that ends
# a step (mdt_sample_opt); any other scaler object keeps the host loop.  The noise is drawn here, by torch, with the shapes, count and
# order of the host loop, so a seeded call gives the loop's result and leaves the generator where the loop leaves it.  The
# plan the call builds assumes what every get_sigmas_* guarantees -- all levels > 0 but a final 0 -- which a host schedule is
# checked for (else: the host loop); a device schedule is read in place, unchecked.
# ------------------------------------------------------------------------------------------------
def _scaler_native(scaler) -> bool:
    """Whether a sampler's ``scaler`` leaves the native call possible: none, or one whose bounds the call can apply itself."""
    return scaler is None or callable(getattr(scaler, "clip_bounds", None))


def _controls(extra_args):
    """(native, lam, pin, K) of a sampler's ``extra_args``: ``candidates`` = K comes off first (take_candidates), the rest is
    rollout_controls'.  K chunks per observation ride in the native call with a weight and a pin; any further key keeps the host
    loop, whose ``model(...)`` calls get all of them -- GCDenoiser.forward expands the observations there."""
    K, rest = take_candidates(extra_args)
    return rollout_controls(**rest) + (K,)


class _SteeredModel:
    """A foreign denoiser (any callable that is no GCDenoiser) under a steer: D' = D + s(sigma) J^T (weight (known - D)) with
    J^T e from torch.autograd inside torch.enable_grad(), as log_likelihood differentiates such a model.  sigma_data is the
    model's own attribute of that name, 1 without one."""

    def __init__(self, model, steer):
        self.model, self.steer = model, steer
        self.sigma_data = float(getattr(model, "sigma_data", 1.0))

    def __call__(self, state, x, goal, sigma, **kw):
        with torch.enable_grad():
            xg = x.detach().requires_grad_()
            den = self.model(state, xg, goal, sigma, **kw)
            e = self.steer.error(den.detach(), candidate_count(kw.get("candidates")))
            jte, = torch.autograd.grad((den * e).sum(), xg)
        sig = torch.as_tensor(sigma, dtype=x.dtype, device=x.device).reshape(-1)
        return den.detach() + utils.append_dims(self.steer.scale(sig, self.sigma_data), x.ndim) * jte


def _steer(model, extra_args):
    """(model, extra_args, steer) of a sampler call: ``extra_args['steer']`` (an ActionSteer) read once, in front of every other
    key.  No steer, or one whose weight is all zero: the key is dropped and the call is the call without it.  An active steer
    with a pin or a guidance weight raises NotImplementedError.  With this package's GCDenoiser the key stays: the host loops
    hand it to ``forward``, and ``_steer_native`` decides whether the call is the native one instead.  Any other model is
    wrapped (``_SteeredModel``) and the key comes off."""
    if not extra_args or "steer" not in extra_args:
        return model, extra_args, None
    steer, rest = take_steer(extra_args)
    if steer is None:
        return model, rest, None
    steer_alone(cond_lambda=rest.get("cond_lambda"), pin=rest.get("pin"))
    if isinstance(model, GCDenoiser):
        return model, extra_args, steer
    return _SteeredModel(model, steer), rest, steer


def _steer_native(model, sigmas, scaler, callback, extra_args, host_schedule=False) -> bool:
    """Whether a steered sampler call is the native one (mdt_sample_ddim_steer for sample_ddim and churn-free sample_euler,
    mdt_sample_steer for every other kind): ``_native_ok`` says yes to the call without the steer, and the only other key is
    ``candidates``.  ``host_schedule``: the call takes a host schedule only (mdt_sample_steer; a device schedule keeps the host
    loop).  Steered calls are never graphed."""
    rest = take_steer(extra_args)[1]
    if host_schedule and torch.is_tensor(sigmas) and sigmas.device.type == "cuda":
        return False
    return set(rest) <= {"candidates"} and _native_ok(model, sigmas, scaler, callback, rest)


def _plan_native(steer) -> bool:
    """Whether a steer asks for the native call of the plan samplers (``ActionSteer(..., plan_native=True)``).  Without it a
    steered call of those samplers is the host loop it has always been: the native route is there for the asking."""
    return bool(getattr(steer, "plan_native", False))


def _admits(model, sigmas, scaler, callback, extra_args, steer) -> bool:
    """Whether a plan sampler's call is a native one: ``_native_ok`` without a steer; with one, the steer asks for it
    (``_plan_native``) and ``_steer_native`` says yes on a host schedule."""
    if steer is None:
        return _native_ok(model, sigmas, scaler, callback, extra_args)
    return _plan_native(steer) and _steer_native(model, sigmas, scaler, callback, extra_args, host_schedule=True)


def _run_steer(model, state, action, goal, sigmas, steer, extra_args, scaler=None, kind=None, noise=None, n_steps=None, **params):
    """The steered native call: DDIM's (``kind`` None) or the plan sampler ``kind``'s with its noise rows and parameters."""
    K = take_candidates(take_steer(extra_args)[1])[0]
    rows, noise = _chunk_view(state, action, noise, K)
    kw = {} if kind is None else dict(params, kind=kind, noise=noise, n_steps=n_steps)
    return model.sample_steered(state, rows, goal, sigmas, steer, candidates=K, bounds=scaler, **kw).reshape(action.shape)


def _native(kind, model, state, action, goal, sigmas, noise, steer=None, n_steps=None, extra_args=None, tree=None, scaler=None,
            **params):
    """The native call of a plan sampler that ``_admits`` admitted: ``_run_native`` (graphs included), or under a steer the eager
    steered call with the same noise rows and parameters."""
    if steer is None:
        return _run_native(kind, model, state, action, goal, sigmas, noise, n_steps=n_steps, extra_args=extra_args, tree=tree,
                           scaler=scaler, **params)
    return _run_steer(model, state, action, goal, sigmas, steer, extra_args, scaler=scaler, kind=kind, noise=noise,
                      n_steps=n_steps, **params)


def _chunk_view(state, action, noise, K):
    """A candidates call's ``action`` as its (B*K, Ta, A) chunks (chunk_rows checks the leading size) and its noise rows to match."""
    if K == 1 and action.dim() != 4:
        return action, noise
    B = next(v for v in state.values() if torch.is_tensor(v)).shape[0]
    rows = chunk_rows(action, B, K)
    if noise is not None and noise.dim() == action.dim() + 1:
        noise = noise.reshape((noise.shape[0],) + tuple(rows.shape))
    return rows, noise


def _native_ok(model, sigmas, scaler, callback, extra_args) -> bool:
    if not isinstance(model, GCDenoiser) or callback is not None or not _controls(extra_args)[0]:
        return False
    if not _scaler_native(scaler):
        return False
    n = len(sigmas) - 1
    if n < 1 or n > _lib.SAMPLER_MAX_STEPS:
        return False
    if torch.is_tensor(sigmas) and sigmas.device.type == "cuda":
        return True
    sig = _host(sigmas)
    return bool((sig[:-1] > 0).all()) and float(sig[-1]) == 0.0


def _randn_rows(action, n):
    """n draws of torch.randn_like(action), in order, as one (n, *action.shape) tensor (None for n = 0)."""
    return torch.stack([torch.randn_like(action) for _ in range(n)]) if n else None


def _sampled_rows(action, values):
    """noise_sampler values (any device, broadcastable to action) as one (n, *action.shape) tensor."""
    if not values:
        return None
    return torch.stack([torch.broadcast_to(v.to(device=action.device, dtype=action.dtype), action.shape) for v in values])


def _ancestral_draws(sigmas, eta):
    """randn draws of euler_ancestral / dpm_2_ancestral: one per step with sigma_down > 0 -- the loop's own test on a host schedule,
    every step but the last on a device schedule (the schedule assumption; no read-back)."""
    n = len(sigmas) - 1
    if torch.is_tensor(sigmas) and sigmas.device.type == "cuda":
        return n - 1
    sig = _host(sigmas)
    return sum(1 for i in range(n) if get_ancestral_step(sig[i], sig[i + 1], eta=eta)[0] > 0)


def _run_native(kind, model, state, action, goal, sigmas, noise, n_steps=None, extra_args=None, tree=None, scaler=None,
                **params):
    """The native call, replayed as a HIP graph by sample_ddim's rule (rollout-sized batches from the third identical call).
    ``n_steps``: dpm_fast's evaluation count (its schedule is the two levels, which join the graph key with it).  ``extra_args``:
    the sampler's, which _native_ok admitted -- a guidance weight joins the parameters (and with them the graph key).  ``tree``
    (dpmpp_sde, in place of ``noise``): (seeds, tol, lo, hi) of the Brownian tree the call draws from; (tol, lo, hi) join the
    graph key and the seeds are the graph's per-call input.  ``scaler``: None or the sampler's, which _native_ok admitted -- its
    bounds ride in the call; a graph holds them in static buffers refreshed before every replay, so only their presence joins the
    graph key.  A pin among the ``extra_args`` (an ActionPin) rides in the call the same way; ``candidates`` joins the parameters
    as the weight does, and the "rollout-sized" rule then counts chunks."""
    bounds = None if scaler is None else scaler.clip_bounds(action.device)
    _, lam, pin, K = _controls(extra_args)
    shape = action.shape
    action, noise_rows = _chunk_view(state, action, None if tree is not None else noise, K)
    if tree is None:
        noise = noise_rows
    if pin is not None:
        pin = pin.on(action.device, action.shape, K)
    if lam is not None:
        params = dict(params, cond_lambda=lam)
    if K != 1:
        params = dict(params, candidates=K)
    tag = (kind, tuple(sorted(params.items())))
    if n_steps is not None:
        tag += (n_steps, tuple(float(v) for v in sigmas))
    key = (kind, params, n_steps)
    meta = None
    if tree is not None:
        noise, meta = tree[0], tuple(float(v) for v in tree[1:])
        tag += (("tree",) + meta,)
        key += (("tree",) + meta,)
    if bounds is not None:
        tag += ("bounds",)
        key += ("bounds",)
    if pin is not None:
        tag += ("pin",)
        key += ("pin",)
    out = _graph_route(model, "_graphed_native", tag, key, state, action, goal, sigmas,
                       lambda sig: GraphedSampler(model, kind, params, state, action, goal, sig, noise, n_steps, tree=meta,
                                                  bounds=bounds, pin=pin),
                       f"sample_{kind}", noise=noise, bounds=bounds, pin=pin)
    if out is not None:
        return out.reshape(shape)
    kw = {} if bounds is None else {"bounds": bounds}
    if pin is not None:
        kw["pin"] = pin
    if tree is not None:
        return model.sample_native(kind, state, action, goal, sigmas, tree=tree, **kw, **params).reshape(shape)
    return model.sample_native(kind, state, action, goal, sigmas, noise=noise, n_steps=n_steps, **kw, **params).reshape(shape)


def replay_callback(rec, callback):
    """Feed the record of ``GCDenoiser.sample_native(..., record=True)`` to a sampler ``callback``: one call per step with the dict
    the loops pass -- {'x', 'i', 'sigma', 'sigma_hat', 'denoised'} -- for a hook that wants the trajectory of the native call.
    (A ``callback`` passed to ``sample_*`` itself keeps the host loop, which calls it between the steps.)"""
    for i in range(rec["x"].shape[0]):
        callback({'x': rec["x"][i], 'i': i, 'sigma': rec["sigma"][i], 'sigma_hat': rec["sigma_hat"][i],
                  'denoised': rec["denoised"][i]})


@torch.no_grad()
def sample_ddim(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                eta=1.):
    """DPM-Solver-1 / DDIM (reference gc_sampling.py:922-951):
    x <- (sigma_{i+1}/sigma_i) x - expm1(-(t_{i+1} - t_i)) D(x; sigma_i),  t = -ln sigma.
    `scaler` is accepted and never read, exactly as in the reference (its DDIM has no `clip_output` call), so a harness run
    with `use_scaler` (mdtv_agent.py:606-614) keeps the fused native loop; only `callback` / `extra_args` need the step loop
    (a guidance weight, pinned actions and a candidate count, ``extra_args={"cond_lambda": lam, "pin": ActionPin(...),
    "candidates": K}``, ride in the native call: K chunks per observation of ``state`` / ``goal`` from one encoded context,
    ``action`` (B*K, Ta, A) or (B, K, Ta, A)).  ``extra_args={"steer": ActionSteer(...)}`` (utils/action_steer.py) steers every
    step's denoised value through the denoiser's Jacobian; alone or with ``candidates`` it is one native call of its own
    (mdt_sample_ddim_steer), eager, never a graph."""
    model, extra_args, steer = _steer(model, extra_args)
    extra_args = {} if extra_args is None else extra_args
    if steer is not None and _steer_native(model, sigmas, None, callback, extra_args):
        return _run_steer(model, state, action, goal, sigmas, steer, extra_args)  # one native call, eager (never a graph)
    native, lam, pin, K = _controls(extra_args)
    if isinstance(model, GCDenoiser) and callback is None and native:
        # guidance: the guided native call, its graphs keyed by the weight too; a pin: by its presence (the values are copied in)
        tag, kw = (None, {}) if lam is None else (("ddim_guided", lam), {"cond_lambda": lam})
        key = lam
        shape = action.shape
        action = _chunk_view(state, action, None, K)[0]
        if pin is not None:
            pin = pin.on(action.device, action.shape, K)
            tag, key, kw = ("ddim_pin", lam), (lam, "pin"), dict(kw, pin=pin)
        if K != 1:  # the candidate count: part of the graph key (GraphedDDIM._call_key)
            tag, key, kw = (tag, ("candidates", K)), (key, ("candidates", K)), dict(kw, candidates=K)
        out = _graph_route(model, "_graphed_samplers", tag, key, state, action, goal, sigmas,
                           lambda sig: GraphedDDIM(model, state, action, goal, sig, cond_lambda=lam, pin=pin, candidates=K),
                           "sample_ddim" if lam is None else "guided sample_ddim", pin=pin)
        if out is not None:
            return out.reshape(shape)
        return model.sample_ddim(state, action, goal, sigmas, **kw).reshape(shape)  # fused native loop
    sig = _host(sigmas)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            if callback is not None:
                callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            t, t_next = _t(sig[i]), _t(sig[i + 1])
            h = t_next - t
            action = _f(_sigma(t_next) / _sigma(t)) * action - _f((-h).expm1()) * denoised
    return action


@torch.no_grad()
def sample_euler(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                 s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """Karras Algorithm 2 without the 2nd-order correction (reference gc_sampling.py:164-209).  Steered
    (``extra_args={"steer": ActionSteer}``) and without churn it is sample_ddim's update and runs as that native call, the scaler's
    bounds inside."""
    model, extra_args, steer = _steer(model, extra_args)
    if steer is not None and s_churn == 0 and _steer_native(model, sigmas, scaler, callback, extra_args):
        _randn_rows(action, len(sigmas) - 1)  # the loop's draws: a seeded call leaves the generator where the loop leaves it
        return _run_steer(model, state, action, goal, sigmas, steer, extra_args, scaler=scaler)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        return _native("euler", model, state, action, goal, sigmas, _randn_rows(action, len(sigmas) - 1), steer=steer,
                       s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise, extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    n = len(sig) - 1
    with _hoist(model, state, goal):
        for i in range(n):
            gamma = min(s_churn / n, 2 ** 0.5 - 1) if s_tmin <= sig[i] <= s_tmax else 0.
            eps = torch.randn_like(action) * s_noise  # drawn every step, like the reference (same generator stream)
            sigma_hat = sig[i] * (gamma + 1)
            if gamma > 0:
                action = action + eps * _f((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
            denoised = model(state, action, goal, _sig_in(sigma_hat, action, model), **extra_args)
            d = to_d(action, sigma_hat, denoised)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
            action = action + d * _f(sig[i + 1] - sigma_hat)
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_euler_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                           disable=None, eta=1.):
    """Euler steps to sigma_down plus fresh noise sigma_up (reference gc_sampling.py:213-252)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        noise = _randn_rows(action, _ancestral_draws(sigmas, eta))
        return _native("euler_ancestral", model, state, action, goal, sigmas, noise, steer=steer, eta=eta, extra_args=extra_args,
                       scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            d = to_d(action, sig[i], denoised)
            action = action + d * _f(sigma_down - sig[i])
            if sigma_down > 0:
                action = action + torch.randn_like(action) * _f(sigma_up)
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_heun(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """Karras Algorithm 2 with Heun's trapezoidal correction; plain Euler on the final step to sigma = 0
    (reference gc_sampling.py:256-312)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        return _native("heun", model, state, action, goal, sigmas, _randn_rows(action, len(sigmas) - 1), steer=steer,
                       s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise, extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    n = len(sig) - 1
    with _hoist(model, state, goal):
        for i in range(n):
            gamma = min(s_churn / n, 2 ** 0.5 - 1) if s_tmin <= sig[i] <= s_tmax else 0.
            eps = torch.randn_like(action) * s_noise  # drawn every step, like the reference (same generator stream)
            sigma_hat = sig[i] * (gamma + 1)
            if gamma > 0:
                action = action + eps * _f((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
            denoised = model(state, action, goal, _sig_in(sigma_hat, action, model), **extra_args)
            d = to_d(action, sigma_hat, denoised)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
            dt = _f(sig[i + 1] - sigma_hat)
            if sig[i + 1] == 0:
                action = action + d * dt
            else:
                action_2 = action + d * dt
                denoised_2 = model(state, action_2, goal, _sig_in(sig[i + 1], action, model), **extra_args)
                d_2 = to_d(action_2, sig[i + 1], denoised_2)
                action = action + (d + d_2) / 2 * dt
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_dpmpp_2m(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None):
    """DPM-Solver++(2M) multistep (reference gc_sampling.py:699-734)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        # (the loop below never reads `scaler`, as in the reference: no bounds to pass)
        return _native("dpmpp_2m", model, state, action, goal, sigmas, None, steer=steer, extra_args=extra_args)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    old_denoised = None
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            if callback is not None:
                callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            t, t_next = _t(sig[i]), _t(sig[i + 1])
            h = t_next - t
            if old_denoised is None or sig[i + 1] == 0:
                denoised_d = denoised
            else:
                r = (t - _t(sig[i - 1])) / h
                denoised_d = _f(1 + 1 / (2 * r)) * denoised - _f(1 / (2 * r)) * old_denoised
            action = _f(_sigma(t_next) / _sigma(t)) * action - _f((-h).expm1()) * denoised_d
            old_denoised = denoised
    return action


@torch.no_grad()
def sample_dpmpp_2s(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                    eta=1.):
    """DPM-Solver++(2S) single-step second order (reference gc_sampling.py:955-994)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        return _native("dpmpp_2s", model, state, action, goal, sigmas, None, steer=steer, extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            if callback is not None:
                callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            if sig[i + 1] == 0:
                action = action + to_d(action, sig[i], denoised) * _f(sig[i + 1] - sig[i])
            else:
                t, t_next = _t(sig[i]), _t(sig[i + 1])
                h = t_next - t
                s = t + 0.5 * h
                x_2 = _f(_sigma(s) / _sigma(t)) * action - _f((-h * 0.5).expm1()) * denoised
                denoised_2 = model(state, x_2, goal, _sig_in(_sigma(s), action, model), **extra_args)
                action = _f(_sigma(t_next) / _sigma(t)) * action - _f((-h).expm1()) * denoised_2
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_dpm_2(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None,
                 s_churn=0., s_tmin=0., s_tmax=float('inf'), s_noise=1.):
    """DPM-Solver-2 flavoured midpoint steps (reference gc_sampling.py:315-371): derivative at sigma_hat, a second
    evaluation at the log-midpoint sigma, full step with the midpoint derivative; Euler on the last step."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        return _native("dpm_2", model, state, action, goal, sigmas, _randn_rows(action, len(sigmas) - 1), steer=steer,
                       s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise, extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    n = len(sig) - 1
    with _hoist(model, state, goal):
        for i in range(n):
            gamma = min(s_churn / n, 2 ** 0.5 - 1) if s_tmin <= sig[i] <= s_tmax else 0.
            eps = torch.randn_like(action) * s_noise  # drawn every step, like the reference (same generator stream)
            sigma_hat = sig[i] * (gamma + 1)
            if gamma > 0:
                action = action + eps * _f((sigma_hat ** 2 - sig[i] ** 2) ** 0.5)
            denoised = model(state, action, goal, _sig_in(sigma_hat, action, model), **extra_args)
            d = to_d(action, sigma_hat, denoised)
            if callback is not None:
                callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
            if sig[i + 1] == 0:
                action = action + d * _f(sig[i + 1] - sigma_hat)
            else:
                sigma_mid = sigma_hat.log().lerp(sig[i + 1].log(), 0.5).exp()
                action_2 = action + d * _f(sigma_mid - sigma_hat)
                denoised_2 = model(state, action_2, goal, _sig_in(sigma_mid, action, model), **extra_args)
                d_2 = to_d(action_2, sigma_mid, denoised_2)
                action = action + d_2 * _f(sig[i + 1] - sigma_hat)
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_dpm_2_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                           disable=None, eta=1.):
    """Ancestral sampling with DPM-Solver-2 midpoint steps (reference gc_sampling.py:374-407)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        noise = _randn_rows(action, _ancestral_draws(sigmas, eta))
        return _native("dpm_2_ancestral", model, state, action, goal, sigmas, noise, steer=steer, eta=eta, extra_args=extra_args,
                       scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            d = to_d(action, sig[i], denoised)
            if sigma_down == 0:
                action = action + d * _f(sigma_down - sig[i])
            else:
                sigma_mid = sig[i].log().lerp(sigma_down.log(), 0.5).exp()
                action_2 = action + d * _f(sigma_mid - sig[i])
                denoised_2 = model(state, action_2, goal, _sig_in(sigma_mid, action, model), **extra_args)
                d_2 = to_d(action_2, sigma_mid, denoised_2)
                action = action + d_2 * _f(sigma_down - sig[i])
                action = action + torch.randn_like(action) * _f(sigma_up)
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


def linear_multistep_coeff(order, t, i, j):
    """Integral over [t_i, t_{i+1}] of the j-th Lagrange basis polynomial through the last `order` nodes
    (reference gc_sampling.py:410-422; scipy quadrature, epsrel 1e-4)."""
    from scipy import integrate
    if order - 1 > i:
        raise ValueError(f'Order {order} too high for step {i}')

    def basis(tau):
        prod = 1.
        for k in range(order):
            if k != j:
                prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
        return prod
    return integrate.quad(basis, t[i], t[i + 1], epsrel=1e-4)[0]


@torch.no_grad()
def sample_lms(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None, disable=None, order=4):
    """Linear multistep (Adams-Bashforth in sigma) sampler (reference gc_sampling.py:425-460)."""
    model, extra_args, steer = _steer(model, extra_args)
    if 1 <= order <= 4 and _admits(model, sigmas, scaler, callback, extra_args, steer):
        return _native("lms", model, state, action, goal, sigmas, None, steer=steer, order=order, extra_args=extra_args,
                       scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    sig_np = sig.numpy()
    ds = []
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            ds.append(to_d(action, sig[i], denoised))
            if len(ds) > order:
                ds.pop(0)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            cur_order = min(i + 1, order)
            coeffs = [linear_multistep_coeff(cur_order, sig_np, i, j) for j in range(cur_order)]
            action = action + sum(coeff * d for coeff, d in zip(coeffs, reversed(ds)))
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


@torch.no_grad()
def sample_dpmpp_2_with_lms(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                            disable=None):
    """The reference's second name for DPM-Solver++(2M) (gc_sampling.py:785-816 is line-for-line its :699-734)."""
    return sample_dpmpp_2m(model, state, action, goal, sigmas, scaler=scaler, extra_args=extra_args,
                           callback=callback, disable=disable)


@torch.no_grad()
def sample_dpmpp_2s_ancestral(model, state, action, goal, sigmas, scaler=None, extra_args=None, callback=None,
                              disable=None, eta=1., s_noise=1., noise_sampler=None):
    """Ancestral sampling with DPM-Solver++(2S) steps (reference gc_sampling.py:864-907)."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        n = len(sigmas) - 1
        if noise_sampler is None:
            noise = _randn_rows(action, n)  # default_noise_sampler: randn_like(action) per step
        else:
            sig = _host(sigmas)
            noise = _sampled_rows(action, [noise_sampler(sig[i], sig[i + 1]) for i in range(n)])
        return _native("dpmpp_2s_ancestral", model, state, action, goal, sigmas, noise, steer=steer, eta=eta, s_noise=s_noise,
                       extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
    sig = _host(sigmas)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            sigma_down, sigma_up = get_ancestral_step(sig[i], sig[i + 1], eta=eta)
            if callback is not None:
                callback({'action': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            if sigma_down == 0:
                action = action + to_d(action, sig[i], denoised) * _f(sigma_down - sig[i])
            else:
                t, t_next = _t(sig[i]), _t(sigma_down)
                h = t_next - t
                s = t + 0.5 * h
                x_2 = _f(_sigma(s) / _sigma(t)) * action - _f((-h * 0.5).expm1()) * denoised
                denoised_2 = model(state, x_2, goal, _sig_in(_sigma(s), action, model), **extra_args)
                action = _f(_sigma(t_next) / _sigma(t)) * action - _f((-h).expm1()) * denoised_2
            action = action + noise_sampler(sig[i], sig[i + 1]) * s_noise * _f(sigma_up)
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


# ------------------------------------------------------------------------------------------------
# DPM-Solver (fixed-step "fast" and adaptive) and DPM-Solver++ SDE      (reference gc_sampling.py:495-690,737-790,834-870)
# ------------------------------------------------------------------------------------------------
def _identity(x):
    return x


def _torchsde_available() -> bool:
    import importlib.util
    return importlib.util.find_spec("torchsde") is not None


class NativeBrownianTreeNoiseSampler:
    """The noise sampler of ``BrownianTreeNoiseSampler`` without torchsde: the library's virtual Brownian tree (include/mdt_hip.h
    mdt_brownian_noise; the definition is in csrc/mdt_brownian.h), on the GPU for a GPU ``x`` and on the host for a CPU one.  The
    reference's constructor and call: ``seed`` None draws one ``torch.randint(0, 2**63 - 1, [])`` from the default generator, an
    int gives one tree for the whole tensor, a list of B ints one tree per sample (a sample's noise does not then depend on the
    rest of the batch).  A call returns (W(to) - W(from)) / sqrt(|to - from|) of the transformed points, shaped like ``x``.  The
    law is torchsde's; the values are not (another construction).  sample_dpmpp_sde runs such a sampler with the identity
    ``transform`` inside its native call."""

    def __init__(self, x, sigma_min, sigma_max, seed=None, transform=_identity, tol=1e-6):
        self.transform = transform
        t0, t1 = self._point(sigma_min), self._point(sigma_max)
        self.sign = 1 if t0 < t1 else -1
        self.lo, self.hi = (t0, t1) if t0 < t1 else (t1, t0)
        seeds = [torch.randint(0, 2 ** 63 - 1, []).item()] if seed is None else ([seed] if isinstance(seed, int) else list(seed))
        self.batched = not (seed is None or isinstance(seed, int))
        self.seeds = [int(s) for s in seeds]
        self.tol = float(tol)
        self.shape, self.dtype, self.device = tuple(x.shape), x.dtype, x.device
        if self.batched and (x.ndim == 0 or len(self.seeds) != x.shape[0]):
            raise ValueError(f"NativeBrownianTreeNoiseSampler: {len(self.seeds)} seeds for a batch of {tuple(x.shape)[:1]}")
        if any(not 0 <= s < 2 ** 64 for s in self.seeds):
            raise ValueError("NativeBrownianTreeNoiseSampler: seeds must be in [0, 2**64)")
        self.batch = len(self.seeds) if self.batched else 1
        self.per_row = max(1, x.numel() // self.batch)
        self._dev_seeds = None
        _lib.brownian_noise_host(self.seeds, self.lo, self.hi, self.tol, [], self.batch, self.per_row)  # the checks, no values

    def _point(self, v):
        return float(self.transform(torch.as_tensor(v)))

    def seeds_on(self, device):
        """The seeds as the int64 device tensor the library reads (bit pattern of the unsigned keys)."""
        if self._dev_seeds is None or self._dev_seeds.device != device:
            vals = [s - 2 ** 64 if s >= 2 ** 63 else s for s in self.seeds]
            self._dev_seeds = torch.tensor(vals, dtype=torch.int64, device=device)
        return self._dev_seeds

    def native_tree(self, device):
        """(seeds, tol, lo, hi) for GCDenoiser.sample_native's ``tree``, or None where the call cannot walk this sampler's trees
        (a transform other than the identity, a reversed interval, another device)."""
        if self.transform is not _identity or self.sign != 1 or torch.device(device) != self.device:
            return None
        return self.seeds_on(self.device), self.tol, self.lo, self.hi

    def __call__(self, sigma, sigma_next):
        pair = [self._point(sigma), self._point(sigma_next)]
        if self.device.type == "cuda":
            lib = _lib.load()
            out = torch.empty((1, self.batch, self.per_row), device=self.device, dtype=torch.float32)
            pr = (ctypes.c_double * 2)(*pair)
            _lib.check(lib.mdt_brownian_noise(self.seeds_on(self.device).data_ptr(), len(self.seeds), self.lo, self.hi, self.tol,
                                              pr, 1, self.batch, self.per_row, out.data_ptr(),
                                              torch.cuda.current_stream(self.device).cuda_stream))
        else:
            out = torch.from_numpy(_lib.brownian_noise_host(self.seeds, self.lo, self.hi, self.tol, [pair], self.batch,
                                                            self.per_row))
        out = out.view(self.shape)
        return (out if self.sign == 1 else -out).to(self.dtype)


class BrownianTreeNoiseSampler:
    """Noise sampler backed by torchsde.BrownianTree (reference gc_sampling.py:112-160), the default of
    ``sample_dpmpp_sde``.  torchsde is an optional dependency, as in the reference; without it the constructor returns a
    ``NativeBrownianTreeNoiseSampler`` (the same law from the library's own tree)."""

    def __new__(cls, x, sigma_min, sigma_max, seed=None, transform=_identity):
        if not _torchsde_available():
            return NativeBrownianTreeNoiseSampler(x, sigma_min, sigma_max, seed=seed, transform=transform)
        return super().__new__(cls)

    def __init__(self, x, sigma_min, sigma_max, seed=None, transform=_identity):
        import torchsde
        self.transform = transform
        t0, t1 = self.transform(torch.as_tensor(sigma_min)), self.transform(torch.as_tensor(sigma_max))
        self.sign = 1 if t0 < t1 else -1
        lo, hi = (t0, t1) if t0 < t1 else (t1, t0)
        seeds = [torch.randint(0, 2 ** 63 - 1, []).item()] if seed is None else ([seed] if isinstance(seed, int) else list(seed))
        self.batched = not (seed is None or isinstance(seed, int))
        w0 = torch.zeros_like(x[0] if self.batched else x)
        self.trees = [torchsde.BrownianTree(lo, w0, hi, entropy=sd) for sd in seeds]

    def __call__(self, sigma, sigma_next):
        t0, t1 = self.transform(torch.as_tensor(sigma)), self.transform(torch.as_tensor(sigma_next))
        sign = 1 if t0 < t1 else -1
        lo, hi = (t0, t1) if t0 < t1 else (t1, t0)
        w = torch.stack([tree(lo, hi) for tree in self.trees]) * (self.sign * sign)
        return (w if self.batched else w[0]) / (t1 - t0).abs().sqrt()


# ------------------------------------------------------------------------------------------------
# DPM-Solver (arXiv:2206.00927) behind sample_dpm_fast / sample_dpm_adaptive (reference gc_sampling.py:495-697,
# 834-870).  One exponential-integrator routine covers the three orders: with lambda = t = -ln(sigma), h the step and
# r_1 < r_2 the interior nodes of the order,
#     x(t+h) = x - sigma(t+h) * [ expm1(h) * eps_0  +  c_k * (eps_k - eps_0) ]
# where eps_k is the noise prediction at node k (evaluated on the lower-order estimate at that node), and
#     order 1: no correction;   order 2: c_1 = expm1(h) / (2 r_1);   order 3: c_2 = (expm1(h)/h - 1) / r_2.
# ------------------------------------------------------------------------------------------------
_DPM_NODES = {1: (), 2: (1 / 2,), 3: (1 / 3, 2 / 3)}


class _EpsEvaluator:
    """eps(x, t) = (x - D(x; sigma(t))) / sigma(t) of a denoiser, counting its evaluations."""

    def __init__(self, model, state, goal, extra_args, on_eval=None):
        self.model, self.state, self.goal, self.kw = model, state, goal, (extra_args or {})
        self.evals, self.on_eval = 0, on_eval

    def __call__(self, x, t):
        sig = _sigma(t)
        self.evals += 1
        if self.on_eval is not None:
            self.on_eval()
        return (x - self.model(self.state, x, self.goal, _sig_in(sig, x, self.model), **self.kw)) / _f(sig)


def _dpm_stages(eps, x, t, t_next, nodes, eps0):
    """Noise predictions at the left end and at the interior `nodes` of [t, t_next] (each on the estimate the lower
    stages give there): the list [eps_0, eps_1, ...]."""
    h = t_next - t
    out = [eps0]
    for k, r in enumerate(nodes):
        s = t + r * h
        u = x - _f(_sigma(s) * (r * h).expm1()) * eps0
        if k == 1:  # second interior node: first-node correction scaled to this node
            r1 = nodes[0]
            u = u - _f(_sigma(s) * (r / r1) * ((r * h).expm1() / (r * h) - 1)) * (out[1] - eps0)
        out.append(eps(u, s))
    return out


def _dpm_combine(x, t, t_next, nodes, stages):
    """The order-(len(nodes)+1) update from the stage values of _dpm_stages."""
    h = t_next - t
    sn = _sigma(t_next)
    new = x - _f(sn * h.expm1()) * stages[0]
    if len(nodes) == 1:
        new = new - _f(sn / (2 * nodes[0]) * h.expm1()) * (stages[1] - stages[0])
    elif len(nodes) == 2:
        new = new - _f(sn / nodes[1] * (h.expm1() / h - 1)) * (stages[2] - stages[0])
    return new


def _ancestral_split(t, t_next, t_end, eta):
    """Deterministic end point and the noise level re-injected after it (eta > 0), in t = -ln(sigma)."""
    if not eta:
        return t_next, 0.
    sd, _ = get_ancestral_step(_sigma(t), _sigma(t_next), eta)
    t_det = torch.minimum(torch.as_tensor(t_end), _t(sd))
    return t_det, (_sigma(t_next) ** 2 - _sigma(t_det) ** 2) ** 0.5


class _StepControl:
    """Proportional-integral-derivative step-size control on the inverse error history (Soederlind's digital-filter
    form, as torchdiffeq / k-diffusion use it), evaluated in the log domain, with the arctan limiter."""

    def __init__(self, h, kp, ki, kd, order, safety, eps=1e-8):
        self.h = h
        self.weights = ((kp + ki + kd) / order, -(kp + 2 * kd) / order, kd / order)
        self.safety, self.eps = safety, eps
        self.history = None  # log inverse errors: [current, previous, the one before]

    def update(self, error):
        """Feed the scaled error of the step just tried; returns whether it is accepted and rescales ``h``."""
        cur = -math.log(float(error) + self.eps)
        self.history = [cur, cur, cur] if self.history is None else [cur] + self.history[1:]
        factor = math.exp(sum(w * e for w, e in zip(self.weights, self.history)))
        factor = 1 + math.atan(factor - 1)
        ok = factor >= self.safety
        if ok:
            self.history = [cur, cur, self.history[1]]  # shift: the accepted error becomes "previous"
        self.h *= factor
        return ok


def _check_sigma_range(sigma_min, sigma_max):
    if sigma_min <= 0 or sigma_max <= 0:
        raise ValueError('sigma_min and sigma_max must not be 0')


@torch.no_grad()
def sample_dpm_fast(model, state, action, goal, sigma_min, sigma_max, n, scaler=None, extra_args=None, callback=None,
                    disable=None, eta=0., s_noise=1., noise_sampler=None):
    """DPM-Solver-Fast, fixed step size, n model evaluations (reference gc_sampling.py:673-697 / 592-624): m =
    floor(n/3)+1 uniform steps in t, third order except for the tail (.., 2, 1 when 3 | n, else .., n mod 3).
    (The reference builds its default noise sampler from an undefined name, :600, so it only runs with an explicit one;
    the default here is the action-shaped Gaussian sampler it meant.)"""
    model, extra_args, steer = _steer(model, extra_args)
    _check_sigma_range(sigma_min, sigma_max)
    t_start, t_end = _t(torch.tensor(float(sigma_max))), _t(torch.tensor(float(sigma_min)))
    if eta and not t_end > t_start:
        raise ValueError('eta must be 0 for reverse sampling')
    noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
    rest = extra_args if steer is None else take_steer(extra_args)[1]  # a steer rides alone or with ``candidates``
    if (isinstance(model, GCDenoiser) and callback is None and _controls(rest)[0] and _scaler_native(scaler)
            and (steer is None or (_plan_native(steer) and set(rest) <= {"candidates"}))
            and 1 <= n <= _lib.SAMPLER_MAX_EVALS):  # (the solver never reads `scaler`, here as in the reference: no bounds to pass)
        return _native("dpm_fast", model, state, action, goal, [float(sigma_max), float(sigma_min)],
                       _dpm_fast_noise(action, t_start, t_end, n, eta, noise_sampler), steer=steer, n_steps=n, eta=eta,
                       s_noise=s_noise, extra_args=extra_args)
    with _hoist(model, state, goal):
        return _dpm_fast_run(_EpsEvaluator(model, state, goal, extra_args), action, t_start, t_end, n, eta, s_noise,
                             noise_sampler, callback)


def _dpm_fast_noise(action, t_start, t_end, n, eta, noise_sampler):
    """The noise_sampler values _dpm_fast_run draws, in its order: one per step with s_up != 0 (none at eta = 0), padded with
    zero rows to one per step -- the rows a device schedule may read (rows beyond the plan's are unread)."""
    if not eta:
        return None
    m = n // 3 + 1
    grid = torch.linspace(_f(t_start), _f(t_end), m + 1)
    values = []
    for i in range(m):
        t, t_next = grid[i], grid[i + 1]
        if _f(_ancestral_split(t, t_next, t_end, eta)[1]) != 0:
            values.append(noise_sampler(_sigma(t), _sigma(t_next)))
    values += [torch.zeros_like(action)] * (m - len(values))
    return _sampled_rows(action, values)


def _dpm_fast_run(eps, action, t_start, t_end, n, eta, s_noise, noise_sampler, callback):
    m = n // 3 + 1
    grid = torch.linspace(_f(t_start), _f(t_end), m + 1)
    orders = [3] * (m - 2) + [2, 1] if n % 3 == 0 else [3] * (m - 1) + [n % 3]
    for i, order in enumerate(orders):
        t, t_next = grid[i], grid[i + 1]
        t_det, s_up = _ancestral_split(t, t_next, t_end, eta)
        e0 = eps(action, t)
        if callback is not None:
            callback({'x': action, 'i': i, 't': t, 't_up': t, 'denoised': action - _f(_sigma(t)) * e0,
                      'sigma': _sigma(t), 'sigma_hat': _sigma(t)})
        nodes = _DPM_NODES[order]
        action = _dpm_combine(action, t, t_det, nodes, _dpm_stages(eps, action, t, t_det, nodes, e0))
        if _f(s_up) != 0:
            action = action + _f(s_up) * s_noise * noise_sampler(_sigma(t), _sigma(t_next))
    return action


@torch.no_grad()
def sample_dpm_adaptive(model, state, action, goal, sigma_min, sigma_max, extra_args=None, callback=None, disable=None,
                        order=3, rtol=0.05, atol=0.0078, h_init=0.05, pcoeff=0., icoeff=1., dcoeff=0., accept_safety=0.81,
                        eta=0., s_noise=1., return_info=False, noise_sampler=None):
    """DPM-Solver-12 / -23 with adaptive step size (reference gc_sampling.py:834-870 / 626-670): the embedded pair
    (order-1, order) shares its stage evaluations -- the order-2 estimate of the 23 pair uses r_1 = 1/3, the first node
    of the order-3 step -- and the scaled difference of the two drives the step-size control.
    (The reference reads `noise_sampler` before assigning it, :633: its adaptive solver cannot run.  Parity unpinned.)"""
    model, extra_args, steer = _steer(model, extra_args)
    _check_sigma_range(sigma_min, sigma_max)
    if order not in (2, 3):
        raise ValueError('order should be 2 or 3')
    t_start = _t(torch.tensor(float(sigma_max))).to(torch.float32)
    t_end = _t(torch.tensor(float(sigma_min))).to(torch.float32)
    if eta and not bool(t_end > t_start):
        raise ValueError('eta must be 0 for reverse sampling')
    native, lam, pin, K = _controls(extra_args)
    # mdt_sample_dpm_adaptive takes no pin and no candidates: the host loop hands both to forward
    native = native and pin is None and K == 1
    if (isinstance(model, GCDenoiser) and callback is None and native and not eta and action.device.type == "cuda"
            and not torch.cuda.is_current_stream_capturing()):
        kw = {} if lam is None else {"cond_lambda": lam}  # guidance: mdt_sample_dpm_adaptive_guided
        action, info = model.sample_dpm_adaptive_native(state, action, goal, float(sigma_min), float(sigma_max), order=order,
                                                        rtol=rtol, atol=atol, h_init=h_init, pcoeff=pcoeff, icoeff=icoeff,
                                                        dcoeff=dcoeff, accept_safety=accept_safety, **kw)
        return (action, info) if return_info else action
    noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
    with _hoist(model, state, goal):
        action, info = _dpm_adaptive_run(_EpsEvaluator(model, state, goal, extra_args), action, t_start, t_end, order, rtol, atol,
                                         h_init, pcoeff, icoeff, dcoeff, accept_safety, eta, s_noise, noise_sampler, callback)
    return (action, info) if return_info else action


def _dpm_adaptive_run(eps, action, t_start, t_end, order, rtol, atol, h_init, pcoeff, icoeff, dcoeff, accept_safety, eta,
                      s_noise, noise_sampler, callback):
    forward = bool(t_end > t_start)
    ctl = _StepControl(abs(h_init) if forward else -abs(h_init), pcoeff, icoeff, dcoeff, 1.5 if eta else order, accept_safety)
    info = {'steps': 0, 'nfe': 0, 'n_accept': 0, 'n_reject': 0}
    nodes_hi = _DPM_NODES[order]
    nodes_lo = nodes_hi[:-1]  # order 2: () ; order 3: (1/3,) -- the same first node, so the pair shares eps_1
    s, prev = t_start, action
    while (s < t_end - 1e-5) if forward else (s > t_end + 1e-5):
        t = torch.minimum(t_end, s + ctl.h) if forward else torch.maximum(t_end, s + ctl.h)
        t_det, s_up = _ancestral_split(s, t, t_end, eta)
        stages = _dpm_stages(eps, action, s, t_det, nodes_hi, eps(action, s))
        low = _dpm_combine(action, s, t_det, nodes_lo, stages)
        high = _dpm_combine(action, s, t_det, nodes_hi, stages)
        denoised = action - _f(_sigma(s)) * stages[0]
        tol = torch.clamp(rtol * torch.maximum(low.abs(), prev.abs()), min=atol)
        error = torch.linalg.norm((low - high) / tol) / action.numel() ** 0.5
        if ctl.update(error):
            prev = low
            action = high if _f(s_up) == 0 else high + _f(s_up) * s_noise * noise_sampler(_sigma(s), _sigma(t))
            s = t
            info['n_accept'] += 1
        else:
            info['n_reject'] += 1
        info['steps'] += 1
        info['nfe'] = eps.evals
        if callback is not None:
            callback({'x': action, 'i': info['steps'] - 1, 't': s, 't_up': s, 'denoised': denoised, 'error': error,
                      'h': ctl.h, 'sigma': _sigma(s), 'sigma_hat': _sigma(s), **info})
    return action, info


class PIDStepSizeController(_StepControl):
    """The reference's controller by its own name and call form (gc_sampling.py:495-521) over _StepControl."""

    def __init__(self, h, pcoeff, icoeff, dcoeff, order=1, accept_safety=0.81, eps=1e-8):
        super().__init__(h, pcoeff, icoeff, dcoeff, order, accept_safety, eps)

    @staticmethod
    def limiter(action):
        return 1 + math.atan(action - 1)

    def propose_step(self, error):
        return self.update(error)


class DPMSolver(torch.nn.Module):
    """The reference's solver object by its own name and method set (gc_sampling.py:524-670), for code that builds
    ``DPMSolver(model, ...)`` directly; the work is done by the routines above.  ``eps_cache`` dictionaries carry the stage
    values under the reference's keys ('eps', 'eps_r1', 'eps_r2') and are honoured the same way (by key, whatever nodes
    produced them)."""
    _KEYS = ('eps', 'eps_r1', 'eps_r2')

    def __init__(self, model, extra_args=None, eps_callback=None, info_callback=None):
        super().__init__()
        self.model = model
        self.extra_args = {} if extra_args is None else extra_args
        self.eps_callback = eps_callback
        self.info_callback = info_callback

    def t(self, sigma):
        return -sigma.log()

    def sigma(self, t):
        return t.neg().exp()

    def _evaluator(self, state, goal):
        return _EpsEvaluator(self.model, state, goal, self.extra_args, self.eps_callback)

    def eps(self, eps_cache, key, state, action, goal, t, *args, **kwargs):
        if key in eps_cache:
            return eps_cache[key], eps_cache
        e = self._evaluator(state, goal)(action, t)
        return e, {key: e, **eps_cache}

    def _step(self, nodes, state, action, goal, t, t_next, eps_cache):
        cache = dict(eps_cache or {})
        ev = self._evaluator(state, goal)
        if 'eps' not in cache:
            cache['eps'] = ev(action, t)
        stage = [1]

        def staged(u, s):  # stage k of _dpm_stages <-> key k of the reference's cache
            key = self._KEYS[stage[0]]
            stage[0] += 1
            if key not in cache:
                cache[key] = ev(u, s)
            return cache[key]
        out = _dpm_combine(action, t, t_next, nodes, _dpm_stages(staged, action, t, t_next, nodes, cache['eps']))
        return out, cache

    def dpm_solver_1_step(self, state, action, goal, t, t_next, eps_cache=None):
        return self._step((), state, action, goal, t, t_next, eps_cache)

    def dpm_solver_2_step(self, state, action, goal, t, t_next, r1=1 / 2, eps_cache=None):
        return self._step((r1,), state, action, goal, t, t_next, eps_cache)

    def dpm_solver_3_step(self, state, action, goal, t, t_next, r1=1 / 3, r2=2 / 3, eps_cache=None):
        return self._step((r1, r2), state, action, goal, t, t_next, eps_cache)

    def dpm_solver_fast(self, state, action, goal, t_start, t_end, nfe, eta=0., s_noise=1., noise_sampler=None):
        t_start, t_end = torch.as_tensor(t_start), torch.as_tensor(t_end)
        if eta and not t_end > t_start:
            raise ValueError('eta must be 0 for reverse sampling')
        noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
        with _hoist(self.model, state, goal):
            return _dpm_fast_run(self._evaluator(state, goal), action, t_start, t_end, nfe, eta, s_noise, noise_sampler,
                                 self.info_callback)

    def dpm_solver_adaptive(self, state, action, goal, t_start, t_end, order=3, rtol=0.05, atol=0.0078, h_init=0.05, pcoeff=0.,
                            icoeff=1., dcoeff=0., accept_safety=0.81, eta=0., s_noise=1., noise_sampler=None):
        if order not in (2, 3):
            raise ValueError('order should be 2 or 3')
        t_start, t_end = torch.as_tensor(t_start, dtype=torch.float32), torch.as_tensor(t_end, dtype=torch.float32)
        if eta and not bool(t_end > t_start):
            raise ValueError('eta must be 0 for reverse sampling')
        noise_sampler = default_noise_sampler(action) if noise_sampler is None else noise_sampler
        with _hoist(self.model, state, goal):
            return _dpm_adaptive_run(self._evaluator(state, goal), action, t_start, t_end, order, rtol, atol, h_init, pcoeff,
                                     icoeff, dcoeff, accept_safety, eta, s_noise, noise_sampler, self.info_callback)


@torch.no_grad()
def sample_dpmpp_sde(model, state, action, goal, sigmas, extra_args=None, callback=None, disable=None, eta=1., s_noise=1.,
                     scaler=None, noise_sampler=None, r=1 / 2):
    """DPM-Solver++ (stochastic) (reference gc_sampling.py:737-790): a midpoint evaluation at s = t + r h, ancestral
    noise at both sub-steps from ``noise_sampler(sigma, sigma_next)`` (default: a torchsde Brownian tree, or without torchsde
    the library's own, NativeBrownianTreeNoiseSampler).  On the native path that tree -- the default without torchsde, or a
    NativeBrownianTreeNoiseSampler with the identity transform on the model's device -- is walked inside the call
    (mdt_sample_sde_tree): no noise on the host and no read-back of a device schedule."""
    model, extra_args, steer = _steer(model, extra_args)
    if _admits(model, sigmas, scaler, callback, extra_args, steer):
        tree = None
        # (the steered call takes noise rows, not a tree: they are read below from the sampler the host loop would construct, at
        # the loop's points)
        if steer is None and noise_sampler is None and not _torchsde_available():  # the default's one seed draw, as its constructor makes it
            seed = torch.randint(0, 2 ** 63 - 1, []).item()
            tree = (torch.tensor([seed], dtype=torch.int64, device=action.device), 1e-6, 0., 0.)
        elif steer is None and isinstance(noise_sampler, NativeBrownianTreeNoiseSampler):
            tree = noise_sampler.native_tree(action.device)
        if tree is not None:
            return _run_native("dpmpp_sde", model, state, action, goal, sigmas, None, eta=eta, s_noise=s_noise, r=r,
                               extra_args=extra_args, tree=tree, scaler=scaler)
        sig = _host(sigmas)  # the noise sampler takes host values (a device schedule is read back for it)
        if noise_sampler is None:
            noise_sampler = BrownianTreeNoiseSampler(action, sig[sig > 0].min(), sig.max())
        values = []
        for i in range(len(sig) - 2):  # the loop's calls, in its order
            t, t_next = _t(sig[i]), _t(sig[i + 1])
            s = t + (t_next - t) * r
            if _f(get_ancestral_step(_sigma(t), _sigma(s), eta)[1]) != 0:
                values.append(noise_sampler(_sigma(t), _sigma(s)))
            if _f(get_ancestral_step(_sigma(t), _sigma(t_next), eta)[1]) != 0:
                values.append(noise_sampler(_sigma(t), _sigma(t_next)))
        return _native("dpmpp_sde", model, state, action, goal, sigmas, _sampled_rows(action, values), steer=steer, eta=eta,
                       s_noise=s_noise, r=r, extra_args=extra_args, scaler=scaler)
    extra_args = {} if extra_args is None else extra_args
    sig = _host(sigmas)
    if noise_sampler is None:
        noise_sampler = BrownianTreeNoiseSampler(action, sig[sig > 0].min(), sig.max())
    fac = 1 / (2 * r)
    with _hoist(model, state, goal):
        for i in range(len(sig) - 1):
            denoised = model(state, action, goal, _sig_in(sig[i], action, model), **extra_args)
            if callback is not None:
                callback({'x': action, 'i': i, 'sigma': sig[i], 'sigma_hat': sig[i], 'denoised': denoised})
            if sig[i + 1] == 0:
                action = action + to_d(action, sig[i], denoised) * _f(sig[i + 1] - sig[i])  # Euler
                continue
            t, t_next = _t(sig[i]), _t(sig[i + 1])
            h = t_next - t
            s = t + h * r
            sd, su = get_ancestral_step(_sigma(t), _sigma(s), eta)
            s_ = _t(sd)
            x_2 = _f(_sigma(s_) / _sigma(t)) * action - _f((t - s_).expm1()) * denoised
            if _f(su) != 0:
                x_2 = x_2 + noise_sampler(_sigma(t), _sigma(s)) * (s_noise * _f(su))
            denoised_2 = model(state, x_2, goal, _sig_in(_sigma(s), action, model), **extra_args)
            sd, su = get_ancestral_step(_sigma(t), _sigma(t_next), eta)
            t_next_ = _t(sd)
            denoised_d = (1 - fac) * denoised + fac * denoised_2
            action = _f(_sigma(t_next_) / _sigma(t)) * action - _f((t - t_next_).expm1()) * denoised_d
            if _f(su) != 0:
                action = action + noise_sampler(_sigma(t), _sigma(t_next)) * (s_noise * _f(su))
            if scaler is not None:
                action = scaler.clip_output(action)
    return action


# ------------------------------------------------------------------------------------------------
# log-likelihood (reference gc_sampling.py:468-490)
# ------------------------------------------------------------------------------------------------
# Dormand-Prince 5(4) tableau: node positions, stage weights (row i feeds stage i+1), the 5th-order solution
# weights (= the last row: first-same-as-last) and the difference to the embedded 4th-order weights.
_DP_C = (0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_A = (
    (),
    (1 / 5,),
    (3 / 40, 9 / 40),
    (44 / 45, -56 / 15, 32 / 9),
    (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
    (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
    (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84),
)
_DP_E = (35 / 384 - 5179 / 57600, 0.0, 500 / 1113 - 7571 / 16695, 125 / 192 - 393 / 640, -2187 / 6784 + 92097 / 339200,
         11 / 84 - 187 / 2100, -1 / 40)


def _scaled_rms(parts, scale_parts):
    """Root mean square of err / scale over ALL entries of a tuple state (one number: the step is shared)."""
    num = sum(float(((p / s) ** 2).sum()) for p, s in zip(parts, scale_parts))
    return math.sqrt(num / sum(p.numel() for p in parts))


def _dopri5(fn, y0, t0, t1, rtol, atol, max_steps=10000, stats=None):
    """Adaptive Dormand-Prince 5(4) integration of y' = fn(t, y) from t0 to t1 for a tuple of tensors ``y0``: embedded
    error estimate in a mixed absolute / relative norm, first-same-as-last stage reuse, step controller
    h <- h * clip(0.9 * err^(-1/5), 0.2, 10), Hairer's starting step; the last step is shortened to end on t1.  The role
    torchdiffeq.odeint(..., method='dopri5') plays in the reference (gc_sampling.py:486) -- that package is not a
    dependency here.  ``stats``: a dict whose 'steps' / 'n_accept' / 'n_reject' count the attempted steps."""
    y = tuple(y0)
    t, direction = float(t0), (1.0 if t1 >= t0 else -1.0)
    k1 = fn(t, y)
    scale = tuple(atol + rtol * p.abs() for p in y)
    d0, d1 = _scaled_rms(y, scale), _scaled_rms(k1, scale)
    h = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    y_probe = tuple(p + direction * h * k for p, k in zip(y, k1))
    d2 = _scaled_rms(tuple(a - b for a, b in zip(fn(t + direction * h, y_probe), k1)), scale) / h
    h = min(100 * h, max(1e-6, 1e-3 * h) if max(d1, d2) <= 1e-15 else (0.01 / max(d1, d2)) ** 0.2)
    for _ in range(max_steps):
        if (t1 - t) * direction <= 0:
            return y
        h = min(h, abs(t1 - t))
        ks = [k1]
        for i in range(1, 7):
            yi = tuple(p + direction * h * sum(a * k[j] for a, k in zip(_DP_A[i], ks) if a != 0.0)
                       for j, p in enumerate(y))
            if i == 6:
                y_new = yi
            ks.append(fn(t + direction * _DP_C[i] * h, yi))
        err = tuple(h * sum(e * k[j] for e, k in zip(_DP_E, ks) if e != 0.0) for j in range(len(y)))
        scale = tuple(atol + rtol * torch.maximum(p.abs(), q.abs()) for p, q in zip(y, y_new))
        ratio = _scaled_rms(err, scale)
        if stats is not None:
            stats['steps'] += 1
            stats['n_accept' if ratio <= 1.0 else 'n_reject'] += 1
        if ratio <= 1.0:  # accept
            t = t1 if h >= abs(t1 - t) else t + direction * h
            y, k1 = y_new, ks[6]
        h *= 10.0 if ratio == 0.0 else min(10.0, max(0.2, 0.9 * ratio ** -0.2))
    raise RuntimeError("_dopri5: step budget exhausted before reaching the end of the interval")


def _probe_signs(action):
    """Rademacher probe of Hutchinson's trace estimator, drawn the way the reference draws it (gc_sampling.py:475)."""
    return torch.randint_like(action, 2) * 2 - 1


def _probes(action, probes):
    """The probe tensors (P, *action.shape) of log_likelihood's ``extra_args['probes']``: an int P >= 1 -- P = 1 is one
    ``_probe_signs(action)`` draw, as without the key; P > 1 draws all P * action.numel() signs in one call, probe-major -- or
    the caller's own tensor of that shape, used as given."""
    if torch.is_tensor(probes):
        if probes.dim() != action.dim() + 1 or probes.shape[0] < 1 or tuple(probes.shape[1:]) != tuple(action.shape):
            raise ValueError(f"probes is {tuple(probes.shape)}: {action.shape[0]} chunks take (P, {', '.join(map(str, action.shape))})")
        return probes.to(device=action.device, dtype=action.dtype)
    if isinstance(probes, bool) or not isinstance(probes, int) or probes < 1:
        raise ValueError(f"probes must be an int >= 1 or a tensor of probes, got {probes!r}")
    if probes == 1:
        return _probe_signs(action)[None]
    return _probe_signs(action.new_empty((probes,) + tuple(action.shape)))


def best_candidates(chunks, scores, K):
    """The step after scoring K candidate chunks per observation: (best (B, Ta, A), index (B,)) by per-observation argmax of
    ``scores`` -- (B*K,) or (B, K), e.g. log_likelihood's -- over ``chunks`` -- (B*K, Ta, A) or (B, K, Ta, A), chunk k of
    observation b at row b*K + k.  Ties go to the lowest index, NaN scores lose; on the tensors' device, no read-back."""
    K = candidate_count(K)
    if scores.numel() % K or chunks.numel() % max(scores.numel(), 1) or chunks.dim() < 3:
        raise ValueError(f"scores {tuple(scores.shape)} and chunks {tuple(chunks.shape)} do not hold K = {K} candidates per observation")
    sc = torch.nan_to_num(scores.reshape(-1, K), nan=float("-inf"))
    B = sc.shape[0]
    if chunks.numel() // (chunks.shape[-2] * chunks.shape[-1]) != B * K:
        raise ValueError(f"chunks {tuple(chunks.shape)} hold no {B} x {K} chunks")
    ks = torch.arange(K, device=sc.device).expand(B, K)
    index = torch.where(sc == sc.max(1, keepdim=True).values, ks, K - 1).min(1).values
    rows = chunks.reshape((B, K) + tuple(chunks.shape[-2:]))
    return rows[torch.arange(B, device=rows.device), index.to(rows.device)], index


@torch.no_grad()
def log_likelihood(model, state, action, goal, sigma_min, sigma_max, extra_args=None, atol=1e-4, rtol=1e-4):
    """log p(action | state, goal) by integrating the probability-flow ODE dx/dsigma = (x - D(x; sigma)) / sigma from
    sigma_min to sigma_max together with its divergence, estimated with Rademacher probes v as v^T (d f / d x) v
    (reference gc_sampling.py:468-490).  Returns (log-likelihood per sample, {'fevals', 'steps', 'n_accept', 'n_reject'}).

    ``extra_args`` keys read here:
      'probes'     -- an int P >= 1 (default 1, the reference's single draw) or a tensor (P, *action.shape) of the caller's own
                      probes: the divergence estimate is the mean over the P probes.
      'candidates' -- K chunks for each of the B observations of ``state`` / ``goal``: ``action`` is (B*K, Ta, A) or
                      (B, K, Ta, A), chunk k of observation b at row b*K + k, and the result is (B*K,) or (B, K) to match
                      (``best_candidates`` picks from it).  A leading size other than B*K raises ValueError.

    With this package's GCDenoiser the whole integration is one blocking native call (``GCDenoiser.log_likelihood`` ->
    mdt_log_likelihood): the encoder runs once on the B observations, each evaluation is a decoder forward on the B*K chunks
    and one input-gradient-only backward per probe, and the Dormand-Prince loop reads one number back per attempted step.  One
    step size serves the whole call, so a chunk's value depends on its batch-mates at the integrator's tolerance.  Any further
    key (cond_lambda, pin) raises NotImplementedError.  Any other model is differentiated with torch.autograd in the host
    loop, as in the reference, and gets the other keys; it has no shared context to exploit, so 'candidates' raises
    ValueError."""
    rest = dict(extra_args or {})
    has_k = "candidates" in rest
    K, rest = take_candidates(rest)
    probes = rest.pop("probes", 1)
    if isinstance(model, GCDenoiser):
        if rest:
            raise NotImplementedError(f"log_likelihood: extra_args[{sorted(rest)[0]!r}] is not supported with GCDenoiser "
                                      "(the native call scores the unguided, unpinned model; keys read: 'candidates', 'probes')")
        rows, _ = _chunk_view(state, action, None, K)
        ll, _, _, info = model.log_likelihood(state, rows, goal, _probes(rows, probes), sigma_min, sigma_max, candidates=K,
                                              rtol=rtol, atol=atol)
        return ll.reshape(action.shape[:-2]), info
    if has_k:
        raise ValueError("log_likelihood: 'candidates' needs this package's GCDenoiser (a foreign model has no shared context to "
                         "exploit): expand the observations and score the chunks as a batch")
    v = _probes(action, probes)
    P = v.shape[0]
    info = {'fevals': 0, 'steps': 0, 'n_accept': 0, 'n_reject': 0}

    def flow(sigma, y):
        info['fevals'] += 1
        with torch.enable_grad():
            x = y[0].detach().requires_grad_()
            denoised = model(state, x, goal, x.new_full((x.shape[0],), sigma), **rest)
            d = to_d(x, sigma, denoised)
            div = 0
            for p in range(P):
                grad = torch.autograd.grad((d * v[p]).sum(), x, retain_graph=p + 1 < P)[0]
                div = div + (v[p] * grad).flatten(1).sum(1)
        return d.detach(), (div if P == 1 else div / P)

    latent, delta_ll = _dopri5(flow, (action, action.new_zeros([action.shape[0]])), float(sigma_min), float(sigma_max),
                               rtol, atol, stats=info)
    ll_prior = torch.distributions.Normal(0, sigma_max).log_prob(latent).flatten(1).sum(1)
    return ll_prior + delta_ll, info


def _score_levels(sigmas, weights):
    """The levels and weights of ``denoising_score`` as Python floats.  ``weights`` None: the trapezoid rule in ln sigma over the
    levels in the order given -- half the distance to each neighbour, 1 for a single level -- which needs strictly monotone
    levels.  What mdt_denoising_score checks and forms, in the same arithmetic (float64, rounded once)."""
    levels = [float(v) for v in (sigmas.detach().reshape(-1).tolist() if torch.is_tensor(sigmas) else sigmas)]
    S = len(levels)
    if S < 1:
        raise ValueError("denoising_score: sigmas must hold at least one level")
    for i, v in enumerate(levels):
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f"denoising_score: sigmas[{i}] is {v}, must be finite and > 0")
    if weights is not None:
        w = [float(v) for v in (weights.detach().reshape(-1).tolist() if torch.is_tensor(weights) else weights)]
        if len(w) != S:
            raise ValueError(f"denoising_score: weights hold {len(w)} values, {S} levels take {S}")
        for i, v in enumerate(w):
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"denoising_score: weights[{i}] is {v}, must be finite and >= 0")
        return levels, w
    up = S > 1 and levels[1] > levels[0]
    for i in range(1, S):
        if not (levels[i] > levels[i - 1] if up else levels[i] < levels[i - 1]):
            raise ValueError(f"denoising_score: sigmas[{i}] is {levels[i]} after {levels[i - 1]}: without weights the levels must be "
                             "strictly monotone (the default is the trapezoid rule in ln sigma)")
    ln = [math.log(v) for v in levels]
    return levels, [1.0 if S == 1 else 0.5 * ((abs(ln[i] - ln[i - 1]) if i > 0 else 0.0) +
                                              (abs(ln[i + 1] - ln[i]) if i + 1 < S else 0.0)) for i in range(S)]


@torch.no_grad()
def denoising_score(model, state, action, goal, sigmas, extra_args=None, draws=2, weights=None, noise=None, antithetic=True):
    """Score action chunks by their likelihood-weighted denoising error, forwards only:

        score = - sum_s w_s (1 / M) sum_m || (x0 - D(x0 + sigma_s n[s, m]; sigma_s)) / sigma_s ||^2

    over the S levels ``sigmas`` (any order; host values) and M = ``draws`` noise rows per level, the same rows for every chunk.
    By the pointwise I-MMSE relation this is log p(x0) up to a constant of the call for a denoiser that is the posterior mean,
    truncated to the range of the levels.  Higher is better and ``best_candidates(chunks, score, K)`` takes it as it is; it ranks
    chunks, it is no calibrated likelihood.  ``action`` is (B*K, Ta, A) or (B, K, Ta, A) and the result is shaped
    ``action.shape[:-2]``.

    ``weights``: None -- the trapezoid rule in ln sigma over the levels in the order given (they must then be strictly monotone; a
    single level weighs 1) -- or S values >= 0.  ``noise``: None or the rows (S, M, Ta, A).  None draws ``torch.randn`` rows of the
    action's dtype on its device in (S, M) order; with ``antithetic`` (the default) M / 2 rows per level, each followed directly
    by its negative, which cancels the part of the estimate that is odd in n -- on a Gaussian-mixture toy 2 such draws at 16 levels
    rank 8 candidates at Spearman 0.99 against the exact log p where 2 independent ones reach 0.75.  Odd ``draws`` then raise
    ValueError.  ``extra_args`` reads 'candidates' = K only: K chunks for each of the B observations of ``state`` / ``goal``, chunk k
    of observation b at row b*K + k.  Any other key raises NotImplementedError naming it.

    With this package's GCDenoiser the score is one native enqueue (``GCDenoiser.denoising_score`` -> mdt_denoising_score): the
    encoder once on the B observations, one decoder forward on B*K*S*M rows, one reduction -- no tape, no read-back, capturable.
    It forms q from the network's raw output without the subtraction x0 - D.  Any other model runs a host loop over the levels
    in its own dtype through ``model(state, x, goal, sigma)``; that loop uses the D form above as written, so in float32 its small
    levels carry the cancellation of x0 - D.  It has no shared context to exploit: 'candidates' raises ValueError there."""
    rest = dict(extra_args or {})
    has_k = "candidates" in rest
    K, rest = take_candidates(rest)
    if rest:
        raise NotImplementedError(f"denoising_score: extra_args[{sorted(rest)[0]!r}] is not supported (the score is that of the "
                                  "unguided, unpinned model; key read: 'candidates')")
    native = isinstance(model, GCDenoiser)
    if has_k and not native:
        raise ValueError("denoising_score: 'candidates' needs this package's GCDenoiser (a foreign model has no shared context to "
                         "exploit): expand the observations and score the chunks as a batch")
    levels, w = _score_levels(sigmas, weights)
    S = len(levels)
    Ta, A = action.shape[-2:]
    if noise is None:
        if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
            raise ValueError(f"denoising_score: draws must be an int >= 1, got {draws!r}")
        if antithetic:
            if draws % 2:
                raise ValueError(f"denoising_score: draws is {draws}: antithetic pairs need an even count (or antithetic=False)")
            half = torch.randn((S, draws // 2, Ta, A), dtype=action.dtype, device=action.device)
            noise = torch.stack((half, -half), dim=2).reshape(S, draws, Ta, A)
        else:
            noise = torch.randn((S, draws, Ta, A), dtype=action.dtype, device=action.device)
    elif noise.dim() != 4 or noise.shape[0] != S or noise.shape[1] < 1 or tuple(noise.shape[2:]) != (Ta, A):
        raise ValueError(f"denoising_score: noise is {tuple(noise.shape)}: {S} levels take ({S}, draws, {Ta}, {A})")
    if native:
        rows, _ = _chunk_view(state, action, None, K)
        return model.denoising_score(state, rows, goal, levels, noise, weights=None if weights is None else w,
                                     candidates=K).reshape(action.shape[:-2])
    rows = action.reshape(-1, Ta, A)
    noise = noise.to(device=rows.device, dtype=rows.dtype)
    M = noise.shape[1]
    score = rows.new_zeros(rows.shape[0])
    for s in range(S):
        sigma = rows.new_full((rows.shape[0],), levels[s])
        level = rows.new_zeros(rows.shape[0])
        for m in range(M):
            q = (rows - model(state, rows + levels[s] * noise[s, m], goal, sigma)) / levels[s]
            level = level + (q * q).flatten(1).sum(1)
        score = score - (w[s] / M) * level
    return score.reshape(action.shape[:-2])


# ------------------------------------------------------------------------------------------------
# sample, score and select as one native call
# ------------------------------------------------------------------------------------------------
# The samplers sample_select runs inside the one call, with the draws their sample_<name> makes at its default parameters: None,
# one randn per step ("steps": the churn's, drawn whether it is used or not), or one per step that adds noise ("ancestral").  Any
# other sampler runs the three functions in sequence.
_SELECT_DRAWS = {"ddim": None, "dpmpp_2m": None, "lms": None, "euler": "steps", "heun": "steps", "dpm_2": "steps",
                 "euler_ancestral": "ancestral", "dpm_2_ancestral": "ancestral"}


def _select_sequence(model, state, action, goal, sigmas, levels, sampler, scaler, extra_args, K, draws, weights, noise, antithetic):
    """sample_select as its three functions: ``sample_<sampler>``, ``denoising_score``, ``best_candidates``."""
    fn = globals().get("sample_" + sampler)
    if fn is None or sampler in ("select", "dpm_fast"):
        raise ValueError(f"sample_select: no sampler {sampler!r} that takes a schedule")
    if sampler == "dpm_adaptive":  # the two ends of the schedule are its range
        sig = [float(v) for v in sigmas if float(v) > 0]
        chunks = fn(model, state, action, goal, min(sig), max(sig), extra_args=extra_args)
    else:
        chunks = fn(model, state, action, goal, sigmas, scaler=scaler, extra_args=extra_args)
    has_k = extra_args is not None and "candidates" in extra_args
    scores = denoising_score(model, state, chunks, goal, levels, extra_args={"candidates": K} if has_k else None, draws=draws,
                             weights=weights, noise=noise, antithetic=antithetic)
    if not has_k:  # a foreign model: every chunk its own observation
        return chunks, torch.zeros(chunks.shape[:-2], dtype=torch.int64, device=chunks.device).reshape(-1), scores, chunks
    best, index = best_candidates(chunks, scores, K)
    return best, index, scores, chunks


@torch.no_grad()
def sample_select(model, state, action, goal, sigmas, levels, sampler="ddim", scaler=None, extra_args=None, draws=2, weights=None,
                  noise=None, antithetic=True):
    """The replan-and-select loop as one call: K candidate chunks per observation sampled from ``action`` by ``sample_<sampler>``
    over ``sigmas``, scored by ``denoising_score`` over ``levels`` (``draws``, ``weights``, ``noise`` and ``antithetic`` are its
    arguments: ``noise`` the score's rows (S, M, Ta, A)), and the best of each observation picked by ``best_candidates``.  Returns
    (best (B, Ta, A), index (B,) int64, scores, chunks): ``chunks`` in ``action``'s shape -- (B*K, Ta, A) or (B, K, Ta, A) -- and
    ``scores`` in ``action.shape[:-2]``.

    ``extra_args`` reads 'candidates' = K (required with this package's GCDenoiser), 'cond_lambda' and 'pin'; any other key raises
    NotImplementedError naming it.  The guidance weight, the pin and the scaler's bounds shape the sampling only: the score is that
    of the unguided, unpinned model, as ``denoising_score``'s is.

    With a GCDenoiser, a schedule and scaler the native samplers admit, and ``sampler`` one of ddim, euler, heun, dpm_2,
    euler_ancestral, dpm_2_ancestral, lms, dpmpp_2m (at their default parameters) it is ONE native enqueue
    (``GCDenoiser.sample_select`` -> mdt_sample_ddim_select / mdt_sample_select): where the context does not depend on sigma the
    encoder runs once for both halves, the selection is one kernel, nothing is read back.  The sampler's noise rows and then the
    score's are drawn as the three functions draw them, so a seeded call gives their result.  Rollout-sized calls (B*K <= 8) are
    replayed as a HIP graph by ``sample_ddim``'s rule (MDT_HIP_GRAPH); the levels and weights are host values and belong to the
    graph's key, the noise rows, the pin and the bounds sit in static buffers filled before every replay.

    Anything else -- a foreign ``model``, a scaler without ``clip_bounds``, another ``sampler`` ('dpm_adaptive' reads the schedule's
    largest and smallest positive level as its range) -- runs the three functions in sequence and returns the same tuple.  A
    foreign model has no shared context: 'candidates' raises the ValueError ``denoising_score`` raises, and without it every chunk
    is its own observation."""
    rest = dict(extra_args or {})
    for k in sorted(rest):
        if k not in ("candidates", "cond_lambda", "pin"):
            raise NotImplementedError(f"sample_select: extra_args[{k!r}] is not supported (keys read: 'candidates', 'cond_lambda', "
                                      "'pin')")
    ours = isinstance(model, GCDenoiser)
    if "candidates" in rest and not ours:
        raise ValueError("denoising_score: 'candidates' needs this package's GCDenoiser (a foreign model has no shared context to "
                         "exploit): expand the observations and score the chunks as a batch")
    if ours and "candidates" not in rest:
        raise ValueError("sample_select: extra_args['candidates'] (chunks per observation) is required")
    _, lam, pin, K = _controls(rest)
    ddim = sampler == "ddim"
    if not (ours and sampler in _SELECT_DRAWS and _native_ok(model, sigmas, None if ddim else scaler, None, rest)):
        return _select_sequence(model, state, action, goal, sigmas, levels, sampler, scaler, extra_args, K, draws, weights, noise,
                                antithetic)
    lv, w = _score_levels(levels, weights)
    S = len(lv)
    Ta, A = action.shape[-2:]
    if noise is not None and (noise.dim() != 4 or noise.shape[0] != S or noise.shape[1] < 1 or tuple(noise.shape[2:]) != (Ta, A)):
        raise ValueError(f"sample_select: noise is {tuple(noise.shape)}: {S} levels take ({S}, draws, {Ta}, {A})")
    rule = _SELECT_DRAWS[sampler]
    rows_noise = None if rule is None else _randn_rows(action, len(sigmas) - 1 if rule == "steps" else _ancestral_draws(sigmas, 1.))
    if noise is None:
        noise = draw_score_noise("sample_select", S, draws, antithetic, Ta, A, action.dtype, action.device)
    shape = action.shape
    rows, rows_noise = _chunk_view(state, action, rows_noise, K)
    bounds = None if scaler is None or ddim else scaler.clip_bounds(rows.device)
    if pin is not None:
        pin = pin.on(rows.device, rows.shape, K)
    kind = None if ddim else sampler
    wkey = None if weights is None else tuple(w)
    key = ("select", sampler, K, tuple(lv), wkey, int(noise.shape[1]), lam, bounds is not None, pin is not None)
    out = _graph_route(model, "_graphed_select", key, key, state, rows, goal, sigmas,
                       lambda sig: GraphedSelect(model, kind, key, state, rows, goal, sig, (rows_noise, noise), lv,
                                                 None if weights is None else w, K, cond_lambda=lam, bounds=bounds, pin=pin),
                       f"sample_select({sampler})", noise=(rows_noise, noise), bounds=bounds, pin=pin)
    if out is None:
        kw = {} if lam is None else {"cond_lambda": lam}
        out = model.sample_select(state, rows, goal, sigmas, lv, K, kind=kind, noise=rows_noise, pin=pin, bounds=bounds,
                                  weights=None if weights is None else w, score_noise=noise, **kw)
    best, index, scores, chunks = out
    return best, index, scores.reshape(shape[:-2]), chunks.reshape(shape)
