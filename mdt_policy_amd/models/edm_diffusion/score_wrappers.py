"""EDM preconditioner facade (reference: mdt/models/edm_diffusion/score_wrappers.py:18-100).

``GCDenoiser(inner_model, sigma_data)`` keeps the reference's constructor (Hydra ``_target_`` with
``_recursive_: false``: ``inner_model`` arrives as a DictConfig and is instantiated here), methods and
state_dict (``inner_model.*``).  ``forward`` / ``loss`` / ``forward_context_only`` each are a single call into
libmdt_hip.so; the preconditioning arithmetic (c_skip, c_out, c_in) runs inside the action-embedding and
action-head kernels.
"""
from __future__ import annotations

import importlib
import math
from contextlib import contextmanager

import torch
from torch import nn

from ..networks._engine import HipScoreNetwork, candidate_count, chunk_rows, steer_alone, take_steer


def _staged_backward() -> bool:
    """One autograd node per stage of the HIP backward (``_autograd.staged_diffusion_loss``) instead of one for all of it:
    MDT_HIP_BWD_STAGES=1 always, 0 never, unset: whenever a process group with more than one rank exists -- the case in which
    gradients that appear block by block let DistributedDataParallel reduce them behind the backward."""
    import os
    v = os.environ.get("MDT_HIP_BWD_STAGES", "auto")
    if v != "auto":
        return v not in ("", "0")
    try:
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    except Exception:  # noqa: BLE001
        return False


def _instantiate(cfg):
    """hydra.utils.instantiate when Hydra is installed, else the same thing for a flat kwargs mapping."""
    if isinstance(cfg, nn.Module):
        return cfg
    try:
        import hydra  # the user's harness has it; the build/GPU images do not
        return hydra.utils.instantiate(cfg)
    except ImportError:
        kwargs = {k: v for k, v in dict(cfg).items() if k not in ("_target_", "_recursive_")}
        module, cls = dict(cfg)["_target_"].rsplit(".", 1)
        return getattr(importlib.import_module(module), cls)(**kwargs)


def _record_sigmas(kind, sigmas, n_steps, params):
    """(sigma, sigma_hat) of every step of a native sampler call, as its Python loop hands them to ``callback``: from
    mdt_sampler_plan for a host schedule (CPU tensors), computed with torch in place for a device one (no read-back)."""
    from ... import _lib
    if not (torch.is_tensor(sigmas) and sigmas.device.type == "cuda"):
        sig = [float(v) for v in sigmas]
        plan = _lib.sampler_plan(kind, sig, n_steps, **params)
        first = [plan.e[k] for k in range(plan.n_evals) if plan.e[k].begins_step]
        hat = torch.tensor([e.sigma for e in first], dtype=torch.float32)
        return (hat.clone() if kind == "dpm_fast" else torch.tensor(sig[:len(first)], dtype=torch.float32)), hat
    sig = sigmas.detach().to(torch.float32).reshape(-1)
    if kind == "dpm_fast":  # the solver steps' left ends on the uniform grid in t = -ln(sigma)
        m = int(n_steps) // 3 + 1
        t = torch.stack([torch.lerp(-sig[0].log(), -sig[1].log(), i / m) for i in range(m)])
        return t.neg().exp(), t.neg().exp()
    sigma = sig[:-1]
    if kind in ("euler", "heun", "dpm_2") and params.get("s_churn", 0.):
        gamma = min(params["s_churn"] / sigma.numel(), 2 ** 0.5 - 1)
        inside = (sigma >= params.get("s_tmin", 0.)) & (sigma <= params.get("s_tmax", float("inf")))
        return sigma, sigma * (1 + gamma * inside.to(sigma.dtype))
    return sigma, sigma.clone()


def _record_dict(rec, kind, sigmas, n_steps, params):
    """A native call's (steps, 2, ...) record tensor as the dict a ``callback`` of the loop sees, step by step."""
    sigma, sigma_hat = _record_sigmas(kind, sigmas, n_steps, params)
    return {"x": rec[:, 0], "denoised": rec[:, 1], "sigma": sigma, "sigma_hat": sigma_hat}


def _bounds_pair(bounds, device):
    """An ``ActionBounds`` or a (lo, hi) pair as two fp32 tensors on ``device``; None as it came."""
    pair = bounds.clip_bounds(device) if callable(getattr(bounds, "clip_bounds", None)) else bounds
    return None if bounds is None else tuple(torch.as_tensor(b, dtype=torch.float32).to(device) for b in pair)


def _pin_rows(pin, action, K):
    """An ``ActionPin`` as its (known, keep) pair over the chunks of ``action``; a pair, or None, as it came."""
    Ta, A = action.shape[-2:]
    return pin.on(action.device, (action.numel() // (Ta * A), Ta, A), K) if callable(getattr(pin, "on", None)) else pin


def draw_score_noise(who, S, draws, antithetic, Ta, A, dtype, device):
    """The noise rows (S, draws, Ta, A) of a denoising score whose caller gave none, by ``gc_sampling.denoising_score``'s rule:
    ``torch.randn`` in (S, M) order; with ``antithetic`` draws / 2 rows per level, each followed directly by its negative, and an
    odd ``draws`` raises ValueError."""
    if isinstance(draws, bool) or not isinstance(draws, int) or draws < 1:
        raise ValueError(f"{who}: draws must be an int >= 1, got {draws!r}")
    if not antithetic:
        return torch.randn((S, draws, Ta, A), dtype=dtype, device=device)
    if draws % 2:
        raise ValueError(f"{who}: draws is {draws}: antithetic pairs need an even count (or antithetic=False)")
    half = torch.randn((S, draws // 2, Ta, A), dtype=dtype, device=device)
    return torch.stack((half, -half), dim=2).reshape(S, draws, Ta, A)


class GCDenoiser(nn.Module):
    """Karras et al. (2022) preconditioner around the MI355X-native score network."""

    def __init__(self, inner_model, sigma_data=1.):
        super().__init__()
        self.inner_model = _instantiate(inner_model)
        if not isinstance(self.inner_model, HipScoreNetwork):
            raise TypeError("mdt_policy_amd.GCDenoiser wraps mdt_policy_amd score networks "
                            f"(MDTVTransformer / MDTTransformer), got {type(self.inner_model).__name__}")
        self.sigma_data = sigma_data
        self.inner_model._sigma_data = float(sigma_data)
        self._ctx_key = None

    # -- reference API -------------------------------------------------------------------------
    def get_scalings(self, sigma):
        """c_skip, c_out, c_in (reference score_wrappers.py:31-43)."""
        sd = self.sigma_data
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd / (sigma ** 2 + sd ** 2) ** 0.5
        c_in = 1 / (sigma ** 2 + sd ** 2) ** 0.5
        return c_skip, c_out, c_in

    def _engine(self, allow_grad: bool = False, state=None):
        self.inner_model._sigma_data = float(self.sigma_data)
        self.inner_model._guard_mode(allow_grad)
        return self.inner_model.hip_engine(float(self.sigma_data), state)

    def _wants_grad(self, *tensors) -> bool:
        return torch.is_grad_enabled() and (any(p.requires_grad for p in self.inner_model.parameters()) or
                                            any(torch.is_tensor(t) and t.requires_grad for t in tensors))

    def _train_inputs(self, eng, state, goal, honour_modality: bool, uncond: bool = False):
        """Encoder inputs as the contiguous fp32 tensors the C ABI takes, still attached to the autograd graph, and
        the parameters THIS forward reads: the others (proprio_emb, MDT-V's pos_emb, the other modality's goal
        embedder) stay out of the graph, so their .grad stays None and DistributedDataParallel's
        find_unused_parameters sees them exactly as it does on the reference modules."""
        im = self.inner_model
        prep = lambda t: t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0) \
            else t.float().contiguous().clone()
        if im._arch == "mdtv":
            # the proprioceptive input rides in the second token slot of the C ABI (include/mdt_hip.h: tokens2)
            tok, tok2 = prep(state["state_images"]), (prep(state["state_obs"]) if eng.proprio else None)
            B = tok.shape[0]
        else:
            tok, tok2 = prep(state["static"]), prep(state["gripper"])
            B = tok.shape[0]
        eng._tokens(state)  # shape validation
        g = prep(im._goals(goal, uncond))  # uncond: the goal is zeroed (preprocess_goals, mdtv_transformer.py:256-257)
        eng._goal(g, B)
        eng.train_prepare()
        unused = eng.unused_goal_embedder(state, honour_modality)
        named = [(n, p) for n, p in im.named_parameters()
                 if ("inner_model." + n) in eng._grad_layout and not (unused and n.startswith(unused))]
        return tok, tok2, g, B, [n for n, _ in named], [p for _, p in named]

    def forward(self, state, action, goal, sigma, cond_lambda=1.0, pin=None, candidates=None, steer=None, **kwargs):
        """D(x; sigma) = F(x*c_in, sigma)*c_out + x*c_skip (reference score_wrappers.py:65-80).

        ``cond_lambda`` != 1: classifier-free guidance, D_lambda = D(x; sigma, 0) + lambda (D(x; sigma, g) - D(x; sigma, 0)) from the
        conditional and the ``uncond`` evaluation (the latter first, so latent_encoder_emb ends as the conditional context).
        ``pin`` (an ActionPin, utils/action_pin.py): pinned actions, D' = keep * known + (1 - keep) * D, applied after the
        guidance -- what the native samplers compute in their action head.
        ``candidates`` = K: ``action`` holds K chunks for each of the B observations of ``state`` and ``goal``, (B*K, Ta, A) or
        (B, K, Ta, A), chunk k of observation b at row b*K + k; the observations are expanded with ``repeat_interleave`` and the
        call runs at batch B*K (the samplers' host loops; the native samplers encode each observation once instead).  A pin
        given per observation goes to each of its chunks; latent_encoder_emb stays (B, Te, d).
        ``steer`` (an ActionSteer, utils/action_steer.py): D' = D + s(sigma) J^T (weight (known - D)) from one taped decoder forward
        and one input-gradient-only backward over it; with ``candidates`` the observations are encoded once.  Together with
        ``cond_lambda`` != 1 or ``pin`` it raises NotImplementedError.  A steer whose weight is all zero is no steer."""
        steer = take_steer({"steer": steer})[0]
        if steer is not None:
            steer_alone(cond_lambda=cond_lambda, pin=pin)
            return self._steered(state, action, goal, sigma, steer, candidates, **kwargs)
        K = candidate_count(candidates)
        if K != 1 or (candidates is not None and action.dim() == 4):
            B = next(v for v in state.values() if torch.is_tensor(v)).shape[0]
            rows = chunk_rows(action, B, K)
            wide = {k: (v.repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
            out = self.forward(wide, rows, goal.repeat_interleave(K, 0), sigma, cond_lambda=cond_lambda, **kwargs)  # sigma: 1 or B*K values
            im = self.inner_model
            if torch.is_tensor(im.latent_encoder_emb) and im.latent_encoder_emb.shape[0] == B * K:
                im.latent_encoder_emb = im.latent_encoder_emb[::K]
            if pin is not None:
                out = pin.apply(out, K)
            return out.reshape(action.shape)
        if pin is not None:
            return pin.apply(self.forward(state, action, goal, sigma, cond_lambda=cond_lambda, **kwargs))
        lam = float(cond_lambda)
        if lam != 1.0:
            if not math.isfinite(lam):
                raise ValueError(f"cond_lambda must be finite, got {lam}")
            if kwargs.get("uncond", False):
                raise ValueError("uncond=True and cond_lambda != 1 contradict each other")
            kwargs = {k: v for k, v in kwargs.items() if k != "uncond"}
            d_u = self.forward(state, action, goal, sigma, uncond=True, **kwargs)
            d_g = self.forward(state, action, goal, sigma, **kwargs)
            return d_u + lam * (d_g - d_u)
        im = self.inner_model
        eng = self._engine(state=state)
        goal = im._goals(goal, bool(kwargs.get("uncond", False)))
        if self._ctx_key is not None and self._ctx_key == (id(state), id(goal), action.shape[0], eng.ctx_generation):
            return eng.denoise_cached(action, sigma, 0)  # inside cached_context(): encoder hoisted
        # (any other call that re-encoded on this handle since -- an uncond / other-state evaluation inside the block --
        #  bumped eng.ctx_generation: the key no longer matches and this call runs the full forward)
        out, ctx = eng.forward(state, action, goal, sigma)
        im.latent_encoder_emb = ctx
        return out

    def _steered(self, state, action, goal, sigma, steer, candidates=None, **kwargs):
        """``forward`` with an active steer: the context of the B observations (the one ``cached_context`` holds, where it is
        this call's), the taped decoder forward on the B*K chunks, e = weight (known - D), the backward for d_x alone."""
        im = self.inner_model
        K = candidate_count(candidates)
        eng = self._engine(state=state)
        g = im._goals(goal, bool(kwargs.get("uncond", False)))
        B = next(v for v in state.values() if torch.is_tensor(v)).shape[0]
        rows = chunk_rows(action, B, K) if (K != 1 or action.dim() == 4) else action
        R = rows.shape[0]
        sg = sigma.to(device=rows.device, dtype=torch.float32).reshape(-1)
        if sg.numel() not in (1, R):
            raise ValueError(f"sigma holds {sg.numel()} values, {R} chunks take 1 or {R}")
        if self._ctx_key is not None and self._ctx_key == (id(state), id(g), B, eng.ctx_generation):
            ctx = im.latent_encoder_emb  # inside cached_context(): encoder hoisted
        else:  # (sigma is read by use_ada_conditioning=False models only: one value per observation)
            ctx = eng.encode(state, g, honour_modality=im._arch == "mdtv", sigma=sg if sg.numel() == 1 else sg[::K])
            im.latent_encoder_emb = ctx
        sg = sg.expand(R) if sg.numel() == 1 else sg
        den, tape = eng.train_denoise_fwd(eng._in(ctx if K == 1 else ctx.repeat_interleave(K, 0)),
                                          eng._in(rows, (R, eng.Ta, eng.A)), eng._in(sg, (R,)))
        try:
            jte = eng.train_denoise_bwd(tape, steer.error(den, K), R, (False, True, False), False)[2]
        finally:
            eng.tape_release(tape)
        return (den + steer.scale(sg, self.sigma_data).reshape(R, 1, 1) * jte).reshape(action.shape)

    def loss(self, state, action, goal, noise, sigma, **kwargs):
        """Denoising score-matching loss, forward value (reference score_wrappers.py:45-63)."""
        im = self.inner_model
        if self._wants_grad(goal, *[v for v in state.values() if torch.is_tensor(v)]):
            # training step: HIP forward with a tape + HIP backward behind torch.autograd
            from ._autograd import HipDiffusionLoss, staged_diffusion_loss
            eng = self._engine(allow_grad=True, state=state)
            tok, tok2, g, B, names, params = self._train_inputs(eng, state, goal, im._arch == "mdtv")
            a, nz = eng._in(action, (B, eng.Ta, eng.A)), eng._in(noise, (B, eng.Ta, eng.A))
            if _staged_backward():  # one autograd node per stage of the backward: gradients appear block by block (DDP overlap)
                eng.train_prepare()
                loss, model_output, ctx = staged_diffusion_loss(eng, state, tok, tok2, g, a, nz, eng._in(sigma, (B,)),
                                                                im.train_dropout(), names, params)
            else:
                loss, model_output, ctx = HipDiffusionLoss.apply(eng, state, tok, tok2, g, a, nz, eng._in(sigma, (B,)),
                                                                 im.train_dropout(), names, *params)
            im.latent_encoder_emb = ctx
            return loss, model_output
        loss, model_output, ctx = self._engine(state=state).loss_fwd(state, action, im._goals(goal, False), noise, sigma)
        im.latent_encoder_emb = ctx
        return loss, model_output

    def forward_context_only(self, state, action, goal, sigma, **kwargs):
        """Encoder tokens only (reference score_wrappers.py:82-97 -> inner_model.forward_enc_only)."""
        im = self.inner_model
        if self._wants_grad(goal, *[v for v in state.values() if torch.is_tensor(v)]):
            from ._autograd import HipContextOnly
            eng = self._engine(allow_grad=True, state=state)
            tok, tok2, g, B, names, params = self._train_inputs(eng, state, goal, True, bool(kwargs.get("uncond", False)))
            sg = eng._in(sigma, (B,)) if eng.sigma_in_context else None  # the sigma token leads the context
            ctx = HipContextOnly.apply(eng, state, tok, tok2, g, True, im.train_dropout(), sg, names, *params)
            if im._arch == "mdtv":
                im.latent_encoder_emb = ctx
            return ctx
        return im.forward_enc_only(state, action, goal, sigma, **kwargs)

    def get_params(self):
        return self.inner_model.parameters()

    def _context_engine(self, state, context):
        """The handle a given context tensor belongs to: the one ``state`` selects or, where its context layout has another
        token count (MDT-V with / without the proprioceptive token; ``state`` may be None), the other layout's."""
        eng = self._engine(allow_grad=True, state=state)
        if self.inner_model._arch == "mdtv" and context.dim() == 3 and context.shape[1] != eng.Te:
            other = {} if eng.proprio else {"state_obs": None}  # hip_engine keys on the presence of 'state_obs' alone
            try:
                alt = self._engine(allow_grad=True, state=other)
            except Exception:  # noqa: BLE001 -- a model without that layout: the shape error below names the mismatch
                return eng
            if context.shape[1] == alt.Te:
                return alt
        return eng

    def denoise_grad(self, state, action, goal, sigma, cond_lambda=1.0, context=None, uncond=False):
        """``forward`` recorded by torch.autograd: D(x; sigma), differentiable in the parameters, the state tokens, the goal,
        the noisy ``action`` and ``sigma`` -- custom objectives on the denoised chunk, guidance gradients, hand-unrolled solver
        steps.  The implicit call ``self(...)`` stays inference-only; this is the opt-in.

        ``context``: None -- the encoder runs as a differentiable node of its own (as ``forward`` runs it; latent_encoder_emb is
        set); or a context tensor, e.g. one ``forward_context_only`` under autograd, against which only the decoder runs: several
        evaluations then share one encoder forward and backward (``goal`` is not read, ``state`` may be None: the handle is the one
        whose context layout has the tensor's token count, with or without the proprioceptive token; with
        use_ada_conditioning=False the context must have been encoded with this ``sigma``).  ``cond_lambda`` != 1 composes
        d_u + lambda (d_g - d_u) from two evaluations as ``forward`` does (needs ``context`` None).  In train() mode the shipped
        dropouts apply, a fresh seed per evaluation, as in ``loss``.  Under torch.no_grad(), or when nothing requires grad, this
        is ``forward``.  ``sigma.requires_grad`` on a use_ada_conditioning=False model raises: sigma is a context token there
        and its gradient through the encoder is not formed."""
        lam = float(cond_lambda)
        if lam != 1.0:
            if not math.isfinite(lam):
                raise ValueError(f"cond_lambda must be finite, got {lam}")
            if uncond:
                raise ValueError("uncond=True and cond_lambda != 1 contradict each other")
            if context is not None:
                raise ValueError("cond_lambda != 1 encodes the goal and the zeroed goal itself: it takes no context")
            d_u = self.denoise_grad(state, action, goal, sigma, uncond=True)
            d_g = self.denoise_grad(state, action, goal, sigma)
            return d_u + lam * (d_g - d_u)
        im = self.inner_model
        tensors = [goal, action, sigma, context] + ([v for v in state.values() if torch.is_tensor(v)] if context is None else [])
        if not self._wants_grad(*tensors):
            if context is None:
                return self.forward(state, action, goal, sigma, uncond=uncond)
            eng = self._context_engine(state, context)  # a given context: the taped decoder forward, its tape handed back
            B = action.shape[0]
            sg = sigma.reshape(-1).expand(B) if sigma.numel() == 1 and B > 1 else sigma
            out, tape = eng.train_denoise_fwd(eng._in(context), eng._in(action, (B, eng.Ta, eng.A)), eng._in(sg, (B,)),
                                              im.train_dropout())
            eng.tape_release(tape)
            return out
        from ._autograd import HipContextOnly, HipDenoise
        eng = self._engine(allow_grad=True, state=state) if context is None else self._context_engine(state, context)
        if eng.sigma_in_context and torch.is_tensor(sigma) and sigma.requires_grad:
            raise NotImplementedError("use_ada_conditioning=False: sigma is a context token and its gradient through the encoder "
                                      "is not formed (d_sigma exists for adaLN-Zero and NoiseBlock conditioning only)")
        B = action.shape[0]
        drop = im.train_dropout()  # one seed for the encoder's and the decoder's sites, as in loss
        # float32 (B,) / (B, Ta, A) views by differentiable torch ops: the node sees the layout the C ABI takes
        sg = sigma.to(torch.float32).reshape(-1)
        sg = sg.expand(B) if sg.numel() == 1 and B > 1 else sg
        x = action.to(torch.float32).reshape(B, eng.Ta, eng.A)
        if context is None:
            tok, tok2, g, Bs, names, params = self._train_inputs(eng, state, goal, im._arch == "mdtv", uncond)
            if Bs != B:
                raise ValueError(f"state holds {Bs} samples, action {B}")
            s_tok = eng._in(sg, (B,)) if eng.sigma_in_context else None  # the sigma token leads the context
            enc = [(n, p) for n, p in zip(names, params) if not eng.decoder_side(n)]  # the decoder's get theirs from the node below
            context = HipContextOnly.apply(eng, state, tok, tok2, g, im._arch == "mdtv", drop, s_tok, [n for n, _ in enc],
                                           *[p for _, p in enc])
            im.latent_encoder_emb = context
        else:
            eng.train_prepare()
            context = context.to(torch.float32)
        named = [(n, p) for n, p in im.named_parameters() if ("inner_model." + n) in eng._grad_layout and eng.decoder_side(n)]
        return HipDenoise.apply(eng, context, x, sg, drop, [n for n, _ in named], *[p for _, p in named])

    # -- additions ---------------------------------------------------------------------------
    @contextmanager
    def cached_context(self, state, goal):
        """Evaluate the (sigma-independent) encoder + cross-attention K/V once and reuse them for every
        ``self(state, x, goal, sigma)`` inside the block -- what the Python samplers in gc_sampling use."""
        im = self.inner_model
        eng = self._engine(state=state)
        if eng.sigma_in_context:  # use_ada_conditioning=False: sigma is a context token, nothing can be hoisted
            yield None
            return
        g = im._goals(goal, False)
        ctx = eng.encode(state, g, honour_modality=im._arch == "mdtv")
        im.latent_encoder_emb = ctx
        B = ctx.shape[0]
        prev = self._ctx_key
        # _goals() returns its argument unchanged for the usual (B, goal_seq_len, goal_dim) goal, so id(goal) identifies it
        self._ctx_key = (id(state), id(g), B, eng.ctx_generation) if g is goal else None
        try:
            yield ctx
        finally:
            self._ctx_key = prev

    @torch.no_grad()
    def denoise_vjp(self, state, action, goal, sigma, v):
        """(D(action; sigma), (dD/daction)^T v) in eval-mode arithmetic: what gc_sampling.log_likelihood needs from
        autograd through ``self(state, action, goal, sigma)`` (reference gc_sampling.py:477-484), as one HIP forward
        and an input-gradient-only HIP backward."""
        im = self.inner_model
        return self._engine(state=state).denoise_vjp(state, action, im._goals(goal, False), sigma, v)

    @torch.no_grad()
    def log_likelihood(self, state, action, goal, v, sigma_min, sigma_max, candidates=None, rtol=1e-4, atol=1e-4, max_steps=10000):
        """gc_sampling.log_likelihood's integration as one blocking native call (mdt_log_likelihood): the encoder and the cross
        K|V product once on the B observations of ``state`` / ``goal``, every evaluation one decoder forward on the B*K chunks of
        ``action`` -- (B*K, Ta, A) or (B, K, Ta, A), ``candidates`` = K -- and one input-gradient-only backward per probe tensor
        of ``v`` (P, B*K, Ta, A).  Returns (ll (B*K,), latent (B*K, Ta, A), delta (B*K,), info) with info = {'fevals', 'steps',
        'n_accept', 'n_reject'}.  One step size serves the whole call: a chunk's value depends on its batch-mates at the
        integrator's tolerance."""
        im = self.inner_model
        return self._engine(state=state).log_likelihood(state, action, im._goals(goal, False), v, float(sigma_min), float(sigma_max),
                                                        candidates=candidate_count(candidates), rtol=rtol, atol=atol,
                                                        max_steps=max_steps)

    @torch.no_grad()
    def denoising_score(self, state, rows, goal, sigmas, noise, weights=None, candidates=1):
        """gc_sampling.denoising_score as one native enqueue (mdt_denoising_score): the encoder and the cross K|V product once on
        the B observations of ``state`` / ``goal``, one decoder forward over B*K*S*M rows -- the chunks ``rows``, (B*K, Ta, A) or
        (B, K, Ta, A) with ``candidates`` = K, at the S levels ``sigmas`` (host values) with the M noise rows per level of
        ``noise`` (S, M, Ta, A) -- and one reduction.  ``weights``: None (trapezoid in ln sigma) or S host values.  Returns the
        score (B*K,), higher is better; latent_encoder_emb is set to the observations' context.  No tape, no read-back, no
        synchronisation: the call can be captured into a graph after one eager call has sized the workspace."""
        im = self.inner_model
        score, ctx = self._engine(state=state).denoising_score(state, rows, im._goals(goal, False), sigmas, noise, weights=weights,
                                                               candidates=candidate_count(candidates))
        im.latent_encoder_emb = ctx
        return score

    @torch.no_grad()
    def sample_native(self, kind, state, action, goal, sigmas, noise=None, n_steps=None, cond_lambda=None, tree=None, bounds=None,
                      record=False, pin=None, candidates=None, **params):
        """One of the other samplers (``kind``: 'euler', 'heun', 'dpmpp_2m', ... -- the gc_sampling function name without
        'sample_') as one enqueue on the current stream (mdt_sample).  ``noise``: None or (n_noise, B, Ta, A) in the Python loop's
        draw order -- raw randn draws (euler / heun / dpm_2 / the ancestral samplers) or the noise_sampler values (dpmpp_2s_ancestral,
        dpmpp_sde); s_noise and the step scales are applied inside.  ``params``: the sampler's keyword arguments (eta, s_churn,
        s_tmin, s_tmax, s_noise, r, order).  'dpm_fast': ``sigmas`` is [sigma_max, sigma_min] and ``n_steps`` the evaluation
        count.  ``cond_lambda``: classifier-free guidance weight (None or 1: the unguided call; include/mdt_hip.h
        mdt_sample_guided; _engine.guidance reads it).  ``tree`` ('dpmpp_sde' only, in place of ``noise``): (seeds, tol) or
        (seeds, tol, lo, hi) -- the Brownian tree the call draws its noise rows from (mdt_sample_sde_tree): ``seeds`` an int64
        tensor of 1 or B keys on the model's device, ``lo`` < ``hi`` the tree's interval (default: the schedule's).
        ``bounds``: an ``ActionBounds`` (utils/action_bounds.py) or a (lo, hi) pair of length-A sequences / tensors -- what the
        loop's ``scaler.clip_output`` clamps to, applied inside the call where the reference's loop of this kind clips (after
        every step; dpmpp_sde: not after the last; dpmpp_2m and dpm_fast: never -- include/mdt_hip.h mdt_sample_opts).
        ``record=True``: returns (actions, rec) with rec = {'x', 'denoised': (n_steps, B, Ta, A), 'sigma', 'sigma_hat':
        (n_steps,)}, what a ``callback`` of the loop sees per step (dpm_fast: per solver step); gc_sampling.replay_callback feeds
        it to one.  The actions are those of the call without ``record``, bit for bit.
        ``pin``: an ``ActionPin`` (utils/action_pin.py) or its (known, keep) pair of (B, Ta, A) device tensors -- pinned actions:
        every evaluation's denoised value becomes keep * known + (1 - keep) * D inside the action head (mdt_sample_opts.pin_known /
        pin_keep), for every kind, guided or not, with bounds, record and tree noise as without it.
        ``candidates`` = K (an int >= 1): K action chunks for each of the B observations of ``state`` and ``goal`` from ONE encoded
        context (mdt_sample_multi): the encoder, the cross K|V product and the cross-attention fold run on B samples, the decoder on
        B*K.  ``action`` is (B*K, Ta, A) or (B, K, Ta, A), chunk k of observation b at row b*K + k, and the result has its shape;
        ``noise``, the record, ``tree``'s seeds and a per-chunk pin count chunks the same way; a pin given per observation,
        (B, Ta, A), goes to each of its K chunks; latent_encoder_emb is (B, Te, d).  A leading size other than B*K raises ValueError."""
        from ... import _lib
        im = self.inner_model
        K = candidate_count(candidates)
        pin = _pin_rows(pin, action, K)
        bounds = _bounds_pair(bounds, action.device)
        if tree is not None:
            if kind != "dpmpp_sde" or noise is not None or n_steps is not None:
                raise ValueError("sample_native: tree noise is for 'dpmpp_sde' and takes no noise rows")
            tree = (tuple(tree) + (0., 0.))[:4]
        out, ctx, rec = self._engine(state=state).sample_native(
            _lib.SAMPLER_KIND[kind], _lib.sampler_params(**params), state, action, im._goals(goal, False), sigmas, noise,
            n_steps=n_steps, cond_lambda=cond_lambda, tree=tree, bounds=bounds, record=record, pin=pin, candidates=K)
        im.latent_encoder_emb = ctx
        return (out, _record_dict(rec, kind, sigmas, n_steps, params)) if record else out

    @torch.no_grad()
    def sample_select(self, state, action, goal, sigmas, levels, candidates, kind=None, noise=None, n_steps=None, cond_lambda=1.0,
                      pin=None, bounds=None, draws=2, weights=None, score_noise=None, antithetic=True, **params):
        """Sample, score and select as one enqueue (mdt_sample_ddim_select, ``kind`` None; mdt_sample_select, ``kind`` a sampler
        name): ``candidates`` = K chunks per observation sampled as ``sample_ddim`` / ``sample_native`` sample them (``sigmas``,
        ``noise``, ``n_steps``, ``cond_lambda``, ``pin``, ``bounds`` and ``params`` are theirs), scored as ``denoising_score`` scores
        them (``levels`` the S host levels, ``weights`` None or S values, ``score_noise`` (S, M, Ta, A) or None: ``draws`` rows per
        level drawn here, in antithetic pairs by default), and per observation the chunk of the largest score selected by
        ``gc_sampling.best_candidates``' rule.  The guidance weight, the pin and the bounds shape the sampling only: the score is
        that of the unguided, unpinned model.  Where the context does not depend on sigma the score reads the context the sampler
        encoded: the encoder runs once.  Returns (best (B, Ta, A), index (B,) int64, scores, chunks): ``chunks`` in ``action``'s
        shape, (B*K, Ta, A) or (B, K, Ta, A), ``scores`` in ``action.shape[:-2]``.  No read-back, no synchronisation; capturable
        after one eager call."""
        from ... import _lib
        im = self.inner_model
        K = candidate_count(candidates)
        Ta, A = action.shape[-2:]
        S = int(levels.numel()) if torch.is_tensor(levels) else len(levels)
        if score_noise is None:
            score_noise = draw_score_noise("sample_select", S, draws, antithetic, Ta, A, action.dtype, action.device)
        pin = _pin_rows(pin, action, K)
        bounds = _bounds_pair(bounds, action.device)
        best, index, scores, chunks, ctx = self._engine(state=state).sample_select(
            None if kind is None else _lib.SAMPLER_KIND[kind], _lib.sampler_params(**params), state, action, im._goals(goal, False),
            sigmas, levels, score_noise, K, weights=weights, noise=noise, n_steps=n_steps, cond_lambda=cond_lambda, bounds=bounds,
            pin=pin)
        im.latent_encoder_emb = ctx
        return best, index.long(), scores.reshape(action.shape[:-2]), chunks

    @torch.no_grad()
    def sample_dpm_adaptive_native(self, state, action, goal, sigma_min, sigma_max, cond_lambda=None, **params):
        """sample_dpm_adaptive with eta = 0 as one blocking call (mdt_sample_dpm_adaptive): ``params`` its keyword arguments
        (order, rtol, atol, h_init, pcoeff, icoeff, dcoeff, accept_safety).  Returns (action, info).  ``cond_lambda``:
        classifier-free guidance weight (mdt_sample_dpm_adaptive_guided)."""
        from ... import _lib
        im = self.inner_model
        out, ctx, info = self._engine(state=state).sample_dpm_adaptive(_lib.dpm_adaptive_params(**params), state, action,
                                                                       im._goals(goal, False), sigma_min, sigma_max,
                                                                       cond_lambda=cond_lambda)
        im.latent_encoder_emb = ctx
        return out, info

    @torch.no_grad()
    def sample_steered(self, state, action, goal, sigmas, steer, candidates=None, bounds=None, kind=None, noise=None, n_steps=None,
                       record=False, **params):
        """A steered sampler loop as one enqueue.  ``kind`` None: DDIM (mdt_sample_ddim_steer) -- what ``sample_ddim(...,
        steer=steer)`` runs, and with ``bounds`` -- an ``ActionBounds`` or a (lo, hi) pair, x clamped after every step -- what
        gc_sampling.sample_euler without churn runs under a clipping scaler (the same update).  ``kind`` a sampler name
        ('euler', 'heun', 'dpmpp_2m', ...: mdt_sample_steer): that sampler in ``sample_native``'s conventions -- ``noise`` None or
        (n_noise, B*K, Ta, A) in the Python loop's draw order, ``n_steps`` dpm_fast's evaluation count (``sigmas`` then
        [sigma_max, sigma_min]), ``params`` the sampler's keyword arguments, ``bounds`` applied where the kind's loop clips,
        ``record=True`` returning (actions, rec) with the dict ``gc_sampling.replay_callback`` takes, 'denoised' holding D'."""
        from ... import _lib
        im = self.inner_model
        bounds = _bounds_pair(bounds, action.device)
        K = candidate_count(candidates)
        if kind is None:
            if noise is not None or n_steps is not None or record or params:
                raise ValueError("sample_steered: noise, n_steps, record and sampler parameters need a sampler kind")
            out, ctx = self._engine(state=state).sample_ddim_steer(state, action, im._goals(goal, False), sigmas, steer,
                                                                   candidates=K, bounds=bounds)
        else:
            out, ctx, rec = self._engine(state=state).sample_steer(
                _lib.SAMPLER_KIND[kind], _lib.sampler_params(**params), state, action, im._goals(goal, False), sigmas, steer,
                noise=noise, n_steps=n_steps, candidates=K, bounds=bounds, record=record)
        im.latent_encoder_emb = ctx
        return (out, _record_dict(rec, kind, sigmas, n_steps, params)) if record else out

    @torch.no_grad()
    def sample_ddim(self, state, action, goal, sigmas, cond_lambda=None, bounds=None, record=False, pin=None, candidates=None,
                    steer=None):
        """Whole DDIM loop (reference gc_sampling.py:922-951) as one enqueue on the current stream.  ``cond_lambda``:
        classifier-free guidance weight (None or 1: the unguided call; mdt_sample_ddim_guided).  ``bounds`` is accepted and not
        read, as the reference's DDIM accepts a scaler and never clips; the DDIM head keeps no per-step record.  ``pin``: an
        ``ActionPin`` or its (known, keep) pair of (B, Ta, A) device tensors -- pinned actions (mdt_sample_ddim_opt): every step's
        denoised value becomes keep * known + (1 - keep) * D inside the action head.  ``candidates`` = K: K chunks per
        observation from one encoded context (mdt_sample_ddim_multi), with the shapes ``sample_native`` documents.  ``steer``: an
        ``ActionSteer`` (utils/action_steer.py) -- every step's denoised value becomes D + s(sigma) J^T (weight (known - D))
        (mdt_sample_ddim_steer: per step one taped decoder forward and one input-gradient-only backward; eager, never a graph);
        with ``cond_lambda`` != 1 or ``pin`` it raises NotImplementedError; a steer whose weight is all zero is no steer."""
        steer = take_steer({"steer": steer})[0]
        if steer is not None:
            steer_alone(cond_lambda=cond_lambda, pin=pin)
        if record:
            raise NotImplementedError("sample_ddim keeps no per-step record; run the host loop with a callback")
        if steer is not None:
            return self.sample_steered(state, action, goal, sigmas, steer, candidates=candidates)
        im = self.inner_model
        K = candidate_count(candidates)
        pin = _pin_rows(pin, action, K)
        out, ctx = self._engine(state=state).sample_ddim(state, action, im._goals(goal, False), sigmas, cond_lambda=cond_lambda,
                                                         pin=pin, candidates=K)
        im.latent_encoder_emb = ctx
        return out
