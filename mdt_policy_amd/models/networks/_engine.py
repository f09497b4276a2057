"""Bridge between the nn.Module facades and libmdt_hip.so.

``HipEngine`` owns one ``mdt_model`` handle (include/mdt_hip.h) for one score network on one GPU.  It keeps the
library's fragment-packed weight arena in sync with the module's ``nn.Parameter``s (re-uploading a parameter
when its storage pointer or in-place version counter changes, e.g. after ``load_state_dict`` / an EMA copy /
an optimizer step) and turns tensors into the raw device pointers + stream the C ABI takes.

``HipScoreNetwork`` is the shared base of ``MDTVTransformer`` / ``MDTTransformer`` (reference
mdt/models/networks/mdtv_transformer.py:35, mdt/models/networks/mdt_transformer.py:38).

There is no eager/CPU fallback here on purpose: a missing library, a CPU tensor, or an unsupported
configuration raises.
"""
from __future__ import annotations

import ctypes as C
import math
import operator
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn as nn

from ... import _lib
from ._handle import grad_layout


import os

_RESYNC_EVERY = int(os.environ.get("MDT_HIP_PARAM_RESYNC", "0") or 0)


def guidance(cond_lambda=None, **other):
    """The one reading of a guidance weight: ``guidance(**extra_args)`` for a sampler's ``extra_args``, ``guidance(cond_lambda)`` for
    a weight.  Returns (native, lam).  native is False when there is more than the weight: the host loop runs then, and hands
    the arguments to GCDenoiser.forward.  lam is the weight as the C ABI takes it, or None for the unguided call.  No weight and
    exactly 1 both give None: the conditional model's unguided call gives the same bits.  A weight that is not a finite number
    raises ValueError, before anything is enqueued."""
    if other:
        return False, None
    if cond_lambda is None:
        return True, None
    lam = float(cond_lambda)
    if not math.isfinite(lam):
        raise ValueError(f"cond_lambda must be finite, got {lam}")
    return True, (None if lam == 1.0 else lam)


def rollout_controls(cond_lambda=None, pin=None, **other):
    """``guidance`` for a sampler's ``extra_args`` that may also carry pinned actions (``pin``: an ActionPin,
    utils/action_pin.py): ``rollout_controls(**extra_args)`` returns (native, lam, pin).  The weight and the pin both ride inside
    the native call; any further key keeps the host loop, which hands all of them to GCDenoiser.forward.  ``extra_args`` reach
    ``forward`` too, which applies the pin through ``ActionPin.apply``: a bare (known, keep) pair (what ``sample_native(pin=)``
    also takes) is a TypeError here, before anything is enqueued."""
    if pin is not None and not (callable(getattr(pin, "on", None)) and callable(getattr(pin, "apply", None))):
        raise TypeError(f"extra_args['pin'] must be an ActionPin (ActionPin(known, keep)), got {type(pin).__name__}")
    native, lam = guidance(cond_lambda, **other)
    return native, lam, pin


def candidate_count(candidates=None) -> int:
    """The one reading of ``candidates``: action chunks per observation as an int >= 1 (None: 1).  Anything else raises ValueError,
    before anything is enqueued."""
    if candidates is None:
        return 1
    if isinstance(candidates, bool) or not isinstance(candidates, int) or candidates < 1:
        raise ValueError(f"candidates must be an int >= 1, got {candidates!r}")
    return candidates


def take_candidates(extra_args):
    """(K, the other keys) of a sampler's ``extra_args``: ``candidates`` comes off in front of ``rollout_controls`` and ``guidance``,
    which keep their signatures -- alone or with a weight and / or a pin it rides in the native call."""
    rest = dict(extra_args or {})
    return candidate_count(rest.pop("candidates", None)), rest


def take_steer(extra_args):
    """(steer, the other keys) of a sampler's ``extra_args``: ``steer`` (an ActionSteer, utils/action_steer.py) comes off in front
    of ``take_candidates`` and ``rollout_controls``.  A steer whose weight is all zero comes back as None -- it is treated as
    absent everywhere, so the call is the call without it.  Anything that is no ActionSteer is a TypeError, before anything is
    enqueued."""
    rest = dict(extra_args or {})
    steer = rest.pop("steer", None)
    if steer is None:
        return None, rest
    if not (callable(getattr(steer, "on", None)) and callable(getattr(steer, "scale", None)) and hasattr(steer, "active")):
        raise TypeError(f"extra_args['steer'] must be an ActionSteer (ActionSteer(known, weight, beta)), got {type(steer).__name__}")
    return (steer if steer.active else None), rest


def steer_alone(cond_lambda=None, pin=None):
    """What an active steer does not combine with yet: the Jacobian of the guided call's doubled batch, and the order of pin
    against steer.  Raises NotImplementedError naming the key."""
    if pin is not None:
        raise NotImplementedError("'steer' together with 'pin' is not implemented (the order of pin against steer is not defined yet)")
    if cond_lambda is not None and float(cond_lambda) != 1.0:
        raise NotImplementedError("'steer' together with 'cond_lambda' != 1 is not implemented (the Jacobian of the guided call's "
                                  "doubled batch is not formed)")


def chunk_rows(action: torch.Tensor, B: int, K: int) -> torch.Tensor:
    """``action`` of a call with K candidates for each of B observations, (B*K, Ta, A) or (B, K, Ta, A), as its (B*K, Ta, A)
    chunks (observation-major: chunk k of observation b is row b*K + k).  A leading size that is not B*K raises ValueError."""
    if action.dim() == 4:
        if tuple(action.shape[:2]) != (B, K):
            raise ValueError(f"action is {tuple(action.shape)}: {B} observations at candidates={K} take ({B}, {K}, Ta, A) "
                             f"or ({B * K}, Ta, A)")
        return action.reshape((B * K,) + tuple(action.shape[2:]))
    if action.shape[0] != B * K:
        raise ValueError(f"action holds {action.shape[0]} chunks, {B} observations at candidates={K} take {B * K}")
    return action


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def check_goal_rows(goal: torch.Tensor, goal_seq_len: int) -> None:
    """A goal holds goal_seq_len rows per sample: (B, goal_seq_len, goal_dim), or (B, goal_dim) where goal_seq_len is 1."""
    rows = goal.shape[1] if goal.dim() >= 3 else 1
    if goal_seq_len > 1 and rows != goal_seq_len:
        raise ValueError(f"goal has {rows} token(s) per sample, shape {tuple(goal.shape)}; this model was built with "
                         f"goal_seq_len={goal_seq_len} and takes (B,{goal_seq_len},goal_dim)")


class HipEngine:
    def __init__(self, module: nn.Module, cfg: _lib.MDTConfig, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError(
                "the MDT denoiser runs only on a ROCm GPU (hand-written gfx950 kernels); move the model with "
                ".to('cuda') -- there is no CPU execution path in mdt_policy_amd")
        self.lib = _lib.load()
        self.module = module
        self.device = device
        self.cfg = cfg
        handle = C.c_void_p()
        from ...utils import torch_allocator
        torch_allocator.install()  # workspace / tapes / scratch live in torch's caching allocator, not beside it
        with torch.cuda.device(device):
            _lib.check(self.lib.mdt_create(C.byref(cfg), C.byref(handle)))
        self.handle = handle
        n = self.lib.mdt_param_count(handle)
        self.expected = {self.lib.mdt_param_name(handle, i).decode(): self.lib.mdt_param_numel(handle, i)
                         for i in range(n)}
        self._uploaded: Dict[str, tuple] = {}
        self.ctx_generation = 0  # bumped by every call that rewrites the handle's cached context (encoder output, K|V, folds)
        self.sigma_in_context = not cfg.use_ada_conditioning  # sigma embedding is the first context token
        # goal_conditioned=False: MDTV keeps the goal rows (behind the state tokens), MDT has none
        # (and MDTV gives it up when the proprioceptive token takes that place, mdtv_transformer.py:291-294)
        self.proprio = bool(cfg.use_proprio)
        self.has_goal_token = not (cfg.no_goal_conditioning and (cfg.arch == 1 or self.proprio))
        self.goal_seq_len = int(cfg.goal_seq_len)  # goal rows per sample: the goal is (B, goal_seq_len, goal_dim)
        self.Te = int(self.sigma_in_context) + int(self.has_goal_token) * self.goal_seq_len + \
            (cfg.n_obs_token if cfg.arch == 0 else 2) + int(self.proprio)
        self.Ta, self.A, self.D = cfg.action_seq_len, cfg.action_dim, cfg.embed_dim

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self.lib.mdt_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def invalidate(self) -> None:
        """Forget what was uploaded: the next call re-uploads (and re-packs) every parameter.  For in-place weight
        updates the version counter does not see -- ``p.data.mul_()/copy_()``, apex / DeepSpeed multi-tensor kernels, any
        raw-pointer write other than this package's FusedAdamW / multi_tensor_ema (which bump the counter)."""
        self._uploaded.clear()
        self._fast = None

    def sync_params(self) -> None:
        """Upload every parameter whose storage or version changed since the last upload.  MDT_HIP_PARAM_RESYNC=N
        (debug safety net) additionally re-uploads everything every N-th call."""
        stream = self._stream()
        if _RESYNC_EVERY > 0:
            self._calls = getattr(self, "_calls", 0) + 1
            if self._calls % _RESYNC_EVERY == 0:
                self._uploaded.clear()
        # fast path (a rollout calls this ~1000 times a second with nothing changed): three C-level sweeps over the cached lists --
        # every parameter still the object its module holds, same version counters, same storage pointers -- instead of a Python
        # loop body per parameter (73 -> ~45 us per call of a 1.2 ms rollout step)
        fast = getattr(self, "_fast", None)
        if fast is not None and not self._dirty_fast():
            return
        seen = 0
        changed = []  # (key, source tensor, tag)
        # the parameters the library reads, resolved once per engine as (key, leaf name, owning module, parameter): walking the
        # module tree on every call was ~0.15 ms of host time.  A parameter REPLACED by assignment fails the identity check
        # below and the list is resolved again.
        plist = getattr(self, "_plist", None)
        if plist is None:
            plist = self._plist = []
            for n, p in self.module.named_parameters():
                if ("inner_model." + n) in self.expected:
                    owner = self.module.get_submodule(n.rsplit(".", 1)[0]) if "." in n else self.module
                    plist.append(("inner_model." + n, n.rsplit(".", 1)[-1], owner, p))
        uploaded = self._uploaded
        for key, leaf, owner, p in plist:
            if owner._parameters.get(leaf) is not p:
                self._plist = None
                return self.sync_params()
            seen += 1
            tag = (p.data_ptr(), p._version)
            name = key
            if uploaded.get(key) == tag:
                continue
            if p.device != self.device or p.dtype != torch.float32:
                raise RuntimeError(f"parameter {name} must be float32 on {self.device}, got {p.dtype} on {p.device}")
            src = p.detach()
            if not src.is_contiguous():
                src = src.contiguous()
            changed.append((key, src, tag))
        if changed:  # every changed parameter in ONE launch (a training step changes all of them)
            n = len(changed)
            names = (C.c_char_p * n)(*[k.encode() for k, _, _ in changed])
            srcs = (C.c_void_p * n)(*[t.data_ptr() for _, t, _ in changed])
            numels = (C.c_int64 * n)(*[t.numel() for _, t, _ in changed])
            _lib.check(self.lib.mdt_load_params(self.handle, n, names, srcs, numels, stream))
            for key, _, tag in changed:
                self._uploaded[key] = tag
            self._keep_src = [t for _, t, _ in changed]  # non-contiguous parameters were copied: keep those alive
        if seen != len(self.expected):
            have = {"inner_model." + n for n, _ in self.module.named_parameters()}
            raise RuntimeError(f"module lacks parameters the HIP path needs: {sorted(set(self.expected) - have)[:5]}")
        params = [p for _, _, _, p in plist]
        if all(self._uploaded.get(k) == (p.data_ptr(), p._version) for k, _, _, p in plist):
            self._fast = ([o._parameters for _, _, o, _ in plist], [l for _, l, _, _ in plist], params,
                          [p._version for p in params], [p.data_ptr() for p in params], plist)
        else:
            self._fast = None

    def _dirty_fast(self) -> bool:
        """True when the cached snapshot of sync_params no longer describes the module (or cannot tell)."""
        dicts, leafs, params, vers, ptrs, plist = self._fast
        if plist is not getattr(self, "_plist", None) or len(self._uploaded) < len(params):   # invalidate() / a re-resolved list
            self._fast = None
            return True
        try:
            same = all(map(operator.is_, [d[l] for d, l in zip(dicts, leafs)], params))
        except KeyError:
            same = False
        if same and [p._version for p in params] == vers and [p.data_ptr() for p in params] == ptrs:
            return False
        self._fast = None
        return True

    def _in(self, t: torch.Tensor, shape=None) -> torch.Tensor:
        if t.device != self.device:
            raise RuntimeError(f"input tensor on {t.device}, model on {self.device}")
        t = t.detach()
        if t.dtype != torch.float32:
            t = t.float()
        if shape is not None:
            t = t.reshape(shape)
        if not t.is_contiguous():
            t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
        return t

    def _tokens(self, state: dict):
        if self.cfg.arch == 0:
            tok = self._in(state["state_images"])
            if tok.dim() != 3 or tok.shape[1] != self.cfg.n_obs_token or tok.shape[2] != self.cfg.obs_dim:
                raise ValueError(f"state_images must be (B,{self.cfg.n_obs_token},{self.cfg.obs_dim}), got {tuple(tok.shape)}")
            # 'state_obs' in states (mdtv_transformer.py:262) selects the context layout: HipScoreNetwork.hip_engine
            # hands out the handle built for this state dict's layout
            if ("state_obs" in state) != self.proprio:
                raise RuntimeError("state dict and library handle disagree about the proprioceptive token; obtain the "
                                   "engine with hip_engine(state=state)")
            obs = None
            if self.proprio:
                obs = self._in(state["state_obs"])
                if obs.numel() != tok.shape[0] * self.cfg.proprio_dim:
                    raise ValueError(f"state_obs must be (B,1,{self.cfg.proprio_dim}), got {tuple(obs.shape)}")
            return tok, obs, tok.shape[0]
        st, gr = self._in(state["static"]), self._in(state["gripper"])
        B = st.shape[0]
        if st.numel() != B * self.cfg.obs_dim or gr.numel() != B * self.cfg.obs_dim:
            raise ValueError("static / gripper must be (B,1,obs_dim)")
        return st, gr, B

    def _goal(self, goal: torch.Tensor, B: int) -> torch.Tensor:
        G = self.goal_seq_len
        check_goal_rows(goal, G)
        g = self._in(goal)
        if g.numel() != B * G * self.cfg.goal_dim:
            raise ValueError(f"goal must hold (B,{G},{self.cfg.goal_dim}) values, got {tuple(goal.shape)}")
        return g

    def _modality(self, state: dict) -> int:
        return _lib.MODALITY["lang"] if state.get("modality", None) == "lang" else _lib.MODALITY["vis"]

    # ------------------------------------------------------------------------------------------
    def encode(self, state: dict, goal: torch.Tensor, honour_modality: bool,
               sigma: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``sigma`` is only read by use_ada_conditioning=False models (it is their first context token)."""
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        g = self._goal(goal, B)
        s = None
        if self.sigma_in_context:
            if sigma is None:
                raise ValueError("use_ada_conditioning=False: the encoder needs sigma (its first context token)")
            s = self._in(sigma.reshape(-1).expand(B) if sigma.numel() == 1 else sigma, (B,))
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_encode, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state),
                                       int(honour_modality), _ptr(s), B, _ptr(ctx), self._stream())
        return ctx

    def denoise_cached(self, x: torch.Tensor, sigma: torch.Tensor, flags: int = 0) -> torch.Tensor:
        x_ = self._in(x)
        B = x_.shape[0]
        if sigma.numel() == 1 and B > 1:  # one noise level for the whole batch (every sampler): broadcast in-kernel
            s = self._in(sigma, (1,))
            flags |= _lib.SIGMA_SCALAR
        else:
            s = self._in(sigma, (B,))
        out = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        _lib.call(self.lib.mdt_denoise_cached, self.handle, _ptr(x_), _ptr(s), B, flags, _ptr(out), self._stream())
        return out

    def forward(self, state: dict, x: torch.Tensor, goal: torch.Tensor, sigma: torch.Tensor):
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        if sigma.numel() == 1 and B > 1:
            sigma = sigma.reshape(1).expand(B)
        g, x_, s = self._goal(goal, B), self._in(x, (B, self.Ta, self.A)), self._in(sigma, (B,))
        out = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_forward, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state), _ptr(x_),
                                        _ptr(s), B, _ptr(out), _ptr(ctx), self._stream())
        return out, ctx

    # -- the sampler calls: one path to C.  mdt_sample_opt / mdt_sample_ddim_opt (and their _dev forms) state every other entry --
    def _sampler_inputs(self, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas=None, n_steps: Optional[int] = None,
                        noise: Optional[torch.Tensor] = None, candidates: int = 1):
        """What every sampler call starts from, once: the parameters in sync, the inputs as the C ABI takes them (tok, tok2, g,
        x, and nz: ``noise`` as (n_noise, B, Ta, A) or None), the outputs (out, ctx) and the schedule -- sig, its C argument
        sig_arg, dev (on the device: read in place, no copy to the host, no synchronisation) and n (one less than the levels, or
        ``n_steps``).  ``candidates`` = K: p.B observations, p.K and p.N = B*K chunks -- x, nz and out are per chunk (out in the
        shape x_T came in, (B*K, Ta, A) or (B, K, Ta, A)), tok, tok2, g and ctx per observation.  The caller holds the result until its C call has returned: a converted input lives nowhere else, and
        what the enqueued kernels read must not go back to the allocator before they are enqueued.  Bumps ctx_generation."""
        self.sync_params()
        p = SimpleNamespace(modality=self._modality(state), sig=None, sig_arg=None, dev=False, n=None)
        p.tok, p.tok2, p.B = self._tokens(state)
        p.K = candidate_count(candidates)
        p.N = p.B * p.K
        if p.K != 1 or x_T.dim() == 4:
            chunk_rows(x_T, p.B, p.K)
        p.g, p.x = self._goal(goal, p.B), self._in(x_T, (p.N, self.Ta, self.A))
        p.nz = None if noise is None else self._in(noise, (-1, p.N, self.Ta, self.A))
        p.out = torch.empty((p.B, p.K, self.Ta, self.A) if x_T.dim() == 4 else (p.N, self.Ta, self.A), device=self.device,
                            dtype=torch.float32)
        p.ctx = torch.empty((p.B, self.Te, self.D), device=self.device, dtype=torch.float32)
        if sigmas is not None:
            p.dev = torch.is_tensor(sigmas) and sigmas.device.type == "cuda"
            if p.dev:
                p.sig = self._in(sigmas.reshape(-1))
                levels, p.sig_arg = p.sig.numel(), p.sig.data_ptr()
            else:
                vals = [float(v) for v in (sigmas.detach().tolist() if torch.is_tensor(sigmas) else sigmas)]
                levels = len(vals)
                p.sig = p.sig_arg = (C.c_float * levels)(*vals)
            p.n = levels - 1 if n_steps is None else int(n_steps)
        self.ctx_generation += 1
        return p

    def _chunks(self, x_T: torch.Tensor) -> int:
        return x_T.numel() // (self.Ta * self.A)

    def _opts(self, B: int, cond_lambda=None, bounds=None, record=None, tree=None, pin=None, candidates: int = 1):
        """mdt_sample_opts of a call as (the C argument, what it points to).  Nothing asked for: (None, ()), the entries' NULL --
        the plain call, and no struct is built for it.  ``bounds`` (lo, hi): fp32 (A,) tensors on the device; ``record``: the
        (steps, 2, B, Ta, A) tensor to fill; ``tree``: (seeds, tol, lo, hi); ``pin``: (known, keep), fp32 (B, Ta, A) on the device.  ``B`` counts chunks; with
        ``candidates`` = K > 1 a pin of (B / K, Ta, A) is per observation and goes to each of its K chunks."""
        lam = guidance(cond_lambda)[1]
        if lam is None and bounds is None and record is None and tree is None and pin is None:
            return None, ()
        lo = hi = src = seeds = known = keep = None
        if pin is not None:
            known, keep = self._pin(pin, B, candidates)
        if bounds is not None:
            lo, hi = (self._in(b, (self.A,)) for b in bounds)
        if tree is not None:
            seeds = tree[0]
            if seeds.device != self.device or seeds.dtype != torch.int64 or not seeds.is_contiguous():
                raise ValueError("sample_native: seeds must be a contiguous int64 tensor on the model's device")
            src = _lib.BrownianSource(seeds.data_ptr(), int(seeds.numel()), 0, float(tree[2]), float(tree[3]), float(tree[1]))
        opts = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0 if lam is None else lam, _ptr(lo), _ptr(hi), _ptr(record),
                               None if src is None else C.pointer(src), _ptr(known), _ptr(keep))
        return C.byref(opts), (opts, lo, hi, src, seeds, known, keep)

    def _pin(self, pin, B: int, candidates: int = 1):
        """A pin's (known, keep) as the C ABI takes them: contiguous fp32 (B, Ta, A) on the device (a float's alignment will do)."""
        out = []
        for t in pin:
            if t.device != self.device:
                raise RuntimeError(f"pin tensor on {t.device}, model on {self.device}")
            if candidates > 1 and tuple(t.shape) == (B // candidates, candidates, self.Ta, self.A):
                t = t.reshape(B, self.Ta, self.A)
            elif candidates > 1 and tuple(t.shape) == (B // candidates, self.Ta, self.A):
                t = t.repeat_interleave(candidates, 0)  # per observation: the same pin for each of its chunks
            if tuple(t.shape) != (B, self.Ta, self.A):
                raise ValueError(f"pin tensors must be ({B},{self.Ta},{self.A}), got {tuple(t.shape)}")
            t = t.detach()
            out.append(t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous())
        return tuple(out)

    def sample_ddim(self, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas, cond_lambda: Optional[float] = None,
                    pin=None, candidates: int = 1):
        """Fused sampler call (mdt_sample_ddim_opt / mdt_sample_ddim_dev_opt; ``candidates`` = K > 1: mdt_sample_ddim_multi /
        _dev_multi -- K chunks per observation from one encoded context, x_T (B*K, Ta, A) or (B, K, Ta, A)).  ``sigmas`` may live on the host (gc_sampling's
        default) or on the model's device -- the agent builds its schedule there (mdtv_agent.py:660-667); a device schedule is
        consumed in place: no copy to the host, no synchronisation.  ``cond_lambda`` (not None or 1): classifier-free guidance.
        ``pin``: None or (known, keep), fp32 (B, Ta, A) tensors on the device, read when the kernels run -- pinned actions.
        Without either the call passes no options: the plain mdt_sample_ddim call."""
        K = candidate_count(candidates)
        opts, held = self._opts(self._chunks(x_T), cond_lambda, pin=pin, candidates=K)
        p = self._sampler_inputs(state, x_T, goal, sigmas, candidates=K)
        self._keep = (p.sig, None) + held  # the kernels that read them are only enqueued
        head = (self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x), p.sig_arg, p.n, p.B)
        tail = (_ptr(p.out), _ptr(p.ctx), opts, self._stream())
        if K == 1:
            _lib.call(self.lib.mdt_sample_ddim_dev_opt if p.dev else self.lib.mdt_sample_ddim_opt, *head, *tail)
        else:
            _lib.call(self.lib.mdt_sample_ddim_dev_multi if p.dev else self.lib.mdt_sample_ddim_multi, *head, K, *tail)
        return p.out, p.ctx

    def _steered_inputs(self, state: dict, x_T, goal, sigmas, steer, bounds, n_steps=None, noise=None, candidates: int = 1):
        """What both steered calls start from: the tapes prepared, the schedule on the host, ``_sampler_inputs`` on it, the steer
        per chunk, the bounds as fp32 (A,) device tensors or None.  Holds what the enqueued kernels read in ``_keep``."""
        self.train_prepare()
        host = sigmas.detach().to("cpu") if torch.is_tensor(sigmas) else sigmas
        p = self._sampler_inputs(state, x_T, goal, host, n_steps, noise, candidates=candidate_count(candidates))
        known, weight = steer.on(self.device, (p.N, self.Ta, self.A), p.K)
        lo, hi = (None, None) if bounds is None else (self._in(b, (self.A,)) for b in bounds)
        self._keep = (p.sig, p.nz, known, weight, lo, hi)  # the kernels that read them are only enqueued
        return p, host, known, weight, lo, hi

    def sample_ddim_steer(self, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas, steer, candidates: int = 1, bounds=None):
        """mdt_sample_ddim_steer: DDIM with every step's denoised value steered through the denoiser's Jacobian, D' = D + s(sigma)
        J^T (weight (known - D)), as one enqueue -- the observations encoded once, per step one taped decoder forward on the B*K
        chunks and one input-gradient-only backward.  ``steer``: an ActionSteer, per chunk or per observation; ``x_T``
        (B*K, Ta, A) or (B, K, Ta, A); ``bounds``: None or (lo, hi), fp32 (A,) device tensors -- x is clamped after every step
        (sample_euler's clip; sample_ddim passes none).  The schedule goes to the host (a device schedule is read back).  Not
        capture-safe: on a capturing stream the library refuses with MDT_ERR_STATE and enqueues nothing."""
        p, _, known, weight, lo, hi = self._steered_inputs(state, x_T, goal, sigmas, steer, bounds, candidates=candidates)
        _lib.call(self.lib.mdt_sample_ddim_steer, self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x),
                  C.cast(p.sig, C.c_void_p), p.n, p.B, p.K, _ptr(known), _ptr(weight), float(steer.beta), _ptr(lo), _ptr(hi),
                  _ptr(p.out), _ptr(p.ctx), self._stream())
        return p.out, p.ctx

    def sample_steer(self, kind: int, params, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas, steer,
                     noise: Optional[torch.Tensor] = None, n_steps: Optional[int] = None, candidates: int = 1, bounds=None,
                     record: bool = False):
        """mdt_sample_steer: ``sample_native``'s sampler (``kind`` an mdt_sampler_kind, ``params`` an _lib.SamplerParams, ``noise``
        None or (n_noise, B*K, Ta, A) in the Python loop's draw order, ``n_steps`` None or dpm_fast's evaluation count) with every
        evaluation's denoised value steered as ``sample_ddim_steer`` steers DDIM's, as one enqueue.  ``bounds``: None or (lo, hi),
        fp32 (A,) device tensors, applied where the kind's loop clips; ``record``: the call also fills the (steps, 2, B*K, Ta, A)
        record, [i][1] holding D'.  The schedule goes to the host (a device schedule is read back).  Returns (out, ctx, record or
        None).  Not capture-safe: on a capturing stream the library refuses with MDT_ERR_STATE and enqueues nothing."""
        p, host, known, weight, lo, hi = self._steered_inputs(state, x_T, goal, sigmas, steer, bounds, n_steps, noise, candidates)
        rec = None
        if record:
            steps = len(host) - 1 if n_steps is None else int(n_steps) // 3 + 1  # n_steps: dpm_fast's evaluation count
            rec = torch.empty((steps, 2) + tuple(p.out.shape), device=self.device, dtype=torch.float32)
        _lib.call(self.lib.mdt_sample_steer, self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x), int(kind),
                  C.byref(params), p.sig_arg, p.n, _ptr(p.nz), 0 if p.nz is None else p.nz.shape[0], p.B, p.K, _ptr(known),
                  _ptr(weight), float(steer.beta), _ptr(lo), _ptr(hi), _ptr(rec), _ptr(p.out), _ptr(p.ctx), self._stream())
        return p.out, p.ctx, rec

    def sample_native(self, kind: int, params, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas,
                      noise: Optional[torch.Tensor] = None, n_steps: Optional[int] = None, cond_lambda: Optional[float] = None,
                      tree=None, bounds=None, record: bool = False, pin=None, candidates: int = 1):
        """One call of another sampler (mdt_sample_opt / mdt_sample_dev_opt; ``candidates`` = K > 1: mdt_sample_multi / _dev_multi,
        where x_T, the noise rows, the pin, the record and the tree's seeds are per chunk, B*K of them): ``kind`` an mdt_sampler_kind, ``params`` an
        _lib.SamplerParams, ``noise`` None or (n_noise, B, Ta, A) in the Python loop's draw order, ``n_steps`` None (one less
        than the levels) or dpm_fast's evaluation count.  Like sample_ddim, a device schedule is read in place (no copy, no
        synchronisation).  ``cond_lambda`` (not None or 1): classifier-free guidance.  ``tree``: None or (seeds, tol, lo, hi) --
        dpmpp_sde with Brownian-tree noise drawn inside the call: ``seeds`` an int64 tensor of 1 or B keys on the device, ``tol``
        the tree's resolution, ``lo`` < ``hi`` its interval (0, 0: the schedule's smallest positive and largest level).
        ``bounds``: None or (lo, hi), fp32 (A,) tensors on the device, read when the kernels run (a captured call reads what they
        hold at replay); ``record``: the call also fills the (steps, 2, B, Ta, A) record -- [i][0] the input of step i's first
        evaluation, [i][1] its denoised output; ``pin``: None or (known, keep), fp32 (B, Ta, A) tensors on the device, read when
        the kernels run -- the denoised value of every evaluation becomes keep * known + (1 - keep) * D (the record then holds
        that).  Returns (out, ctx, record or None).  Capture-safe."""
        rec = None
        if record:
            steps = len(sigmas) - 1 if n_steps is None else int(n_steps) // 3 + 1  # n_steps: dpm_fast's evaluation count
            rec = torch.empty((steps, 2) + tuple(x_T.shape[:-2]) + (self.Ta, self.A), device=self.device, dtype=torch.float32)
        K = candidate_count(candidates)
        opts, held = self._opts(self._chunks(x_T), cond_lambda, bounds, rec, tree, pin, candidates=K)
        p = self._sampler_inputs(state, x_T, goal, sigmas, n_steps, noise, candidates=K)
        self._keep = (p.sig, p.nz) + held  # the kernels that read them are only enqueued
        head = (self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x), int(kind), C.byref(params), p.sig_arg, p.n,
                _ptr(p.nz), 0 if p.nz is None else p.nz.shape[0], p.B)
        tail = (_ptr(p.out), _ptr(p.ctx), opts, self._stream())
        if K == 1:
            _lib.call(self.lib.mdt_sample_dev_opt if p.dev else self.lib.mdt_sample_opt, *head, *tail)
        else:
            _lib.call(self.lib.mdt_sample_dev_multi if p.dev else self.lib.mdt_sample_multi, *head, K, *tail)
        return p.out, p.ctx, rec

    def sample_dpm_adaptive(self, params, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigma_min: float, sigma_max: float,
                            cond_lambda: Optional[float] = None):
        """mdt_sample_dpm_adaptive (eta = 0): ``params`` an _lib.DpmAdaptiveParams.  Blocking: the call reads the step error
        back every step.  Returns (out, ctx, info dict).  ``cond_lambda`` (not None or 1): mdt_sample_dpm_adaptive_guided."""
        lam = guidance(cond_lambda)[1]
        info = _lib.DpmAdaptiveInfo()
        p = self._sampler_inputs(state, x_T, goal)
        args = (self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x), float(sigma_min), float(sigma_max),
                C.byref(params), p.B, _ptr(p.out), _ptr(p.ctx))
        if lam is None:
            _lib.call(self.lib.mdt_sample_dpm_adaptive, *args, C.byref(info), self._stream())
        else:
            _lib.call(self.lib.mdt_sample_dpm_adaptive_guided, *args, lam, C.byref(info), self._stream())
        return p.out, p.ctx, {k: int(getattr(info, k)) for k in ("steps", "nfe", "n_accept", "n_reject")}

    def loss_fwd(self, state: dict, action: torch.Tensor, goal: torch.Tensor, noise: torch.Tensor, sigma: torch.Tensor):
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        g = self._goal(goal, B)
        a, nz = self._in(action, (B, self.Ta, self.A)), self._in(noise, (B, self.Ta, self.A))
        s = self._in(sigma, (B,))
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        mo = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_loss_fwd, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state), _ptr(a),
                                         _ptr(nz), _ptr(s), B, _ptr(loss), _ptr(mo), _ptr(ctx), self._stream())
        return loss, mo, ctx

    def reserve(self, max_batch: int) -> None:
        _lib.call(self.lib.mdt_reserve, self.handle, int(max_batch))

    # -- training path (include/mdt_hip_train.h) ----------------------------------------------------
    def train_prepare(self) -> None:
        """Allocate the transposed weight images and learn the gradient layout (idempotent)."""
        if getattr(self, "_grad_layout", None) is not None:
            return
        with torch.cuda.device(self.device):
            _lib.call(self.lib.mdt_train_prepare, self.handle)
        self._uploaded.clear()  # every parameter is re-uploaded so that its transposed image exists
        self._grad_layout, self._grad_numel = grad_layout(self.lib, "mdt", self.handle)
        n = self.lib.mdt_param_count(self.handle)
        # the stage of the staged backward (mdt_train_loss_bwd_stage) that completes each parameter's gradient
        self._n_stages = int(self.lib.mdt_train_loss_bwd_stages(self.handle))
        self._param_stage = {self.lib.mdt_param_name(self.handle, i).decode(): int(self.lib.mdt_train_param_stage(self.handle, i))
                             for i in range(n)}
        self.stages_enqueued = 0  # stages of staged backwards enqueued so far (tests read it from DDP communication hooks)

    def train_loss_fwd(self, state: dict, tok, tok2, goal, action, noise, sigma, drop=None):
        self.train_prepare()
        self.sync_params()
        B = tok.shape[0]
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        mo = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        tape = C.c_int32(-1)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_train_loss_fwd, self.handle, _ptr(tok), _ptr(tok2), _ptr(goal), self._modality(state),
                                               _ptr(action), _ptr(noise), _ptr(sigma), B,
                                               None if drop is None else C.byref(drop), _ptr(loss), _ptr(mo), _ptr(ctx),
                                               C.byref(tape), self._stream())
        return loss, mo, ctx, int(tape.value)

    def train_encode_fwd(self, state: dict, tok, tok2, goal, honour_modality: bool, drop=None, sigma=None):
        self.train_prepare()
        self.sync_params()
        B = tok.shape[0]
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        tape = C.c_int32(-1)
        if self.sigma_in_context and sigma is None:
            raise ValueError("use_ada_conditioning=False: sigma is a context token and must be given")
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_train_encode_fwd, self.handle, _ptr(tok), _ptr(tok2), _ptr(goal), self._modality(state),
                                                 int(honour_modality), _ptr(sigma) if self.sigma_in_context else None, B,
                                                 None if drop is None else C.byref(drop), _ptr(ctx), C.byref(tape),
                                                 self._stream())
        return ctx, int(tape.value)

    def _input_grads(self, tok, tok2, goal, needs):
        d_tok = torch.empty_like(tok) if needs[0] else None
        d_tok2 = torch.empty_like(tok2) if (needs[1] and tok2 is not None) else None
        d_goal = torch.empty_like(goal) if needs[2] else None
        return d_tok, d_tok2, d_goal

    def train_loss_bwd(self, tape: int, g_loss, g_ctx, tok, tok2, goal, needs):
        grads = torch.zeros(self._grad_numel, device=self.device, dtype=torch.float32)
        d_tok, d_tok2, d_goal = self._input_grads(tok, tok2, goal, needs)
        gl = None if g_loss is None else self._in(g_loss, ())
        gc = None if g_ctx is None else self._in(g_ctx)
        _lib.call(self.lib.mdt_train_loss_bwd, self.handle, tape, _ptr(gl), _ptr(gc), _ptr(grads), _ptr(d_tok),
                                               _ptr(d_tok2), _ptr(d_goal), self._stream())
        return grads, d_tok, d_tok2, d_goal

    def train_loss_bwd_begin(self, g_loss, g_ctx, tok, tok2, goal, needs):
        """Buffers of one staged backward: (flat gradient buffer, input gradients, argument tuple of every stage call)."""
        grads = torch.zeros(self._grad_numel, device=self.device, dtype=torch.float32)
        d_tok, d_tok2, d_goal = self._input_grads(tok, tok2, goal, needs)
        gl = None if g_loss is None else self._in(g_loss, ())
        gc = None if g_ctx is None else self._in(g_ctx)
        return grads, (d_tok, d_tok2, d_goal), (gl, gc)

    def train_loss_bwd_stage(self, tape: int, stage: int, grads, dins, gs) -> None:
        """Enqueue stage `stage`; behind it (stream order) the gradients of the parameters of that stage are complete."""
        _lib.call(self.lib.mdt_train_loss_bwd_stage, self.handle, tape, int(stage), _ptr(gs[0]), _ptr(gs[1]), _ptr(grads),
                                                     _ptr(dins[0]), _ptr(dins[1]), _ptr(dins[2]), self._stream())
        self.stages_enqueued += 1

    def train_encode_bwd(self, tape: int, g_ctx, tok, tok2, goal, needs):
        grads = torch.zeros(self._grad_numel, device=self.device, dtype=torch.float32)
        d_tok, d_tok2, d_goal = self._input_grads(tok, tok2, goal, needs)
        gc = self._in(g_ctx)
        _lib.call(self.lib.mdt_train_encode_bwd, self.handle, tape, _ptr(gc), _ptr(grads), _ptr(d_tok), _ptr(d_tok2),
                                                 _ptr(d_goal), self._stream())
        return grads, d_tok, d_tok2, d_goal

    def decoder_side(self, name: str) -> bool:
        """Whether the decoder half (mdt_train_denoise_fwd) reads parameter ``name`` (module-relative): the action embedding and
        head, the decoder blocks, and the sigma embedding where sigma conditions the decoder -- as a context token it is the
        encoder's."""
        return name.startswith(("decoder.", "action_pred.", "action_emb.")) or \
            (name.startswith("sigma_emb.") and not self.sigma_in_context)

    def train_denoise_fwd(self, ctx: torch.Tensor, x: torch.Tensor, sigma: torch.Tensor, drop=None):
        """D(x; sigma) against the context tensor ``ctx`` with a tape (mdt_train_denoise_fwd); inputs as ``_in`` leaves them."""
        self.train_prepare()
        self.sync_params()
        B = x.shape[0]
        if tuple(ctx.shape) != (B, self.Te, self.D):
            raise ValueError(f"context must be ({B},{self.Te},{self.D}), got {tuple(ctx.shape)}")
        out = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        tape = C.c_int32(-1)  # (the call writes its tape only: the handle's cached context, and ctx_generation, stay)
        _lib.call(self.lib.mdt_train_denoise_fwd, self.handle, _ptr(ctx), _ptr(x), _ptr(sigma), B,
                                                  None if drop is None else C.byref(drop), _ptr(out), C.byref(tape), self._stream())
        return out, int(tape.value)

    def train_denoise_bwd(self, tape: int, g: torch.Tensor, B: int, needs, want_params: bool):
        """mdt_train_denoise_bwd: (flat gradient buffer or None, d_ctx, d_x, d_sigma), each None unless ``needs`` asks for it."""
        grads = torch.zeros(self._grad_numel, device=self.device, dtype=torch.float32) if want_params else None
        d_ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32) if needs[0] else None
        d_x = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32) if needs[1] else None
        d_sigma = torch.empty((B,), device=self.device, dtype=torch.float32) if needs[2] else None
        g_ = self._in(g, (B, self.Ta, self.A))
        _lib.call(self.lib.mdt_train_denoise_bwd, self.handle, tape, _ptr(g_), _ptr(grads), _ptr(d_ctx), _ptr(d_x), _ptr(d_sigma),
                                                  self._stream())
        return grads, d_ctx, d_x, d_sigma

    def denoise_vjp(self, state: dict, x: torch.Tensor, goal: torch.Tensor, sigma: torch.Tensor, v: torch.Tensor):
        """(D(x; sigma), (dD/dx)^T v): the eval-mode denoiser and its vector-Jacobian product w.r.t. the noisy actions
        (mdt_denoise_vjp: a tape-keeping forward plus an input-gradient-only backward)."""
        self.train_prepare()
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        g = self._goal(goal, B)
        x_, v_ = self._in(x, (B, self.Ta, self.A)), self._in(v, (B, self.Ta, self.A))
        s = self._in(sigma.reshape(-1).expand(B) if sigma.numel() == 1 else sigma, (B,))
        den = torch.empty((B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        vjp = torch.empty_like(den)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_denoise_vjp, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state), _ptr(x_),
                                            _ptr(s), _ptr(v_), B, _ptr(den), _ptr(vjp), self._stream())
        return den, vjp

    def log_likelihood(self, state: dict, x: torch.Tensor, goal: torch.Tensor, v: torch.Tensor, sigma_min: float, sigma_max: float,
                       candidates: int = 1, rtol: float = 1e-4, atol: float = 1e-4, max_steps: int = 10000):
        """mdt_log_likelihood: gc_sampling.log_likelihood's probability-flow integration as one blocking call.  ``state`` and
        ``goal`` carry B observations, ``x`` the B*K chunks as (B*K, Ta, A) or (B, K, Ta, A) (chunk k of observation b at row
        b*K + k), ``v`` the probe tensors (P, B*K, Ta, A).  Returns (ll (B*K,), latent (B*K, Ta, A), delta (B*K,), info dict)."""
        self.train_prepare()
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        K = candidate_count(candidates)
        R = B * K
        chunk_rows(x, B, K)
        g = self._goal(goal, B)
        x_ = self._in(x, (R, self.Ta, self.A))
        if v.dim() < 1 or v.numel() == 0 or v.numel() % x_.numel():
            raise ValueError(f"probes hold {v.numel()} values, {R} chunks take (P, {R}, {self.Ta}, {self.A})")
        v_ = self._in(v, (-1, R, self.Ta, self.A))
        params = _lib.loglik_params(probes=v_.shape[0], rtol=rtol, atol=atol, max_steps=max_steps)
        ll = torch.empty((R,), device=self.device, dtype=torch.float32)
        latent = torch.empty((R, self.Ta, self.A), device=self.device, dtype=torch.float32)
        delta = torch.empty((R,), device=self.device, dtype=torch.float32)
        info = _lib.LoglikInfo()
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_log_likelihood, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state), _ptr(x_), _ptr(v_),
                                               float(sigma_min), float(sigma_max), B, K, C.byref(params), _ptr(ll), _ptr(latent),
                                               _ptr(delta), C.byref(info), self._stream())
        return ll, latent, delta, {k: int(getattr(info, k)) for k in ("fevals", "steps", "n_accept", "n_reject")}

    def denoising_score(self, state: dict, x: torch.Tensor, goal: torch.Tensor, sigmas, noise: torch.Tensor, weights=None,
                        candidates: int = 1):
        """mdt_denoising_score: the B*K chunks ``x`` -- (B*K, Ta, A) or (B, K, Ta, A) -- scored by their weighted denoising error
        over the S host levels ``sigmas`` with the noise rows ``noise`` (S, M, Ta, A), as one enqueue on the current stream: no
        tape, no read-back, capturable once the workspace holds B*K*S*M rows.  ``weights``: None (trapezoid in ln sigma) or S
        host values.  Returns (score (B*K,), the observations' context (B, Te, D))."""
        self.sync_params()
        tok, tok2, B = self._tokens(state)
        K = candidate_count(candidates)
        R = B * K
        if K != 1 or x.dim() == 4:
            chunk_rows(x, B, K)
        g = self._goal(goal, B)
        x_ = self._in(x, (R, self.Ta, self.A))
        levels = [float(v) for v in (sigmas.detach().reshape(-1).tolist() if torch.is_tensor(sigmas) else sigmas)]
        S = len(levels)
        if noise.dim() != 4 or noise.shape[0] != S or tuple(noise.shape[2:]) != (self.Ta, self.A):
            raise ValueError(f"noise is {tuple(noise.shape)}: {S} levels take ({S}, draws, {self.Ta}, {self.A})")
        nz = self._in(noise)
        sig = (C.c_float * max(S, 1))(*levels)
        w = None
        if weights is not None:
            wl = [float(v) for v in (weights.detach().reshape(-1).tolist() if torch.is_tensor(weights) else weights)]
            if len(wl) != S:
                raise ValueError(f"weights hold {len(wl)} values, {S} levels take {S}")
            w = (C.c_float * max(S, 1))(*wl)
        score = torch.empty((R,), device=self.device, dtype=torch.float32)
        ctx = torch.empty((B, self.Te, self.D), device=self.device, dtype=torch.float32)
        self.ctx_generation += 1
        _lib.call(self.lib.mdt_denoising_score, self.handle, _ptr(tok), _ptr(tok2), _ptr(g), self._modality(state), _ptr(x_), sig, w, S,
                                                _ptr(nz), int(nz.shape[1]), B, K, _ptr(score), _ptr(ctx), self._stream())
        self._keep = (tok, tok2, g, x_, nz)  # the kernels that read them are only enqueued
        return score, ctx

    def sample_select(self, kind: Optional[int], params, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas, levels,
                      score_noise: torch.Tensor, candidates: int, weights=None, noise: Optional[torch.Tensor] = None,
                      n_steps: Optional[int] = None, cond_lambda: Optional[float] = None, bounds=None, pin=None):
        """mdt_sample_ddim_select / _dev_select (``kind`` None) or mdt_sample_select / _dev_select (``kind`` an mdt_sampler_kind,
        ``params`` an _lib.SamplerParams): ``sample_ddim`` / ``sample_native`` with ``candidates`` = K chunks per observation, the
        chunks scored as ``denoising_score`` scores them -- ``levels`` the S host levels, ``score_noise`` (S, M, Ta, A), ``weights``
        None or S host values -- and the best of each observation selected, as ONE enqueue.  The other arguments are the sampler's.
        Returns (best (B, Ta, A), index (B,) int32, scores (B*K,), chunks in the shape x_T came in, ctx).  Capture-safe once the
        workspace holds max(the sampler's samples, B*K*S*M)."""
        K = candidate_count(candidates)
        opts, held = self._opts(self._chunks(x_T), cond_lambda, bounds, None, None, pin, candidates=K)
        p = self._sampler_inputs(state, x_T, goal, sigmas, n_steps, noise, candidates=K)
        lv = [float(v) for v in (levels.detach().reshape(-1).tolist() if torch.is_tensor(levels) else levels)]
        S = len(lv)
        if score_noise.dim() != 4 or score_noise.shape[0] != S or tuple(score_noise.shape[2:]) != (self.Ta, self.A):
            raise ValueError(f"score noise is {tuple(score_noise.shape)}: {S} levels take ({S}, draws, {self.Ta}, {self.A})")
        snz = self._in(score_noise)
        sig = (C.c_float * max(S, 1))(*lv)
        w = None
        if weights is not None:
            wl = [float(v) for v in (weights.detach().reshape(-1).tolist() if torch.is_tensor(weights) else weights)]
            if len(wl) != S:
                raise ValueError(f"weights hold {len(wl)} values, {S} levels take {S}")
            w = (C.c_float * max(S, 1))(*wl)
        best = torch.empty((p.B, self.Ta, self.A), device=self.device, dtype=torch.float32)
        scores = torch.empty((p.N,), device=self.device, dtype=torch.float32)
        index = torch.empty((p.B,), device=self.device, dtype=torch.int32)
        spec = _lib.SelectSpec(C.sizeof(_lib.SelectSpec), sig, w, S, _ptr(snz), int(snz.shape[1]), _ptr(p.out), _ptr(scores),
                               _ptr(index))
        self._keep = (p.sig, p.nz, snz) + held  # the kernels that read them are only enqueued
        tail = (p.B, K, _ptr(best), _ptr(p.ctx), opts, C.byref(spec), self._stream())
        head = (self.handle, _ptr(p.tok), _ptr(p.tok2), _ptr(p.g), p.modality, _ptr(p.x))
        if kind is None:
            _lib.call(self.lib.mdt_sample_ddim_dev_select if p.dev else self.lib.mdt_sample_ddim_select, *head, p.sig_arg, p.n, *tail)
        else:
            _lib.call(self.lib.mdt_sample_dev_select if p.dev else self.lib.mdt_sample_select, *head, int(kind), C.byref(params),
                      p.sig_arg, p.n, _ptr(p.nz), 0 if p.nz is None else p.nz.shape[0], *tail)
        return best, index, scores, p.out, p.ctx

    def tape_release(self, tape: int) -> None:
        _lib.check(self.lib.mdt_tape_release(self.handle, tape))

    def unused_goal_embedder(self, state: dict, honour_modality: bool) -> Optional[str]:
        """Name prefix(es) of the goal embedder(s) this forward did NOT go through (None: all were used)."""
        if not self.has_goal_token:
            return ("goal_emb.", "lang_emb.")
        if not self.cfg.use_modality_encoder:
            return None
        lang = honour_modality and self._modality(state) == _lib.MODALITY["lang"]
        return "goal_emb." if lang else "lang_emb."

    def param_grads(self, grads: torch.Tensor, params, unused: Optional[str] = None):
        """Views of the flat gradient buffer, one per (name, parameter) of the module; None where this forward did
        not read the parameter (proprio_emb, the other modality's goal embedder), as autograd leaves it in the
        reference -- optimizers skip such parameters instead of decaying them."""
        out = []
        for name, p in params:
            ent = self._grad_layout.get("inner_model." + name)
            if ent is None or not p.requires_grad or (unused and name.startswith(unused)):
                out.append(None)
            else:
                out.append(grads[ent[0]:ent[0] + ent[1]].view(p.shape))
        return out

    def flops_per_chunk(self, n_steps: int) -> float:
        return float(self.lib.mdt_flops_per_chunk(self.handle, int(n_steps)))


class HipScoreNetwork(nn.Module):
    """Common facade logic of the two score networks; subclasses build the parameter tree in reference order."""

    _arch = "mdtv"

    def _init_common(self):
        from ...utils import weight_cache
        weight_cache.track(self)  # fused torch optimizers do not bump version counters: an optimizer hook marks us dirty
        self.latent_encoder_emb = None
        self._engines: Dict[tuple, HipEngine] = {}
        self._sigma_data = 1.0

    # -- configuration handed to the library ---------------------------------------------------
    def _hip_config(self, sigma_data: float) -> _lib.MDTConfig:
        raise NotImplementedError

    def hip_engine(self, sigma_data: Optional[float] = None, state: Optional[dict] = None) -> HipEngine:
        """The (lazily created) library handle.  sigma_data defaults to the value the owning GCDenoiser
        registered (``_sigma_data``); it only matters for the preconditioned entry points.  ``state``: the state dict of
        the call -- MDTVTransformer embeds a proprioceptive ``state['state_obs']`` into one more context token when the
        key is present (mdtv_transformer.py:260-266); the two context layouts live in two handles."""
        if sigma_data is None:
            sigma_data = getattr(self, "_sigma_data", 1.0)
        p = next(self.parameters())
        proprio = self._arch == "mdtv" and state is not None and "state_obs" in state
        key = (str(p.device), float(sigma_data), proprio)
        eng = self._engines.get(key)
        if eng is None:
            eng = HipEngine(self, self._hip_config(float(sigma_data), proprio), p.device)
            # a moved / re-scaled model drops the old arenas; the other context layout of the same model stays
            self._engines = {k: e for k, e in self._engines.items() if k[:2] == key[:2]}
            self._engines[key] = eng
        return eng

    def __getstate__(self):  # copy.deepcopy / pickle (EMA copies, checkpoints of whole modules): never the library handle
        d = self.__dict__.copy()
        d["_engines"] = {}
        d.pop("_ctx_engine", None)
        return d

    def __setstate__(self, state):  # the copy is a new module: the optimizer hook has to know it, and it owns no images yet
        super().__setstate__(state)
        from ...utils import weight_cache
        weight_cache.track(self)
        self.mark_dirty()

    def mark_dirty(self) -> None:
        """Public escape hatch of the weight cache (see HipEngine.invalidate): call after writing parameters through
        ``.data`` or a foreign fused optimizer."""
        for eng in getattr(self, "_engines", {}).values():
            eng.invalidate()

    def train(self, mode: bool = True):  # mode switches are rare and a natural point to re-validate the arena
        out = super().train(mode)
        self.mark_dirty()
        return out

    def _load_from_state_dict(self, *a, **kw):
        super()._load_from_state_dict(*a, **kw)
        self.mark_dirty()

    def _apply(self, fn, *a, **kw):  # .to()/.cuda()/.float(): parameters are re-created, drop stale handles
        out = super()._apply(fn, *a, **kw)
        self._engines = {}
        self._ctx_engine = None
        return out

    def train_dropout(self):
        """mdt_dropout of one train-mode forward (fresh seed from torch's CPU generator, so torch.manual_seed makes
        runs repeatable), or None in eval mode / without dropout."""
        embed_p, attn_p, resid_p, mlp_p, goal_p = (float(p) for p in self._pdrops)
        if not self.training or max(attn_p, resid_p, mlp_p, embed_p) <= 0:
            return None
        seed = int(torch.randint(1, 2 ** 62, (1,)).item())
        return _lib.Dropout(attn_p=attn_p, resid_p=resid_p, mlp_p=mlp_p, embed_p=embed_p, seed=seed)

    def _guard_mode(self, allow_grad: bool = False):
        embed_p, attn_p, resid_p, mlp_p, goal_p = (float(p) for p in self._pdrops)
        if self.training and max(attn_p, resid_p, mlp_p, embed_p) > 0 and not (allow_grad and torch.is_grad_enabled()):
            raise NotImplementedError(
                "train() mode with dropout > 0 outside a training step: only GCDenoiser.loss / forward_context_only "
                "under autograd apply dropout on the HIP path; call .eval() for inference")
        if not allow_grad and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            # forward values are exact, but no autograd graph is recorded
            raise NotImplementedError(
                "autograd through the HIP denoiser is not implemented yet (SURVEY.md 8(f) item 1); wrap the call "
                "in torch.no_grad() for inference / loss evaluation.  GCDenoiser.denoise_grad is the explicit, "
                "differentiable form of this call (autograd through D(x; sigma) on the HIP path)")

    # -- reference API ---------------------------------------------------------------------------
    def _goals(self, goals: torch.Tensor, uncond: bool) -> torch.Tensor:
        """preprocess_goals (reference mdtv_transformer.py:246-258) incl. mask_cond (:302-310): in train() mode every
        goal ELEMENT is zeroed with probability goal_drop -- the reference's own torch.bernoulli draw on the goal's
        device, so a seeded run masks the same elements."""
        if goals.dim() == 2:
            goals = goals[:, None, :]
        # a goal SEQUENCE is reduced to its first entry only where the reference does it: when it is as long as the state
        # sequence (mdtv_transformer.py:249 with states_length = n_obs_token, mdt_transformer.py:213/262 with 1); any
        # other length reaches the shape check of the engine and raises, as the reference's Linear would
        states_length = self.n_obs_token if self._arch == "mdtv" else 1
        if goals.shape[1] == states_length and goals.shape[1] != 1 and self.goal_seq_len == 1:
            goals = goals[:, :1, :]
        check_goal_rows(goals, self.goal_seq_len)  # a handle is built for one layout; checked before anything is enqueued
        goal_p = float(self._pdrops[4])
        if self.training and goal_p > 0.0:
            mask = torch.bernoulli(torch.ones(goals.shape, device=goals.device) * goal_p)
            goals = goals * (1.0 - mask)
        if uncond:
            goals = torch.zeros_like(goals)
        return goals

    def forward(self, states, actions, goals, sigma, uncond: Optional[bool] = False):
        """Raw score network F(states, actions, goals, sigma) (reference mdtv_transformer.py:208-211)."""
        self._guard_mode()
        eng = self.hip_engine(state=states)
        ctx = eng.encode(states, self._goals(goals, uncond), honour_modality=self._arch == "mdtv", sigma=sigma)
        self.latent_encoder_emb = ctx
        self._ctx_engine = eng
        return eng.denoise_cached(actions, sigma, _lib.RAW_OUTPUT | _lib.RAW_INPUT)

    def forward_enc_only(self, states, actions=None, goals=None, sigma=None, uncond: Optional[bool] = False):
        """Context tokens (reference mdtv_transformer.py:213-222 / mdt_transformer.py:257-281)."""
        self._guard_mode()
        eng = self.hip_engine(state=states)
        ctx = eng.encode(states, self._goals(goals, uncond), honour_modality=True, sigma=sigma)
        self._ctx_engine = eng
        if self._arch == "mdtv":  # MDTTransformer.forward_enc_only does not cache (mdt_transformer.py:257-281)
            self.latent_encoder_emb = ctx
        return ctx

    def forward_dec_only(self, context, actions, sigma):
        """reference mdtv_transformer.py:224-236; only valid on the context produced by the last encoder call."""
        if context is not self.latent_encoder_emb:
            raise NotImplementedError("forward_dec_only needs the context tensor returned by the immediately "
                                      "preceding forward_enc_only()/forward() of this module")
        self._guard_mode()
        eng = getattr(self, "_ctx_engine", None) or self.hip_engine()  # the handle that holds this context
        return eng.denoise_cached(actions, sigma, _lib.RAW_OUTPUT | _lib.RAW_INPUT)

    def get_params(self):
        return self.parameters()

    def get_block_size(self):
        return self.block_size
