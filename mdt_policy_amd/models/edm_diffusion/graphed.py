"""One fused DDIM sampler call as a HIP graph.

A rollout calls ``sample_ddim`` with the same shapes step after step (reference mdtv_agent.py:523-550: B = 1, 10 steps).  The
~250 kernel launches of one call are then the same launch sequence with the same addresses, which a HIP graph replays with a
single submission; the results stay bit-identical (same kernels, same order).  Measured on MI355X (``tools/graph_probe.py``,
``MDT_HIP_GRAPH=1 tools/latency.py``): a bare replay takes 1.60 ms host-synchronised at B = 1; through this wrapper (input
copies, parameter check, output clone) 1.67 ms against 1.69 ms for the eager call -- the call is bound by the dependent chain
of its ~250 kernels on the GPU.  Round 3 shortened the chain (1.42 ms of GPU time): now the host needs longer to submit it than
the GPU to run it and the replay wins -- 1.43 against 1.56 ms -- so ``gc_sampling.sample_ddim`` switches rollout-sized calls to
it by itself (``MDT_HIP_GRAPH`` unset: from the third call with the same shapes on, B <= 8).

``GraphedDDIM`` owns static copies of the inputs, captures ``GCDenoiser.sample_ddim`` on them once and replays it; the library's
weight images are updated in place by the usual re-upload (outside the graph), so parameter updates are seen.  The capture is
redone when the library's workspace was re-allocated (``mdt_ws_generation``).  Opt-in: construct it, or set ``MDT_HIP_GRAPH=1`` to
let ``gc_sampling.sample_ddim`` keep one per (batch, steps, modality) of a model.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch


class GraphedDDIM:
    def __init__(self, model, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas: torch.Tensor,
                 cond_lambda: Optional[float] = None, pin: Optional[tuple] = None, candidates: int = 1):
        if x_T.device.type != "cuda":
            raise RuntimeError("GraphedDDIM needs the model and its inputs on a ROCm GPU")
        # pin: (known, keep) of a call captured with pinned actions.  Like the bounds of GraphedSampler the graph reads them from
        # static buffers that every call fills with ITS pin before the replay: only their presence is part of the graph (_call_key)
        if pin is not None:
            self._pin = tuple(t.detach().to(x_T.device, torch.float32).reshape(x_T.shape).clone() for t in pin)
        self.model = model
        self.candidates = int(candidates)  # chunks per observation of the captured call: part of the graph (_call_key)
        self.cond_lambda = cond_lambda  # classifier-free guidance weight of the captured call (None: unguided)
        self.device = x_T.device
        self._static_state: Dict[str, object] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in state.items()}
        self._x = x_T.detach().clone()
        self._goal = goal.detach().clone()
        self._sig = sigmas.detach().to(self.device, torch.float32).clone()
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._gen = None
        self._out = None
        self._ctx = None
        self._last_sig = None
        self._capture()

    def _engine(self):
        return self.model._engine(state=self._static_state)

    _noise = None  # the captured noise rows (GraphedSampler)
    _lo = _hi = None  # the static action bounds of a call captured with bounds (GraphedSampler)
    _pin = None  # the static (known, keep) of a call captured with pinned actions

    def _call_key(self):
        """What besides the shapes a call must share with the captured one to replay it (matches)."""
        key = self.cond_lambda if self._pin is None else (self.cond_lambda, "pin")
        return key if self.candidates == 1 else (key, ("candidates", self.candidates))

    def _run(self):
        kw = {} if self._pin is None else {"pin": self._pin}
        if self.cond_lambda is not None:
            kw["cond_lambda"] = self.cond_lambda
        if self.candidates != 1:
            kw["candidates"] = self.candidates
        return self.model.sample_ddim(self._static_state, self._x, self._goal, self._sig, **kw)

    def _extra_inputs(self, noise, bounds=None, pin=None):
        if (pin is None) != (self._pin is None):
            raise ValueError("a graph captured with pinned actions replays calls with a pin, and only those")
        return ([], []) if pin is None else (list(self._pin), [pin[0], pin[1]])

    def _capture(self) -> None:
        model = self.model
        with torch.no_grad():
            eng = self._engine()
            eng.sync_params()
            eng.reserve(self._x.shape[0])  # chunks; a guided call's warm-up below grows the workspace to twice that before the capture
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):  # warm-up on a side stream, as torch's graph capture wants it
                for _ in range(2):
                    self._run()
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = self._run()
            self._graph, self._out = graph, out
            self._ctx = model.inner_model.latent_encoder_emb
            self._gen = int(eng.lib.mdt_ws_generation(eng.handle))
            self._eng = eng
            self._eng_key = next(k for k, e in model.inner_model._engines.items() if e is eng)

    def matches(self, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas, key=None,
                noise: Optional[torch.Tensor] = None) -> bool:
        """Whether this graph replays the call: the same shapes and noise rows, and ``key`` equal to the captured call's
        (_call_key: the guidance weight, or GraphedSampler's kind, parameters and evaluation count)."""
        if key != self._call_key() or (noise is None) != (self._noise is None):
            return False
        if noise is not None and noise.shape != self._noise.shape:
            return False
        if x_T.shape != self._x.shape or goal.shape != self._goal.shape or len(sigmas) != self._sig.numel():
            return False
        for k, v in self._static_state.items():
            w = state.get(k, None)
            if torch.is_tensor(v):
                if not torch.is_tensor(w) or w.shape != v.shape:
                    return False
            elif w != v:
                return False
        return set(state) == set(self._static_state)

    @torch.no_grad()
    def __call__(self, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas=None, fresh: bool = True,
                 noise: Optional[torch.Tensor] = None, bounds=None, pin=None) -> torch.Tensor:
        """Same result as ``model.sample_ddim(state, x_T, goal, sigmas)``, including ``inner_model.latent_encoder_emb``: both are
        fresh tensors the next call does not touch.  ``fresh=False`` hands out the graph's own static buffers instead (valid
        until the next call; one copy launch less)."""
        eng = self._eng
        im = self.model.inner_model
        if im._engines.get(self._eng_key) is not eng:  # the module was moved / re-created its handle
            eng = self._engine()
            self._gen = None
        eng.sync_params()  # parameter updates go into the arena the graph reads (outside the graph)
        if int(eng.lib.mdt_ws_generation(eng.handle)) != self._gen:
            self._capture()  # the workspace moved: the old graph's addresses are dead
        # the inputs into the graph's static buffers: ONE multi-tensor copy launch for everything that is already on the device
        # (round 5: as one copy_ per tensor these were six dependent ~3 us launches with ~15 us of host cadence between them in front
        # of a 1.19 ms replay)
        dst, src = [], []
        for k, v in self._static_state.items():
            if torch.is_tensor(v):
                dst.append(v); src.append(state[k])
        dst += [self._x, self._goal]; src += [x_T, goal]
        d2, s2 = self._extra_inputs(noise, bounds, pin)
        dst += d2; src += s2
        if sigmas is not None:
            # n + 1 floats: never skipped on identity -- a caller may rewrite its schedule tensor in place (same object, new values).
            # A HOST schedule (the reference's CPU default) is compared by value with the last one copied: equal -> nothing to do
            sg = sigmas if torch.is_tensor(sigmas) else torch.as_tensor(sigmas, dtype=torch.float32)
            if sg.device.type == "cpu":
                sg = sg.detach().to(torch.float32)
                if self._last_sig is None or not torch.equal(sg, self._last_sig):
                    self._sig.copy_(sg)
                    self._last_sig = sg.clone()
            else:
                dst.append(self._sig); src.append(sg.detach())
                self._last_sig = None
        fast = all(torch.is_tensor(b) and b.device == a.device and b.dtype == a.dtype and b.shape == a.shape for a, b in zip(dst, src))
        foreach_copy = getattr(torch, "_foreach_copy_", None)  # private torch API: absent in older wheels -> per-tensor copies
        if fast and foreach_copy is not None:
            foreach_copy(dst, src)
        else:
            for a, b in zip(dst, src):
                a.copy_(b)
        self._graph.replay()
        eng.ctx_generation += 1
        if not fresh:
            self.model.inner_model.latent_encoder_emb = self._ctx
            return self._out
        # Fresh tensors for the caller, as the reference leaves them (mdtv_transformer.py:221 assigns a new tensor at every forward;
        # the agent reads it at mdtv_agent.py:256,330,445): the graph's static action and context buffers leave through ONE
        # concatenating copy launch; the two results are views of that one fresh allocation, so the next replay overwrites neither.
        n = self._out.numel()
        both = torch.cat((self._out.reshape(-1), self._ctx.reshape(-1)))
        self.model.inner_model.latent_encoder_emb = both[n:].view(self._ctx.shape)
        return both[:n].view(self._out.shape)


class GraphedSampler(GraphedDDIM):
    """The same for one of the other samplers (``GCDenoiser.sample_native``): one graph per sampler kind, parameter set and
    shapes (``candidates`` rides among ``params``, as a guidance weight does).  The noise rows of a call (drawn by the caller in
    the Python loop's order) are copied into a static buffer with the other inputs, so a replay consumes the same random stream
    as the eager call."""

    def __init__(self, model, kind: str, params: dict, state: dict, x_T: torch.Tensor, goal: torch.Tensor,
                 sigmas: torch.Tensor, noise: Optional[torch.Tensor], n_steps: Optional[int] = None, tree: Optional[tuple] = None,
                 bounds: Optional[tuple] = None, pin: Optional[tuple] = None):
        # bounds: (lo, hi) action bounds of the captured call (GCDenoiser.sample_native's ``bounds``).  The graph reads them from
        # static (A,) buffers that every call fills with ITS bounds before the replay: the values are not part of the graph, only
        # their presence is (_call_key)
        if bounds is not None:
            self._lo, self._hi = (torch.as_tensor(b).detach().to(x_T.device, torch.float32).reshape(-1).clone() for b in bounds)
        self.kind, self.params, self.n_steps = kind, dict(params), n_steps  # n_steps: dpm_fast's evaluation count
        # tree: (tol, lo, hi) of a dpmpp_sde call that draws Brownian-tree noise inside (GCDenoiser.sample_native's ``tree``); its
        # seeds are then the static input `noise` -- copied in per call, so that a replay walks the new call's trees
        self.tree = None if tree is None else tuple(float(v) for v in tree)
        self._noise = None if noise is None else noise.detach().clone()
        super().__init__(model, state, x_T, goal, sigmas, pin=pin)

    def _call_key(self):
        return ((self.kind, self.params, self.n_steps) + (() if self.tree is None else (("tree",) + self.tree,))
                + (() if self._lo is None else ("bounds",)) + (() if self._pin is None else ("pin",)))

    def _run(self):
        kw = {} if self._lo is None else {"bounds": (self._lo, self._hi)}
        if self._pin is not None:
            kw["pin"] = self._pin
        if self.tree is not None:
            return self.model.sample_native(self.kind, self._static_state, self._x, self._goal, self._sig,
                                            tree=(self._noise,) + self.tree, **kw, **self.params)
        return self.model.sample_native(self.kind, self._static_state, self._x, self._goal, self._sig, noise=self._noise,
                                        n_steps=self.n_steps, **kw, **self.params)

    def _extra_inputs(self, noise, bounds=None, pin=None):
        if (noise is None) != (self._noise is None) or (noise is not None and noise.shape != self._noise.shape):
            raise ValueError("GraphedSampler: the noise rows must have the captured shape")
        if (bounds is None) != (self._lo is None):
            raise ValueError("GraphedSampler: a graph captured with action bounds replays calls with bounds, and only those")
        dst, src = ([], []) if noise is None else ([self._noise], [noise])
        if bounds is not None:
            dst += [self._lo, self._hi]; src += [bounds[0], bounds[1]]
        d2, s2 = super()._extra_inputs(noise, bounds, pin)
        return dst + d2, src + s2


class GraphedSelect(GraphedSampler):
    """The same for ``GCDenoiser.sample_select``: sample, score and select as one replay.  ``kind`` None is DDIM.  ``key`` is the
    call's graph key as ``gc_sampling.sample_select`` forms it: the sampler, K, the score's levels and weights -- host values that
    ride in kernel arguments and are therefore part of the graph -- its draw count, the guidance weight and the presence of bounds
    and a pin.  ``noise`` is the pair (the sampler's noise rows or None, the score's noise rows): both sit in static buffers, with
    the pin and the bounds, and are filled before every replay.  A call returns (best, index, scores, chunks) as fresh tensors."""

    def __init__(self, model, kind: Optional[str], key, state: dict, x_T: torch.Tensor, goal: torch.Tensor, sigmas: torch.Tensor,
                 noise: tuple, levels, weights, candidates: int, cond_lambda: Optional[float] = None,
                 bounds: Optional[tuple] = None, pin: Optional[tuple] = None):
        self._key = key
        self._levels = [float(v) for v in levels]
        self._weights = None if weights is None else [float(v) for v in weights]
        self._K = int(candidates)
        self._lam = cond_lambda
        self._score_noise = noise[1].detach().clone()
        self._sel = None
        super().__init__(model, kind, {}, state, x_T, goal, sigmas, noise[0], bounds=bounds, pin=pin)

    def _call_key(self):
        return self._key

    def _run(self):
        kw = {} if self._lo is None else {"bounds": (self._lo, self._hi)}
        if self._pin is not None:
            kw["pin"] = self._pin
        if self._lam is not None:
            kw["cond_lambda"] = self._lam
        self._sel = self.model.sample_select(self._static_state, self._x, self._goal, self._sig, self._levels, self._K,
                                             kind=self.kind, noise=self._noise, weights=self._weights,
                                             score_noise=self._score_noise, **kw)
        return self._sel[0]

    def matches(self, state, x_T, goal, sigmas, key=None, noise=None) -> bool:
        if noise is None or noise[1].shape != self._score_noise.shape:
            return False
        return super().matches(state, x_T, goal, sigmas, key=key, noise=noise[0])

    def _extra_inputs(self, noise, bounds=None, pin=None):
        dst, src = super()._extra_inputs(noise[0], bounds, pin)
        return dst + [self._score_noise], src + [noise[1]]

    @torch.no_grad()
    def __call__(self, state, x_T, goal, sigmas=None, noise=None, bounds=None, pin=None):
        super().__call__(state, x_T, goal, sigmas, fresh=False, noise=noise, bounds=bounds, pin=pin)
        best, index, scores, chunks = self._sel  # (captured in _capture; a re-capture renews them)
        parts = (best, scores, chunks, self._ctx)
        flat = torch.cat([t.reshape(-1) for t in parts])  # fresh tensors for the caller through ONE copy launch
        views, at = [], 0
        for t in parts:
            views.append(flat[at:at + t.numel()].view(t.shape))
            at += t.numel()
        self.model.inner_model.latent_encoder_emb = views[3]
        return views[0], index.clone(), views[1], views[2]
