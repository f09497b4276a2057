"""Sample, score and select in one call (mdt_sample*_select, include/mdt_hip.h; gc_sampling.sample_select) as far as it can be seen
without a device: the four entries exported with the header's prototypes -- each its ``*_multi`` entry with ``out`` named ``best``
and ``const mdt_select_spec *select`` in front of ``stream`` -- and bound in _lib.SYMBOLS, mdt_select_spec mirrored by
_lib.SelectSpec, what the entries and the kernel's hook refuse before they touch a device (status, text, and nothing written:
host memory stands behind every pointer, as in tests/test_cpu_score_abi.py), the float64 restatement of the selection rule
(tests/select_cases.py) against gc_sampling.best_candidates, and which gc_sampling.sample_select calls go to the one native call
(a recorder stands in for the library, as in tests/test_action_steer.py)."""
import ctypes as C
import os
import re
from contextlib import nullcontext

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
from tests import select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = {"mdt_sample_ddim_select": "mdt_sample_ddim_multi", "mdt_sample_ddim_dev_select": "mdt_sample_ddim_dev_multi",
          "mdt_sample_select": "mdt_sample_multi", "mdt_sample_dev_select": "mdt_sample_dev_multi"}
HEUN = _lib.SAMPLER_KIND["heun"]
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read
HANDLE = C.addressof(_HANDLE)
SIGMAS = (C.c_float * 4)(80.0, 10.0, 1.0, 0.0)
LEVELS = (80.0, 2.0, 0.05, 0.001)
SPEC_SIZE = C.sizeof(_lib.SelectSpec)
NAN, INF = float("nan"), float("inf")
INVALID = 1


def observe(name, handle=HANDLE, batch=2, candidates=3, best=PTR, spec=True, size=SPEC_SIZE, levels=LEVELS, weights=None,
            n_levels=None, noise=PTR, draws=2, chunks=PTR, scores=PTR, index=PTR, opts=None):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    sig = None if levels is None else (C.c_float * len(levels))(*levels)
    w = None if weights is None else (C.c_float * len(weights))(*weights)
    n = (len(levels) if levels is not None else 3) if n_levels is None else n_levels
    sp = _lib.SelectSpec(size, sig, w, n, noise, draws, chunks, scores, index)
    sched = PTR if "_dev" in name else SIGMAS
    mid = (sched, 3) if "ddim" in name else (HEUN, None, sched, 3, None, 0)
    before = bytes(_BUF)
    st = getattr(_lib.load(), name)(handle, None, None, None, _lib.MODALITY["lang"], PTR, *mid, batch, candidates, best, None,
                                    None if opts is None else C.byref(opts), C.byref(sp) if spec else None, None)
    assert bytes(_BUF) == before, f"{name}: a refused call wrote to a buffer"
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


# cause -> (arguments, the field the message names)
CAUSES = {
    "null select": (dict(spec=False), "null select"),
    "select.size": (dict(size=SPEC_SIZE - 8), "select.size"),
    "select.size 0": (dict(size=0), "select.size"),
    "null best": (dict(best=None), "null best"),
    "null chunks": (dict(chunks=None), "null select.chunks"),
    "null scores": (dict(scores=None), "null select.scores"),
    "null index": (dict(index=None), "null select.index"),
    "null sigmas_host": (dict(levels=None), "null select.sigmas_host"),
    "null noise": (dict(noise=None), "null select.noise"),
    "n_levels 0": (dict(n_levels=0), "n_levels is 0, must be in [1, 64]"),
    "n_levels 65": (dict(levels=tuple(100.0 - i for i in range(65))), "n_levels is 65, must be in [1, 64]"),
    "draws 0": (dict(draws=0), "draws is 0, must be in [1, 64]"),
    "draws 65": (dict(draws=65), "draws is 65, must be in [1, 64]"),
    "a level of zero": (dict(levels=(80.0, 0.0, 0.05)), "sigmas[1] is 0, must be finite and > 0"),
    "a negative level": (dict(levels=(80.0, 2.0, -0.05)), "sigmas[2]"),
    "a nan level": (dict(levels=(NAN, 2.0, 0.05)), "sigmas[0]"),
    "an infinite level": (dict(levels=(INF, 2.0, 0.05)), "sigmas[0]"),
    "a negative weight": (dict(weights=(1.0, -1.0, 1.0, 1.0)), "weights[1] is -1, must be finite and >= 0"),
    "a nan weight": (dict(weights=(1.0, 1.0, NAN, 1.0)), "weights[2]"),
    "an infinite weight": (dict(weights=(1.0, 1.0, 1.0, INF)), "weights[3]"),
    "default weights, a repeated level": (dict(levels=(80.0, 2.0, 2.0, 0.001)), "sigmas[2] is 2 after 2: without weights the levels "
                                                                                 "must be strictly monotone"),
    "default weights, a turn": (dict(levels=(80.0, 2.0, 3.0, 0.001)), "sigmas[2] is 3 after 2: without weights"),
    "too many rows": (dict(batch=1 << 22, candidates=2, draws=2), "batch * candidates * n_levels * draws = 4194304 * 2 * 4 * 2 rows "
                                                                   "is more than the decoder's 16777216 samples"),
    "too many rows per observation": (dict(batch=1, candidates=1 << 20, levels=tuple(100.0 - i for i in range(64)), draws=64), "rows"),
}


@pytest.mark.parametrize("name", sorted(SELECT))
@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_a_refusal_names_the_entry_and_the_field_and_writes_nothing(cause, name):
    kw, text = CAUSES[cause]
    st, msg = observe(name, **kw)
    assert st == INVALID and msg.startswith(name + ": ") and text in msg, (cause, st, msg)


def test_the_score_refusals_are_worded_as_mdt_denoising_score_words_them():
    lib = _lib.load()
    for lv, w, draws in (((80.0, 0.0, 0.05), None, 2), ((80.0, 2.0, 3.0), None, 2), (LEVELS, (1.0, -1.0, 1.0, 1.0), 2), (LEVELS, None, 65)):
        sig, wt = (C.c_float * len(lv))(*lv), None if w is None else (C.c_float * len(w))(*w)
        assert lib.mdt_denoising_score(HANDLE, PTR, None, PTR, 1, PTR, sig, wt, len(lv), PTR, draws, 2, 3, PTR, None, None) == INVALID
        want = lib.mdt_last_error().decode()
        assert want.startswith("mdt_denoising_score: ")
        for name in SELECT:
            st, msg = observe(name, levels=lv, weights=w, draws=draws)
            assert st == INVALID and msg == name + want[len("mdt_denoising_score"):], (name, msg, want)


def test_what_the_multi_entry_refuses_is_refused_as_before():
    """The same cause through the *_multi entry and through its *_select form: the same status and, but for the entry's own name
    where the message carries it, the same text."""
    lib = _lib.load()
    for name, base in SELECT.items():
        sched = PTR if "_dev" in name else SIGMAS
        mid = (sched, 3) if "ddim" in name else (HEUN, None, sched, 3, None, 0)
        for handle, batch, cand, o in ((None, 2, 3, None), (HANDLE, 0, 3, None), (HANDLE, 2, 0, None), (HANDLE, 2, -1, None),
                                       (None, 2, 3, _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 3.0, None, None, None, None, None, None)),
                                       (HANDLE, 2, 3, _lib.SampleOpts(48, 1.0, None, None, None, None, None, None)),
                                       (HANDLE, 2, 3, _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0, PTR, None, None, None, None, None)),
                                       (HANDLE, 2, 3, _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0, None, None, None, None, PTR, None))):
            st0 = getattr(lib, base)(handle, None, None, None, 1, PTR, *mid, batch, cand, PTR, None, None if o is None else C.byref(o), None)
            want = lib.mdt_last_error().decode()
            st, msg = observe(name, handle=handle, batch=batch, candidates=cand, opts=o)
            assert st == st0 == INVALID and msg == want.replace(base, name), (name, msg, want)


def test_record_on_ddim_is_refused_through_the_select_entries_too():
    o = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0, None, None, PTR, None, None, None)
    for name in SELECT:
        if "ddim" in name:
            assert observe(name, opts=o) == (INVALID, f"{name}: opts.record: the DDIM head keeps no per-step record")


def _declared(hdr, name):
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and m.group(1) == "mdt_status", f"{name} is not declared in include/mdt_hip.h"
    return [" ".join(a.split()) for a in m.group(2).split(",")]


def test_the_four_symbols_are_exported_with_the_headers_prototypes():
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip.h")).read(), flags=re.S)
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    for name, base in SELECT.items():
        assert hasattr(lib, name), name
        args, multi = _declared(hdr, name), _declared(hdr, base)
        want = ["float *best" if a == "float *out" else a for a in multi]
        assert args == want[:-1] + ["const mdt_select_spec *select", "void *stream"], name
        res, argt = table[name]
        assert res == C.c_int32 and argt == table[base][1][:-1] + [C.POINTER(_lib.SelectSpec), C.c_void_p], name


def test_the_struct_is_the_headers():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    body = re.search(r"typedef struct mdt_select_spec \{(.*?)\} mdt_select_spec;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in decl.split(" ", 2 if decl.startswith("const") else 1)[-1].split(",")]
    assert names == [f[0] for f in _lib.SelectSpec._fields_]
    assert names[0] == "size" and _lib.SelectSpec.size.offset == 0
    P = C.sizeof(C.c_void_p)
    assert [getattr(_lib.SelectSpec, n).offset for n in names] == [0, P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 7 * P, 8 * P]
    assert C.sizeof(_lib.SelectSpec) == 9 * P


# ----------------------------------------------------------------------------------------------------------------
# the kernel's hook
# ----------------------------------------------------------------------------------------------------------------
def hook(scores=PTR, chunks=PTR, B=2, K=3, E=70, best=PTR, index=PTR):
    before = bytes(_BUF)
    st = _lib.load().mdt_op_score_select(scores, chunks, B, K, E, best, index, None)
    assert bytes(_BUF) == before
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


@pytest.mark.parametrize("kw,text", [(dict(scores=None), "null scores"), (dict(chunks=None), "null chunks"), (dict(best=None), "null best"),
                                     (dict(index=None), "null index"), (dict(B=0), "B is 0, must be >= 1"),
                                     (dict(K=0), "K is 0, must be >= 1"), (dict(E=-1), "E is -1, must be >= 1"),
                                     (dict(B=1 << 31), "B is 2147483648")])
def test_the_hook_refuses_by_name_before_anything_is_enqueued(kw, text):
    st, msg = hook(**kw)
    assert st == INVALID and msg.startswith("mdt_op_score_select: ") and text in msg, msg


def test_the_hook_is_declared_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_debug.h")).read(), flags=re.S)
    assert _declared(hdr, "mdt_op_score_select") == ["const float *scores", "const float *chunks", "int64_t B", "int32_t K",
                                                     "int32_t E", "float *best", "int32_t *index", "void *stream"]
    V = C.c_void_p
    assert {n: a for n, _, a in _lib.SYMBOLS}["mdt_op_score_select"] == [V, V, C.c_int64, C.c_int32, C.c_int32, V, V, V]


# ----------------------------------------------------------------------------------------------------------------
# the rule in float64 against best_candidates
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 5, 8, 65, 300])
def test_the_float64_rule_is_best_candidates(K):
    cases = sc.patterns(K)
    names = {n.split(" at ")[0].split(",")[0] for n, _, _ in cases}
    assert {"all nan", "background"} <= names and (K == 1 or {"tie", "one nan", "-inf", "+inf"} <= names)
    scores = torch.from_numpy(np.stack([s for _, s, _ in cases]))          # one observation per pattern
    chunks = torch.arange(scores.numel() * 6, dtype=torch.float32).reshape(-1, 2, 3)
    best, index = gs.best_candidates(chunks, scores.reshape(-1), K)
    want_index, want_best = sc.select(scores.numpy(), chunks.numpy().reshape(scores.numel(), -1), K)
    for (name, s, k), got in zip(cases, index.tolist()):
        assert got == k, (K, name, s.tolist(), got, k)
    assert index.dtype == torch.int64 and index.tolist() == want_index.tolist()
    assert np.array_equal(best.numpy().reshape(len(cases), -1), want_best)


def test_the_rule_on_the_cases_by_hand():
    assert sc.select_index([1.0, 3.0, 3.0]) == 1 and sc.select_index([3.0, 1.0, 3.0]) == 0 and sc.select_index([0.0, 3.0, 3.0, 3.0]) == 1
    assert sc.select_index([NAN, -5.0, NAN]) == 1 and sc.select_index([NAN, NAN, NAN]) == 0
    assert sc.select_index([NAN, -INF, NAN]) == 1 and sc.select_index([-INF, NAN]) == 0
    assert sc.select_index([1.0, INF, 2.0]) == 1 and sc.select_index([7.0]) == 0 and sc.select_index([NAN]) == 0
    assert sc.select_index([sc.F32_MAX, INF]) == 0  # torch.nan_to_num reads +Inf as the largest finite float


# ----------------------------------------------------------------------------------------------------------------
# routing (no device: a recorder stands in for the library)
# ----------------------------------------------------------------------------------------------------------------
B, TA, A, K = 3, 10, 7, 4


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GCDenoiser(configs.mdtv_tiny(), 0.5).eval()


def _args(layout4=False):
    state = {"state_images": torch.randn(B, 3, 128), "modality": "lang"}
    x = torch.randn(B, K, TA, A) if layout4 else torch.randn(B * K, TA, A)
    return state, x, torch.randn(B, 1, 512), gs.get_sigmas_exponential(4, 0.01, 80.0)


@pytest.fixture
def recorder(model, monkeypatch):
    calls = []

    def select(self, state, action, goal, sigmas, levels, candidates, **kw):
        calls.append(("select", kw.get("kind"), candidates, kw, tuple(action.shape), list(levels)))
        n = action.shape[0] // candidates
        scores = torch.arange(action.shape[0], dtype=torch.float32)
        return action[candidates - 1::candidates], torch.full((n,), candidates - 1), scores, action.clone()

    def native(self, kind, state, action, goal, sigmas, noise=None, n_steps=None, **kw):
        calls.append(("sample", kind, kw.get("candidates"), dict(kw, noise=noise), tuple(action.shape)))
        return action.clone()

    def ddim(self, state, action, goal, sigmas, **kw):
        calls.append(("sample", "ddim", kw.get("candidates"), kw, tuple(action.shape)))
        return action.clone()

    def score(self, state, rows, goal, sigmas, noise, weights=None, candidates=1):
        calls.append(("score", None, candidates, {"weights": weights, "noise": noise}, tuple(rows.shape), tuple(noise.shape)))
        return torch.arange(rows.shape[0], dtype=torch.float32)

    def forward(self, state, action, goal, sigma, **kw):
        calls.append(("forward", None, kw.get("candidates"), kw, tuple(action.shape)))
        return 0.5 * action

    monkeypatch.setattr(GCDenoiser, "forward", forward)
    monkeypatch.setattr(GCDenoiser, "cached_context", lambda self, state, goal: nullcontext())
    monkeypatch.setattr(GCDenoiser, "sample_select", select)
    monkeypatch.setattr(GCDenoiser, "sample_native", native)
    monkeypatch.setattr(GCDenoiser, "sample_ddim", ddim)
    monkeypatch.setattr(GCDenoiser, "denoising_score", score)
    monkeypatch.setattr(gs, "GraphedSelect", None)  # tensors on the host are never graphed
    return calls


LV = [80.0, 2.0, 0.05]


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m", "euler_ancestral", "heun", "lms"])
@pytest.mark.parametrize("layout4", [False, True])
def test_the_admitted_calls_are_one_native_call_with_the_shapes_of_action(model, recorder, sampler, layout4):
    state, x, goal, sig = _args(layout4)
    best, index, scores, chunks = gs.sample_select(model, state, x, goal, sig, LV, sampler=sampler, extra_args={"candidates": K})
    assert [c[0] for c in recorder] == ["select"]
    _, kind, k, kw, shape, levels = recorder[0]
    assert kind == (None if sampler == "ddim" else sampler) and k == K and shape == (B * K, TA, A) and levels == LV
    assert tuple(kw["score_noise"].shape) == (3, 2, TA, A) and torch.equal(kw["score_noise"][:, 0], -kw["score_noise"][:, 1])
    want_rows = {"ddim": None, "dpmpp_2m": None, "lms": None, "heun": len(sig) - 1, "euler_ancestral": len(sig) - 2}[sampler]
    assert (kw["noise"] is None) if want_rows is None else tuple(kw["noise"].shape) == (want_rows, B * K, TA, A)
    assert tuple(best.shape) == (B, TA, A) and tuple(index.shape) == (B,)
    assert tuple(scores.shape) == ((B, K) if layout4 else (B * K,)) and chunks.shape == x.shape


def test_the_weight_the_pin_the_bounds_and_the_scoring_arguments_ride_in_the_call(model, recorder):
    from mdt_policy_amd.utils.action_pin import ActionPin
    state, x, goal, sig = _args()
    bounds = type("Bounds", (), {"clip_bounds": lambda self, device: (torch.zeros(A), torch.ones(A)),
                                 "clip_output": lambda self, a: a.clamp(0, 1)})()
    pin = ActionPin.overlap(torch.randn(B, TA, A), 2, 3)
    noise = torch.randn(3, 5, TA, A)
    gs.sample_select(model, state, x, goal, sig, LV, sampler="euler", scaler=bounds, weights=[1.0, 0.0, 2.0], noise=noise,
                     extra_args={"candidates": K, "cond_lambda": 2.0, "pin": pin})
    (tag, kind, k, kw, _, _), = recorder
    assert tag == "select" and kind == "euler" and kw["cond_lambda"] == 2.0 and kw["weights"] == [1.0, 0.0, 2.0]
    assert kw["score_noise"] is noise and len(kw["bounds"]) == 2 and tuple(kw["pin"][0].shape) == (B * K, TA, A)


def test_a_seeded_call_draws_what_the_three_functions_draw(model, recorder):
    state, x, goal, sig = _args()
    torch.manual_seed(7)
    gs.sample_select(model, state, x, goal, sig, LV, sampler="heun", extra_args={"candidates": K})
    torch.manual_seed(7)
    cands = gs.sample_heun(model, state, x, goal, sig, extra_args={"candidates": K})
    gs.denoising_score(model, state, cands, goal, LV, extra_args={"candidates": K})
    one, sample, score = recorder
    assert one[0] == "select" and sample[0] == "sample" and score[0] == "score"
    assert torch.equal(one[3]["noise"], sample[3]["noise"]) and torch.equal(one[3]["score_noise"], score[3]["noise"])


def test_what_the_native_call_does_not_admit_runs_the_three_functions(model, recorder):
    state, x, goal, sig = _args()
    clip_only = type("Scaler", (), {"clip_output": lambda self, a: a})()
    best, index, scores, chunks = gs.sample_select(model, state, x, goal, sig, LV, sampler="euler", scaler=clip_only,
                                                   extra_args={"candidates": K})
    assert [c[0] for c in recorder] == ["forward"] * (len(sig) - 1) + ["score"]  # sample_euler's host loop, then the score
    assert all(c[2] == K for c in recorder)
    assert tuple(best.shape) == (B, TA, A) and index.tolist() == [K - 1] * B and tuple(scores.shape) == (B * K,)
    del recorder[:]
    gs.sample_select(model, state, x, goal, sig, LV, sampler="dpmpp_2s", extra_args={"candidates": K})
    assert [c[:2] for c in recorder] == [("sample", "dpmpp_2s"), ("score", None)]
    del recorder[:]
    gs.sample_select(model, state, x, goal, sig, LV, sampler="ddim", scaler=clip_only, extra_args={"candidates": K})
    assert [c[0] for c in recorder] == ["select"]  # DDIM never reads its scaler


def test_the_named_refusals(model, recorder):
    state, x, goal, sig = _args()
    with pytest.raises(NotImplementedError, match="'steer'"):
        gs.sample_select(model, state, x, goal, sig, LV, extra_args={"candidates": K, "steer": object()})
    with pytest.raises(NotImplementedError, match="'probes'"):
        gs.sample_select(model, state, x, goal, sig, LV, extra_args={"candidates": K, "probes": 2})
    with pytest.raises(ValueError, match="candidates"):
        gs.sample_select(model, state, x, goal, sig, LV)
    with pytest.raises(ValueError, match="antithetic pairs need an even count"):
        gs.sample_select(model, state, x, goal, sig, LV, draws=3, extra_args={"candidates": K})
    with pytest.raises(ValueError, match=r"sigmas\[1\] is 0"):
        gs.sample_select(model, state, x, goal, sig, [80.0, 0.0], extra_args={"candidates": K})
    with pytest.raises(ValueError, match="strictly monotone"):
        gs.sample_select(model, state, x, goal, sig, [80.0, 2.0, 3.0], extra_args={"candidates": K})
    with pytest.raises(ValueError, match="noise is"):
        gs.sample_select(model, state, x, goal, sig, LV, noise=torch.randn(2, 2, TA, A), extra_args={"candidates": K})
    assert recorder == []


class Shrink:
    """A foreign denoiser: D(x; sigma) = x / 2."""

    def __call__(self, state, x, goal, sigma, **kw):
        return 0.5 * x


def test_a_foreign_model_runs_the_three_functions_and_refuses_candidates(recorder):
    state, x, goal, sig = _args()
    with pytest.raises(ValueError, match="'candidates' needs this package's GCDenoiser"):
        gs.sample_select(Shrink(), state, x, goal, sig, LV, extra_args={"candidates": K})
    torch.manual_seed(3)
    best, index, scores, chunks = gs.sample_select(Shrink(), state, x, goal, sig, LV)
    torch.manual_seed(3)
    want = gs.sample_ddim(Shrink(), state, x, goal, sig)
    want_scores = gs.denoising_score(Shrink(), state, want, goal, LV)
    assert torch.equal(chunks, want) and torch.equal(best, want) and torch.equal(scores, want_scores)
    assert index.tolist() == [0] * (B * K) and index.dtype == torch.int64 and recorder == []
