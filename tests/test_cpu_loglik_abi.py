"""mdt_log_likelihood and the mdt_dopri5_* helpers (include/mdt_hip_train.h) as far as they can be seen without a device: exported
with the header's prototypes and bound in _lib.SYMBOLS with matching ctypes, the two structs mirrored field by field, what the
call refuses before it touches a device -- status and mdt_last_error text per cause, against a table recorded from the library,
as tests/test_cpu_candidates_abi.py does for the ``*_multi`` samplers -- the step-size helpers against an instrumented
``gs._dopri5`` run, and the host loop's reading of ``extra_args``."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from mdt_policy_amd import _lib, configs
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.helpers import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdt_log_likelihood"
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read (zeros: MDT-V)
HANDLE = C.addressof(_HANDLE)
_HANDLE_MDT = C.create_string_buffer(1 << 20)  # ... and one whose mdt_config.arch, the handle's first word, says MDT
C.cast(_HANDLE_MDT, C.POINTER(C.c_int32))[0] = 1
HANDLE_MDT = C.addressof(_HANDLE_MDT)
SIZE = C.sizeof(_lib.LoglikParams)

# recorded from the library: (mdt_status, mdt_last_error) per cause
TABLE = {
    "null handle": (1, "mdt_log_likelihood: null handle"),
    "null tokens": (1, "mdt_log_likelihood: null tokens"),
    "null goal": (1, "mdt_log_likelihood: null goal"),
    "null x": (1, "mdt_log_likelihood: null x"),
    "null v": (1, "mdt_log_likelihood: null v"),
    "null ll": (1, "mdt_log_likelihood: null ll"),
    "batch 0": (1, "mdt_log_likelihood: batch is 0, must be >= 1"),
    "candidates 0": (1, "mdt_log_likelihood: candidates is 0, must be >= 1"),
    "candidates -1": (1, "mdt_log_likelihood: candidates is -1, must be >= 1"),
    "probes 0": (1, "mdt_log_likelihood: params.probes is 0, must be >= 1"),
    "params.size": (1, "mdt_log_likelihood: params.size is 24, sizeof(mdt_loglik_params) is 32"),
    "sigma_min 0": (1, "mdt_log_likelihood: sigma_min is 0, must be finite and > 0"),
    "sigma_min nan": (1, "mdt_log_likelihood: sigma_min is nan, must be finite and > 0"),
    "sigma_min inf": (1, "mdt_log_likelihood: sigma_min is inf, must be finite and > 0"),
    "sigma_max <= sigma_min": (1, "mdt_log_likelihood: sigma_max is 0.001, must be finite and > sigma_min (0.001)"),
    "sigma_max inf": (1, "mdt_log_likelihood: sigma_max is inf, must be finite and > sigma_min (0.001)"),
    "rtol 0": (1, "mdt_log_likelihood: params.rtol is 0, must be finite and > 0"),
    "rtol nan": (1, "mdt_log_likelihood: params.rtol is nan, must be finite and > 0"),
    "atol -1": (1, "mdt_log_likelihood: params.atol is -1, must be finite and > 0"),
    "atol inf": (1, "mdt_log_likelihood: params.atol is inf, must be finite and > 0"),
    "max_steps 0": (1, "mdt_log_likelihood: params.max_steps is 0, must be >= 1"),
    "MDT without tokens2": (1, "mdt_log_likelihood: null tokens2: MDT needs the gripper tokens"),
    "not prepared": (5, "training was not prepared: call mdt_train_prepare() and upload the parameters"),
}


def params(size=SIZE, probes=1, rtol=1e-4, atol=1e-4, max_steps=10000):
    return _lib.LoglikParams(size, probes, rtol, atol, max_steps, 0)


def observe(handle=HANDLE, tokens=PTR, tokens2=None, goal=PTR, x=PTR, v=PTR, sigma_min=0.001, sigma_max=80.0, batch=2, candidates=3,
            p=None, ll=PTR):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    st = _lib.load().mdt_log_likelihood(handle, tokens, tokens2, goal, _lib.MODALITY["lang"], x, v, sigma_min, sigma_max, batch,
                                        candidates, None if p is None else C.byref(p), ll, None, None, None, None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


CAUSES = {
    "null handle": dict(handle=None),
    "null tokens": dict(tokens=None),
    "null goal": dict(goal=None),
    "null x": dict(x=None),
    "null v": dict(v=None),
    "null ll": dict(ll=None),
    "batch 0": dict(batch=0),
    "candidates 0": dict(candidates=0),
    "candidates -1": dict(candidates=-1),
    "probes 0": dict(p=params(probes=0)),
    "params.size": dict(p=params(size=SIZE - 8)),
    "sigma_min 0": dict(sigma_min=0.0),
    "sigma_min nan": dict(sigma_min=float("nan")),
    "sigma_min inf": dict(sigma_min=float("inf")),
    "sigma_max <= sigma_min": dict(sigma_max=0.001),
    "sigma_max inf": dict(sigma_max=float("inf")),
    "rtol 0": dict(p=params(rtol=0.0)),
    "rtol nan": dict(p=params(rtol=float("nan"))),
    "atol -1": dict(p=params(atol=-1.0)),
    "atol inf": dict(p=params(atol=float("inf"))),
    "max_steps 0": dict(p=params(max_steps=0)),
    "MDT without tokens2": dict(handle=HANDLE_MDT),
    "not prepared": dict(),  # every argument in order, a handle without a training state: MDT_ERR_STATE, still nothing enqueued
}


def test_the_table_names_every_cause():
    assert set(TABLE) == set(CAUSES)


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_refusals_are_the_recorded_ones(cause):
    assert observe(**CAUSES[cause]) == TABLE[cause]


def test_an_argument_refusal_names_the_entry_and_the_field():
    for cause, field in (("candidates 0", "candidates"), ("probes 0", "probes"), ("params.size", "size"), ("rtol 0", "rtol"),
                         ("atol -1", "atol"), ("max_steps 0", "max_steps"), ("sigma_min 0", "sigma_min"),
                         ("sigma_max <= sigma_min", "sigma_max"), ("batch 0", "batch"), ("MDT without tokens2", "tokens2")):
        st, msg = observe(**CAUSES[cause])
        assert st == 1 and NAME in msg and field in msg, (cause, msg)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_train.h")).read(), flags=re.S)


def _declared(hdr, name):
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/mdt_hip_train.h"
    return m.group(1), [" ".join(a.split()) for a in m.group(2).split(",")]


def test_the_symbols_are_exported_with_the_headers_prototypes():
    lib, hdr = _lib.load(), _header()
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    res, args = _declared(hdr, NAME)
    assert res == "mdt_status" and args == [
        "mdt_model *m", "const float *tokens", "const float *tokens2", "const float *goal", "int32_t modality", "const float *x",
        "const float *v", "float sigma_min", "float sigma_max", "int64_t batch", "int32_t candidates",
        "const mdt_loglik_params *params", "float *ll", "float *latent", "float *delta", "mdt_loglik_info *info", "void *stream"]
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    assert table[NAME] == (I32, [V, V, V, V, I32, V, V, F, F, I64, I32, C.POINTER(_lib.LoglikParams), V, V, V,
                                 C.POINTER(_lib.LoglikInfo), V])
    D = C.c_double
    for name, want_args, want in (("mdt_dopri5_h0", ["double d0", "double d1"], [D, D]),
                                  ("mdt_dopri5_h1", ["double h0", "double d1", "double d2"], [D, D, D]),
                                  ("mdt_dopri5_next", ["double h", "double ratio", "int32_t *accept"], [D, D, C.POINTER(I32)])):
        assert hasattr(lib, name), name
        assert _declared(hdr, name) == ("double", want_args), name
        assert table[name] == (D, want), name
    assert hasattr(lib, NAME)


def test_the_structs_mirror_the_header_field_by_field():
    hdr = _header()
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for cname, mirror in (("mdt_loglik_params", _lib.LoglikParams), ("mdt_loglik_info", _lib.LoglikInfo)):
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if decl:
                base, rest = decl.split(" ", 1)
                fields += [(item.strip(), ctype[base]) for item in rest.split(",")]
        assert [(n, t) for n, t in mirror._fields_] == fields, cname
    assert C.sizeof(_lib.LoglikParams) == 32 and _lib.LoglikParams.rtol.offset == 8 and _lib.LoglikParams.max_steps.offset == 24
    assert C.sizeof(_lib.LoglikInfo) == 16
    p = _lib.loglik_params()
    assert (p.size, p.probes, p.rtol, p.atol, p.max_steps) == (32, 1, 1e-4, 1e-4, 10000)  # what params == NULL stands for


# ----------------------------------------------------------------------------------------------------------------
# the controller helpers against gs._dopri5
# ----------------------------------------------------------------------------------------------------------------
def _instrumented_run(monkeypatch, fn, y0, t0, t1, rtol, atol):
    """gs._dopri5 with every _scaled_rms value and every evaluation time recorded."""
    norms, times = [], []
    rms = gs._scaled_rms
    monkeypatch.setattr(gs, "_scaled_rms", lambda parts, scale: norms.append(rms(parts, scale)) or norms[-1])

    def f(t, y):
        times.append(t)
        return fn(t, y)

    gs._dopri5(f, y0, t0, t1, rtol, atol)
    monkeypatch.undo()
    return norms, times


def _replay(norms, times, t0, t1):
    """The recorded norms through mdt_dopri5_h0 / _h1 / _next: the attempted steps as (h, accepted), with the recorded h of each."""
    d0, d1, d2 = norms[:3]
    h0 = _lib.dopri5_start(d0, d1)
    # the probe evaluation sits one guessed step away (the subtraction rounds at ulp(t0), far above 1e-12 of a 1e-5 step)
    assert abs(abs(times[1] - times[0]) - h0) <= 2 * math.ulp(max(abs(t0), abs(times[1])))
    h = _lib.dopri5_start_refine(h0, d1, d2)
    t, direction, out = t0, (1.0 if t1 >= t0 else -1.0), []
    ratios, evals = norms[3:], times[2:]
    assert len(evals) == 6 * len(ratios)
    for n, ratio in enumerate(ratios):
        assert (t1 - t) * direction > 0
        h = min(h, abs(t1 - t))
        recorded = abs(evals[6 * n + 4] - t)  # the attempt's stage at c = 1 sits at t + h
        assert math.isclose(h, recorded, rel_tol=1e-12, abs_tol=0.0), (n, h, recorded)
        h_next, accept = _lib.dopri5_next(h, ratio)
        assert accept == (ratio <= 1.0)
        out.append((h, accept))
        if accept:
            t = t1 if h >= abs(t1 - t) else t + direction * h
        h = h_next
    assert (t1 - t) * direction <= 0
    return out


def test_the_helpers_replay_dopri5s_step_sequence(monkeypatch):
    """The recorded d0 / d1 / d2 and ratios of a gs._dopri5 run on test_dopri5_known_answers' ODE through the helpers: the same
    accept / reject sequence and every step size equal to 1e-12 relative -- double arithmetic on the same formula.  (The step
    is read off the evaluation at c = 1, (t + h) - t: that subtraction's own rounding is 1e-16 |t| / h relative, 1e-13 here.)"""
    def f(t, y):
        return (-2.0 * y[0] + math.sin(t), torch.full_like(y[1], t * t))

    y0, z0 = torch.tensor([1.0, -0.5, 3.0], dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    rejected = 0
    for t0, t1, rtol, atol in ((0.0, 4.0, 1e-7, 1e-9), (4.0, 0.5, 1e-7, 1e-9), (0.0, 4.0, 1e-3, 1e-5)):
        norms, times = _instrumented_run(monkeypatch, f, (y0, z0), t0, t1, rtol, atol)
        steps = _replay(norms, times, t0, t1)
        assert len(steps) >= 5
        rejected += sum(1 for _, a in steps if not a)
    assert rejected >= 1  # the sequence above holds a rejected step


def test_the_helpers_on_a_zero_error_and_at_the_clip_ends(monkeypatch):
    # y' = 0: every stage derivative is zero, the embedded error is exactly 0 -> ratio == 0 -> h * 10, from the 1e-6 start
    norms, times = _instrumented_run(monkeypatch, lambda t, y: (torch.zeros_like(y[0]),), (torch.ones(3, dtype=torch.float64),),
                                     0.0, 2.0, 1e-6, 1e-8)
    assert norms[1] == 0.0 and set(norms[3:]) == {0.0} and len(norms[3:]) >= 6
    _replay(norms, times, 0.0, 2.0)
    assert _lib.dopri5_next(0.25, 0.0) == (2.5, True)
    assert _lib.dopri5_next(0.25, 1.0) == (0.25 * 0.9, True)
    assert _lib.dopri5_next(0.25, 1e9) == (0.25 * 0.2, False)                      # clipped below
    assert _lib.dopri5_next(0.25, 1e-9) == (2.5, True)                             # clipped above
    h, acc = _lib.dopri5_next(0.25, 2.0)
    assert not acc and h == 0.25 * 0.9 * 2.0 ** -0.2
    assert math.isnan(_lib.dopri5_next(0.25, float("nan"))[0]) or _lib.dopri5_next(0.25, float("nan"))[1] is False
    # the starting step's branches: a tiny norm gives 1e-6, a flat right-hand side the 1e-3 h0 floor, never above 100 h0
    assert _lib.dopri5_start(1e-6, 1.0) == 1e-6 and _lib.dopri5_start(1.0, 1e-6) == 1e-6
    assert _lib.dopri5_start(2.0, 4.0) == 0.01 * 2.0 / 4.0
    assert _lib.dopri5_start_refine(0.5, 0.0, 0.0) == max(1e-6, 1e-3 * 0.5)
    assert _lib.dopri5_start_refine(1e-4, 1e-3, 1e-9) == 100 * 1e-4
    assert _lib.dopri5_start_refine(0.005, 3.0, 0.02) == (0.01 / 4.0) ** 0.2


# ----------------------------------------------------------------------------------------------------------------
# the host loop's reading of extra_args
# ----------------------------------------------------------------------------------------------------------------
def _gaussian():
    s2 = 0.7 ** 2
    model = lambda state, x, goal, sigma: x * (s2 / (s2 + sigma ** 2)).reshape(-1, 1, 1)
    torch.manual_seed(3)
    x = torch.randn(4, 10, 7, dtype=torch.float64) * 0.7
    want = torch.distributions.Normal(0, math.sqrt(s2 + 0.02 ** 2)).log_prob(x).flatten(1).sum(1)
    return model, x, want


def test_host_loop_probes_give_the_gaussians_exact_value_for_one_and_three():
    """test_log_likelihood_of_a_gaussian_is_exact's linear model: sign probes are exact there, so P = 1 and P = 3 give the same
    value within that test's tolerance, and the info dict adds up."""
    model, x, want = _gaussian()
    got = {}
    for P in (1, 3):
        ll, info = gs.log_likelihood(model, {}, x, None, 0.02, 4000.0, extra_args={"probes": P}, atol=1e-7, rtol=1e-7)
        assert_close(ll, want, rtol=1e-5, atol=1e-4, what=f"gaussian log-likelihood, probes={P}")
        assert info["fevals"] == 2 + 6 * info["steps"] and info["steps"] == info["n_accept"] + info["n_reject"]
        got[P] = ll
    assert_close(got[3], got[1], rtol=1e-5, atol=1e-4, what="P = 3 against P = 1")


def test_host_loop_uses_a_tensor_of_probes_as_given(monkeypatch):
    """A tensor under 'probes' draws nothing; a NON-sign probe 2 v scales v^T J v by 4 on the linear model, which only a loop
    that reads the tensor shows; P > 1 as an int is one probe-major draw."""
    model, x, want = _gaussian()
    drawn = []
    signs = gs._probe_signs
    monkeypatch.setattr(gs, "_probe_signs", lambda a: drawn.append(tuple(a.shape)) or signs(a))
    v = signs(x)[None]
    drawn.clear()
    ll1, _ = gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"probes": v})
    ll2, _ = gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"probes": 2.0 * v})
    assert drawn == []
    prior = torch.distributions.Normal(0, 400.0).log_prob
    lat = x * math.sqrt((0.49 + 400.0 ** 2) / (0.49 + 0.02 ** 2))  # the linear flow's latent, the same under both probes
    d1, d2 = ll1 - prior(lat).flatten(1).sum(1), ll2 - prior(lat).flatten(1).sum(1)
    assert_close(d2, 4.0 * d1, rtol=1e-3, atol=1e-2, what="delta under 2 v")
    gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"probes": 3})
    assert drawn == [(3,) + tuple(x.shape)]
    drawn.clear()
    gs.log_likelihood(model, {}, x, None, 0.02, 400.0)
    assert drawn == [tuple(x.shape)]  # without the key: the one draw of the reference
    for bad in (0, -1, 1.5, True, v[0]):
        with pytest.raises(ValueError):
            gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"probes": bad})


def test_candidates_with_a_foreign_model_is_a_value_error():
    model, x, _ = _gaussian()
    with pytest.raises(ValueError, match="candidates"):
        gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"candidates": 2})
    with pytest.raises(ValueError, match="candidates"):
        gs.log_likelihood(model, {}, x, None, 0.02, 400.0, extra_args={"candidates": 0})


def test_a_stray_key_with_gcdenoiser_is_refused_by_name_before_anything_runs():
    """The key check comes before the facade's refusal of CPU execution: no device is needed to see it."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    m = GCDenoiser(configs.mdtv_tiny(), 0.5).eval()
    state = {"state_images": torch.zeros(1, 3, 128), "modality": "lang"}
    for key in ("cond_lambda", "pin"):
        with pytest.raises(NotImplementedError, match=key):
            gs.log_likelihood(m, state, torch.zeros(1, 10, 7), torch.zeros(1, 1, 512), 0.001, 80.0,
                              extra_args={key: 2.0, "candidates": 1, "probes": 1})


def test_best_candidates_picks_each_observations_argmax_with_ties_to_the_lowest_index():
    torch.manual_seed(0)
    B, K = 3, 4
    chunks = torch.randn(B * K, 10, 7)
    scores = torch.tensor([[0.1, 0.7, 0.7, -1.0], [5.0, 5.0, 5.0, 5.0], [float("nan"), -3.0, -2.0, -2.0]])
    for ch, sc in ((chunks, scores.reshape(-1)), (chunks.reshape(B, K, 10, 7), scores)):
        best, index = gs.best_candidates(ch, sc, K)
        assert best.shape == (B, 10, 7) and index.shape == (B,)
        assert index.tolist() == [1, 0, 2]
        assert torch.equal(best, chunks.reshape(B, K, 10, 7)[torch.arange(B), index])
    best, index = gs.best_candidates(chunks, torch.arange(12.0), 1)
    assert torch.equal(best, chunks) and index.tolist() == [0] * 12
    with pytest.raises(ValueError):
        gs.best_candidates(chunks, scores.reshape(-1), 5)
    with pytest.raises(ValueError):
        gs.best_candidates(chunks[:8], scores.reshape(-1), K)
    with pytest.raises(ValueError):
        gs.best_candidates(chunks, scores, 0)
