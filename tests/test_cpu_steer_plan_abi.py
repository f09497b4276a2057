"""mdt_sample_steer (include/mdt_hip_train.h) as far as it can be seen without a device: exported with the header's prototype and
bound in _lib.SYMBOLS with matching ctypes, and what the call refuses before it touches a device -- status and mdt_last_error
text per cause, the message naming the entry and the field (tests/test_cpu_steer_abi.py does the same for mdt_sample_ddim_steer)."""
import ctypes as C
import os
import re

import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdt_sample_steer"
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read (zeros: MDT-V)
HANDLE = C.addressof(_HANDLE)
_HANDLE_MDT = C.create_string_buffer(1 << 20)  # ... and one whose mdt_config.arch, the handle's first word, says MDT
C.cast(_HANDLE_MDT, C.POINTER(C.c_int32))[0] = 1
HANDLE_MDT = C.addressof(_HANDLE_MDT)
INVALID, STATE = 1, 5
SCHEDULE = (80.0, 2.0, 0.05, 0.0)
KIND = _lib.SAMPLER_KIND
_KEEP = []


def observe(handle=HANDLE, tokens=PTR, tokens2=None, goal=PTR, x_T=PTR, kind="heun", params=None, sigmas=SCHEDULE, n_steps=None,
            noise=None, n_noise=0, batch=2, candidates=3, known=PTR, weight=PTR, beta=5.0, lo=None, hi=None, record=None, out=PTR):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    sig = None
    if sigmas is not None:
        sig = (C.c_float * len(sigmas))(*sigmas)
    prm = None if params is None else _lib.sampler_params(**params)
    _KEEP[:] = [sig, prm]
    n = (len(sigmas) - 1 if sigmas is not None else 3) if n_steps is None else n_steps
    st = _lib.load().mdt_sample_steer(handle, tokens, tokens2, goal, _lib.MODALITY["lang"], x_T,
                                      KIND[kind] if isinstance(kind, str) else kind, None if prm is None else C.byref(prm), sig, n,
                                      noise, n_noise, batch, candidates, known, weight, beta, lo, hi, record, out, None, None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


# cause -> (arguments, the field the message names)
CAUSES = {
    "null handle": (dict(handle=None), "handle"),
    "null tokens": (dict(tokens=None), "tokens"),
    "null goal": (dict(goal=None), "goal"),
    "null x_T": (dict(x_T=None), "x_T"),
    "null sigmas": (dict(sigmas=None), "sigmas_host"),
    "null known": (dict(known=None), "known"),
    "null weight": (dict(weight=None), "weight"),
    "null out": (dict(out=None), "out"),
    "batch 0": (dict(batch=0), "batch"),
    "candidates 0": (dict(candidates=0), "candidates"),
    "beta 0": (dict(beta=0.0), "beta"),
    "beta nan": (dict(beta=float("nan")), "beta"),
    "beta inf": (dict(beta=float("inf")), "beta"),
    "kind -1": (dict(kind=-1), "kind"),
    "kind past the last": (dict(kind=11), "kind"),
    "lms order 0": (dict(kind="lms", params=dict(order=0)), "order"),
    "lms order 5": (dict(kind="lms", params=dict(order=5)), "order"),
    "n_steps 0": (dict(n_steps=0), "n_steps"),
    "n_steps above the maximum": (dict(sigmas=tuple([1.0] * (_lib.SAMPLER_MAX_STEPS + 1)) + (0.0,)), "n_steps"),
    "dpm_fast above its maximum": (dict(kind="dpm_fast", sigmas=(80.0, 0.01), n_steps=_lib.SAMPLER_MAX_EVALS + 1), "n_steps"),
    "dpm_fast with eta going up": (dict(kind="dpm_fast", sigmas=(0.01, 80.0), n_steps=6, params=dict(eta=1.0), noise=PTR, n_noise=3),
                                   "eta"),
    "dpm_fast with eta on one level": (dict(kind="dpm_fast", sigmas=(1.0, 1.0), n_steps=6, params=dict(eta=1.0), noise=PTR,
                                            n_noise=3), "eta"),
    "dpm_fast with a zero level": (dict(kind="dpm_fast", sigmas=(80.0, 0.0), n_steps=6), "sigmas_host[1]"),
    "schedule with a zero inside": (dict(sigmas=(80.0, 0.0, 0.05, 0.0)), "sigmas_host[1]"),
    "schedule with a negative level": (dict(sigmas=(80.0, -2.0, 0.05, 0.0)), "sigmas_host[1]"),
    "schedule with a nan": (dict(sigmas=(float("nan"), 2.0, 0.05, 0.0)), "sigmas_host[0]"),
    "schedule with an inf": (dict(sigmas=(float("inf"), 2.0, 0.05, 0.0)), "sigmas_host[0]"),
    "schedule that does not end in 0": (dict(sigmas=(80.0, 2.0, 0.05, 0.01)), "sigmas_host[3]"),
    "churn without noise": (dict(params=dict(s_churn=1.0)), "noise"),
    "ancestral without noise": (dict(kind="euler_ancestral"), "noise"),
    "sde without noise": (dict(kind="dpmpp_sde"), "noise"),
    "churn with too few rows": (dict(params=dict(s_churn=1.0), noise=PTR, n_noise=2), "n_noise"),
    "sde with too few rows": (dict(kind="dpmpp_sde", noise=PTR, n_noise=3), "n_noise"),
    "lo without hi": (dict(lo=PTR), "hi"),
    "hi without lo": (dict(hi=PTR), "lo"),
    "MDT without tokens2": (dict(handle=HANDLE_MDT), "tokens2"),
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_an_argument_refusal_names_the_entry_and_the_field(cause):
    kw, field = CAUSES[cause]
    st, msg = observe(**kw)
    assert st == INVALID and msg.startswith(NAME + ": ") and field in msg, (cause, st, msg)


def test_the_messages_say_what_was_wrong():
    assert observe(batch=0)[1] == NAME + ": batch is 0, must be >= 1"
    assert observe(kind=11)[1] == NAME + ": kind is 11, must be an mdt_sampler_kind in [0, 11)"
    assert observe(n_steps=0)[1] == NAME + f": n_steps is 0, must be in [1, {_lib.SAMPLER_MAX_STEPS}]"
    assert observe(kind="lms", params=dict(order=5))[1] == NAME + ": params.order is 5, lms takes 1..4"
    assert observe(sigmas=(80.0, 2.0, 0.05, 0.01))[1] == \
        NAME + ": sigmas_host[3] is 0.01: the schedule must be finite and > 0, then end in 0"
    assert observe(params=dict(s_churn=1.0))[1] == NAME + ": null noise: this sampler and parameter set read 3 noise rows"
    assert observe(kind="dpmpp_sde", noise=PTR, n_noise=3)[1] == NAME + ": n_noise is 3, the sampler reads 4 noise rows"
    assert observe(lo=PTR)[1] == NAME + ": null hi: the bounds lo and hi come together"


@pytest.mark.parametrize("kw", [
    dict(), dict(kind="dpmpp_2m"), dict(kind="lms", params=dict(order=1)), dict(kind="euler", noise=PTR, n_noise=3),
    dict(params=dict(s_churn=1.0), noise=PTR, n_noise=3), dict(kind="dpmpp_sde", noise=PTR, n_noise=4),
    dict(kind="dpmpp_sde", params=dict(eta=0.0)), dict(kind="dpm_fast", sigmas=(80.0, 0.01), n_steps=_lib.SAMPLER_MAX_EVALS, params=dict(eta=0.0)),
    dict(kind="dpm_fast", sigmas=(80.0, 0.01), n_steps=6, params=dict(eta=1.0), noise=PTR, n_noise=3),
    dict(kind="dpm_fast", sigmas=(0.01, 80.0), n_steps=4, params=dict(eta=0.0)),
    dict(sigmas=tuple([1.0] * _lib.SAMPLER_MAX_STEPS) + (0.0,)), dict(lo=PTR, hi=PTR), dict(record=PTR),
    dict(tokens2=PTR, handle=HANDLE_MDT)],
    ids=lambda kw: str(kw).replace(str(HANDLE_MDT), "HANDLE_MDT").replace(str(PTR), "PTR"))  # no address in a test's name
def test_good_arguments_pass_the_argument_checks(kw):
    """Every argument in order, on a handle without a training state: MDT_ERR_STATE from the guard mdt_log_likelihood has, still
    with nothing enqueued -- the argument checks, the plan's among them, are behind us."""
    st, msg = observe(**kw)
    assert st == STATE and "mdt_train_prepare" in msg, (st, msg)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_train.h")).read(), flags=re.S)


def test_the_symbol_is_exported_with_the_headers_prototype():
    m = re.search(r"(\w+)\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in include/mdt_hip_train.h"
    assert m.group(1) == "mdt_status" and [" ".join(a.split()) for a in m.group(2).split(",")] == [
        "mdt_model *m", "const float *tokens", "const float *tokens2", "const float *goal", "int32_t modality", "const float *x_T",
        "int32_t kind", "const mdt_sampler_params *params", "const float *sigmas_host", "int32_t n_steps", "const float *noise",
        "int32_t n_noise", "int64_t batch", "int32_t candidates", "const float *known", "const float *weight", "float beta",
        "const float *lo", "const float *hi", "float *record", "float *out", "float *ctx_out", "void *stream"]
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    assert table[NAME] == (I32, [V, V, V, V, I32, V, I32, C.POINTER(_lib.SamplerParams), C.POINTER(F), I32, V, I32, I64, I32,
                                 V, V, F, V, V, V, V, V, V])
    assert hasattr(_lib.load(), NAME)


def test_the_ddim_entry_keeps_its_prototype():
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    assert table["mdt_sample_ddim_steer"] == (I32, [V, V, V, V, I32, V, V, I32, I64, I32, V, V, F, V, V, V, V, V])
