"""mdt_sample_ddim_steer (include/mdt_hip_train.h) as far as it can be seen without a device: exported with the header's
prototype and bound in _lib.SYMBOLS with matching ctypes, and what the call refuses before it touches a device -- status and
mdt_last_error text per cause, the message naming the entry and the field (tests/test_cpu_loglik_abi.py does the same for
mdt_log_likelihood)."""
import ctypes as C
import os
import re

import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdt_sample_ddim_steer"
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read (zeros: MDT-V)
HANDLE = C.addressof(_HANDLE)
_HANDLE_MDT = C.create_string_buffer(1 << 20)  # ... and one whose mdt_config.arch, the handle's first word, says MDT
C.cast(_HANDLE_MDT, C.POINTER(C.c_int32))[0] = 1
HANDLE_MDT = C.addressof(_HANDLE_MDT)
INVALID, STATE = 1, 5
SCHEDULE = (80.0, 2.0, 0.05, 0.0)
_KEEP = []


def observe(handle=HANDLE, tokens=PTR, tokens2=None, goal=PTR, x_T=PTR, sigmas=SCHEDULE, n_steps=None, batch=2, candidates=3,
            known=PTR, weight=PTR, beta=5.0, lo=None, hi=None, out=PTR):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    sig = None
    if sigmas is not None:
        sig = (C.c_float * len(sigmas))(*sigmas)
        _KEEP[:] = [sig]
    n = (len(sigmas) - 1 if sigmas is not None else 3) if n_steps is None else n_steps
    st = _lib.load().mdt_sample_ddim_steer(handle, tokens, tokens2, goal, _lib.MODALITY["lang"], x_T,
                                           None if sig is None else C.cast(sig, C.c_void_p), n, batch, candidates, known, weight,
                                           beta, lo, hi, out, None, None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


# cause -> (arguments, the field the message names)
CAUSES = {
    "null handle": (dict(handle=None), "handle"),
    "null tokens": (dict(tokens=None), "tokens"),
    "null goal": (dict(goal=None), "goal"),
    "null x_T": (dict(x_T=None), "x_T"),
    "null sigmas": (dict(sigmas=None), "sigmas"),
    "null known": (dict(known=None), "known"),
    "null weight": (dict(weight=None), "weight"),
    "null out": (dict(out=None), "out"),
    "batch 0": (dict(batch=0), "batch"),
    "candidates 0": (dict(candidates=0), "candidates"),
    "candidates -2": (dict(candidates=-2), "candidates"),
    "n_steps 0": (dict(n_steps=0), "n_steps"),
    "n_steps above the maximum": (dict(sigmas=tuple([1.0] * (_lib.SAMPLER_MAX_STEPS + 1)) + (0.0,)), "n_steps"),
    "beta 0": (dict(beta=0.0), "beta"),
    "beta -1": (dict(beta=-1.0), "beta"),
    "beta nan": (dict(beta=float("nan")), "beta"),
    "beta inf": (dict(beta=float("inf")), "beta"),
    "schedule with a zero inside": (dict(sigmas=(80.0, 0.0, 0.05, 0.0)), "sigmas[1]"),
    "schedule with a negative level": (dict(sigmas=(80.0, -2.0, 0.05, 0.0)), "sigmas[1]"),
    "schedule with a nan": (dict(sigmas=(float("nan"), 2.0, 0.05, 0.0)), "sigmas[0]"),
    "schedule with an inf": (dict(sigmas=(float("inf"), 2.0, 0.05, 0.0)), "sigmas[0]"),
    "schedule that does not end in 0": (dict(sigmas=(80.0, 2.0, 0.05, 0.01)), "sigmas[3]"),
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
    assert observe(candidates=-2)[1] == NAME + ": candidates is -2, must be >= 1"
    assert observe(n_steps=0)[1] == NAME + f": n_steps is 0, must be in [1, {_lib.SAMPLER_MAX_STEPS}]"
    assert observe(beta=float("nan"))[1] == NAME + ": beta is nan, must be finite and > 0"
    assert observe(sigmas=(80.0, 2.0, 0.05, 0.01))[1] == \
        NAME + ": sigmas[3] is 0.01: the schedule must be finite and > 0, then end in 0"
    assert observe(lo=PTR)[1] == NAME + ": null hi: the bounds lo and hi come together"


def test_the_largest_step_count_passes_the_argument_checks():
    """Every argument in order, on a handle without a training state: MDT_ERR_STATE from the guard mdt_log_likelihood has, still
    with nothing enqueued -- the argument checks, the schedule's among them, are behind us."""
    for sigmas in (SCHEDULE, tuple([1.0] * _lib.SAMPLER_MAX_STEPS) + (0.0,), (0.5, 0.0)):
        st, msg = observe(sigmas=sigmas)
        assert st == STATE and "mdt_train_prepare" in msg, (st, msg)
    assert observe(tokens2=PTR, handle=HANDLE_MDT)[0] == STATE
    assert observe(lo=PTR, hi=PTR)[0] == STATE


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_train.h")).read(), flags=re.S)


def test_the_symbol_is_exported_with_the_headers_prototype():
    m = re.search(r"(\w+)\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in include/mdt_hip_train.h"
    assert m.group(1) == "mdt_status" and [" ".join(a.split()) for a in m.group(2).split(",")] == [
        "mdt_model *m", "const float *tokens", "const float *tokens2", "const float *goal", "int32_t modality", "const float *x_T",
        "const float *sigmas", "int32_t n_steps", "int64_t batch", "int32_t candidates", "const float *known", "const float *weight",
        "float beta", "const float *lo", "const float *hi", "float *out", "float *ctx_out", "void *stream"]
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    assert table[NAME] == (I32, [V, V, V, V, I32, V, V, I32, I64, I32, V, V, F, V, V, V, V, V])
    assert hasattr(_lib.load(), NAME)


def test_the_sample_options_did_not_grow():
    assert C.sizeof(_lib.SampleOpts) == 56
