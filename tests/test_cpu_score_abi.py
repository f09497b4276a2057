"""mdt_denoising_score (include/mdt_hip.h) as far as it can be seen without a device: exported with the header's prototype and
bound in _lib.SYMBOLS with matching ctypes, and what the call refuses before it touches a device -- status and mdt_last_error
text per cause, one fault at a time, the message naming the entry and the field (the fake-handle technique of
tests/test_cpu_steer_abi.py: host memory behind every pointer, nothing is ever launched)."""
import ctypes as C
import os
import re

import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mdt_denoising_score"
_BUF = C.create_string_buffer(1 << 16)
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read (zeros: MDT-V)
HANDLE = C.addressof(_HANDLE)
_HANDLE_MDT = C.create_string_buffer(1 << 20)  # ... and one whose mdt_config.arch, the handle's first word, says MDT
C.cast(_HANDLE_MDT, C.POINTER(C.c_int32))[0] = 1
HANDLE_MDT = C.addressof(_HANDLE_MDT)
INVALID = 1
LEVELS = (80.0, 2.0, 0.05, 0.001)
NAN, INF = float("nan"), float("inf")


def observe(handle=HANDLE, tokens=PTR, tokens2=None, goal=PTR, x0=PTR, sigmas=LEVELS, weights=None, n_levels=None, noise=PTR,
            draws=2, batch=2, candidates=3, score=PTR):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    sig = None if sigmas is None else (C.c_float * len(sigmas))(*sigmas)
    w = None if weights is None else (C.c_float * len(weights))(*weights)
    n = (len(sigmas) if sigmas is not None else 3) if n_levels is None else n_levels
    st = _lib.load().mdt_denoising_score(handle, tokens, tokens2, goal, _lib.MODALITY["lang"], x0, sig, w, n, noise, draws, batch,
                                         candidates, score, None, None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


# cause -> (arguments, the field the message names)
CAUSES = {
    "null handle": (dict(handle=None), "handle"),
    "null tokens": (dict(tokens=None), "tokens"),
    "null goal": (dict(goal=None), "goal"),
    "null x0": (dict(x0=None), "x0"),
    "null sigmas": (dict(sigmas=None), "sigmas"),
    "null noise": (dict(noise=None), "noise"),
    "null score": (dict(score=None), "score"),
    "batch 0": (dict(batch=0), "batch"),
    "batch -1": (dict(batch=-1), "batch"),
    "candidates 0": (dict(candidates=0), "candidates"),
    "candidates -2": (dict(candidates=-2), "candidates"),
    "n_levels 0": (dict(n_levels=0), "n_levels"),
    "n_levels 65": (dict(sigmas=tuple(100.0 - i for i in range(65))), "n_levels"),
    "draws 0": (dict(draws=0), "draws"),
    "draws 65": (dict(draws=65), "draws"),
    "a level of zero": (dict(sigmas=(80.0, 0.0, 0.05)), "sigmas[1]"),
    "a negative level": (dict(sigmas=(80.0, 2.0, -0.05)), "sigmas[2]"),
    "a nan level": (dict(sigmas=(NAN, 2.0, 0.05)), "sigmas[0]"),
    "an infinite level": (dict(sigmas=(INF, 2.0, 0.05)), "sigmas[0]"),
    "a negative weight": (dict(weights=(1.0, -1.0, 1.0, 1.0)), "weights[1]"),
    "a nan weight": (dict(weights=(1.0, 1.0, NAN, 1.0)), "weights[2]"),
    "an infinite weight": (dict(weights=(1.0, 1.0, 1.0, INF)), "weights[3]"),
    "default weights, a repeated level": (dict(sigmas=(80.0, 2.0, 2.0, 0.001)), "sigmas[2]"),
    "default weights, a turn": (dict(sigmas=(80.0, 2.0, 3.0, 0.001)), "sigmas[2]"),
    "default weights, a turn while rising": (dict(sigmas=(0.001, 2.0, 1.0)), "sigmas[2]"),
    "MDT without tokens2": (dict(handle=HANDLE_MDT), "tokens2"),
    "too many rows": (dict(batch=1 << 22, candidates=2, draws=2), "rows"),
    "too many rows per observation": (dict(batch=1, candidates=1 << 20, sigmas=tuple(100.0 - i for i in range(64)), draws=64), "rows"),
}


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_an_argument_refusal_names_the_entry_and_the_field(cause):
    kw, field = CAUSES[cause]
    st, msg = observe(**kw)
    assert st == INVALID and msg.startswith(NAME + ": ") and field in msg, (cause, st, msg)


def test_the_messages_say_what_was_wrong():
    assert observe(batch=0)[1] == NAME + ": batch is 0, must be >= 1"
    assert observe(candidates=-2)[1] == NAME + ": candidates is -2, must be >= 1"
    assert observe(n_levels=0)[1] == NAME + ": n_levels is 0, must be in [1, 64]"
    assert observe(draws=65)[1] == NAME + ": draws is 65, must be in [1, 64]"
    assert observe(sigmas=(80.0, 0.0, 0.05))[1] == NAME + ": sigmas[1] is 0, must be finite and > 0"
    assert observe(weights=(1.0, -1.0, 1.0, 1.0))[1] == NAME + ": weights[1] is -1, must be finite and >= 0"
    assert observe(sigmas=(80.0, 2.0, 3.0, 0.001))[1].startswith(NAME + ": sigmas[2] is 3 after 2: without weights the levels must be "
                                                                 "strictly monotone")
    assert observe(handle=HANDLE_MDT)[1] == NAME + ": null tokens2: MDT needs the gripper tokens"


def test_given_weights_lift_the_order_of_the_levels():
    """With weights the levels may come in any order: the same unordered levels that the default refuses pass that check and
    reach the next one (here: too many rows), still with nothing enqueued."""
    st, msg = observe(sigmas=(80.0, 2.0, 3.0, 0.001), weights=(1.0, 0.0, 1.0, 1.0), batch=1 << 22)
    assert st == INVALID and "rows" in msg and "monotone" not in msg, (st, msg)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip.h")).read(), flags=re.S)


def test_the_symbol_is_exported_with_the_headers_prototype():
    m = re.search(r"(\w+)\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{NAME} is not declared in include/mdt_hip.h"
    assert m.group(1) == "mdt_status" and [" ".join(a.split()) for a in m.group(2).split(",")] == [
        "mdt_model *m", "const float *tokens", "const float *tokens2", "const float *goal", "int32_t modality", "const float *x0",
        "const float *sigmas_host", "const float *weights_host", "int32_t n_levels", "const float *noise", "int32_t draws",
        "int64_t batch", "int32_t candidates", "float *score", "float *ctx_out", "void *stream"]
    V, I32, I64, FP = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float)
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    assert table[NAME] == (I32, [V, V, V, V, I32, V, FP, FP, I32, V, I32, I64, I32, V, V, V])
    assert hasattr(_lib.load(), NAME)
