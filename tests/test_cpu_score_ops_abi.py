"""The three score-kernel hooks (include/mdt_hip_debug.h: mdt_op_score_prep, mdt_op_score_repeat, mdt_op_score_reduce) as far as
they can be seen without a device: exported with the header's prototypes, bound in _lib.SYMBOLS with matching ctypes, and every
refusal -- MDT_ERR_INVALID_ARG before anything is launched, the text naming the hook and the field."""
import ctypes as C
import os
import re

import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
INVALID = 1
NAN, INF = float("nan"), float("inf")


def floats(values):
    return (C.c_float * len(values))(*values)


def host(values, n):
    """The host array of a call: ``values`` (a list) or n times the default."""
    return None if values is None else floats(values if isinstance(values, list) else [values] * n)


def prep(x0=PTR, noise=PTR, sigmas=1.0, S=3, K=5, M=2, B=2, Ta=10, A=7, D=64, sd=0.5, WaT=PTR, ba=PTR, y=PTR, noised=PTR, sig_rows=PTR,
         ctx_sig=None):
    return _lib.load().mdt_op_score_prep(x0, noise, host(sigmas, max(S, 1)), S, K, M, B, Ta, A, D, sd, WaT, ba, y, noised, sig_rows,
                                         ctx_sig, None)


def repeat(tok=PTR, tok2=PTR, goal=PTR, B=2, S=3, w1=5, w2=3, wg=7, tok_o=PTR, tok2_o=PTR, goal_o=PTR):
    return _lib.load().mdt_op_score_repeat(tok, tok2, goal, B, S, w1, w2, wg, tok_o, tok2_o, goal_o, None)


def reduce(F=PTR, x0=PTR, noise=PTR, sigmas=1.0, weights=1.0, B=2, S=3, K=5, M=2, E=70, sd=0.5, score=PTR):
    return _lib.load().mdt_op_score_reduce(F, x0, noise, host(sigmas, max(S, 1)), host(weights, max(S, 1)), B, S, K, M, E, sd, score, None)


HOOKS = {"prep": prep, "repeat": repeat, "reduce": reduce}


def nulls(*names):
    return {f"null {n}": ({n: None}, n) for n in names}


def below_1(*names):
    return {f"{n} {v}": ({n: v}, n) for n in names for v in (0, -1)}


def up_to_64(*names):
    return {f"{n} {v}": ({n: v}, n) for n in names for v in (0, -1, 65)}


def level(name, field, bad):
    return {f"{name}[1] {v}": ({name: [1.0, v, 1.0]}, field) for v in bad}


# hook -> cause -> (arguments, the field the message names)
CAUSES = {
    "prep": {**nulls("x0", "noise", "sigmas", "WaT", "ba", "y", "noised", "sig_rows"), **below_1("B", "K", "Ta", "A"),
             **up_to_64("S", "M"), **{f"D {v}": (dict(D=v), "D") for v in (0, 2, -4, 66)},
             **{f"sd {v}": (dict(sd=v), "sd") for v in (0.0, -1.0, NAN, INF)}, **level("sigmas", "sigmas[1]", (0.0, -1.0, NAN, INF))},
    "repeat": {**nulls("tok", "goal", "tok_o", "goal_o", "tok2", "tok2_o"), **below_1("B", "w1", "wg"), **up_to_64("S"),
               "w2 -1": (dict(w2=-1), "w2")},
    "reduce": {**nulls("F", "x0", "noise", "sigmas", "weights", "score"), **below_1("B", "K", "E"), **up_to_64("S", "M"),
               **{f"sd {v}": (dict(sd=v), "sd") for v in (0.0, -1.0, NAN, INF)}, **level("sigmas", "sigmas[1]", (0.0, -1.0, NAN, INF)),
               **level("weights", "weights[1]", (-1.0, NAN, INF)), "B * K 2^31": (dict(B=1 << 28, K=8), "B * K"),
               "B 2^40": (dict(B=1 << 40, K=1), "B * K")},
}
ALL = [(h, c) for h in sorted(CAUSES) for c in sorted(CAUSES[h])]


@pytest.mark.parametrize("hook,cause", ALL, ids=[f"{h}: {c}" for h, c in ALL])
def test_a_refusal_names_the_hook_and_the_field(hook, cause):
    kw, field = CAUSES[hook][cause]
    st = HOOKS[hook](**kw)
    msg = _lib.load().mdt_last_error().decode("utf-8", "replace")
    assert st == INVALID and msg.startswith(f"mdt_op_score_{hook}: ") and field in msg[len(f"mdt_op_score_{hook}: "):], (st, msg)


def test_the_messages_say_what_was_wrong():
    last = lambda: _lib.load().mdt_last_error().decode()
    assert prep(noise=None) == INVALID and last() == "mdt_op_score_prep: null noise"
    assert prep(K=0) == INVALID and last() == "mdt_op_score_prep: K is 0, must be >= 1"
    assert prep(S=65) == INVALID and last() == "mdt_op_score_prep: S is 65, must be in [1, 64]"
    assert prep(D=66) == INVALID and last() == "mdt_op_score_prep: D is 66, must be a multiple of 4 and >= 4"
    assert prep(sigmas=[1.0, 2.0, 0.0]) == INVALID and last() == "mdt_op_score_prep: sigmas[2] is 0, must be finite and > 0"
    assert repeat(w2=-1) == INVALID and last() == "mdt_op_score_repeat: w2 is -1, must be >= 0"
    assert repeat(tok2_o=None) == INVALID and last() == "mdt_op_score_repeat: null tok2_o"
    assert reduce(M=0) == INVALID and last() == "mdt_op_score_reduce: M is 0, must be in [1, 64]"
    assert reduce(weights=[1.0, 1.0, -0.5]) == INVALID and last() == "mdt_op_score_reduce: weights[2] is -0.5, must be finite and >= 0"
    assert reduce(B=1 << 28, K=8) == INVALID and \
        last() == "mdt_op_score_reduce: B * K is 268435456 * 8, more than 2147483647 chunks (one workgroup each)"
    assert reduce(sd=INF) == INVALID and last() == "mdt_op_score_reduce: sd is inf, must be finite and > 0"


def test_what_is_optional_is_not_asked_for():
    """ctx_sig may be null, tok2 and tok2_o where w2 == 0, a zero weight is a weight, and B * K = 2^31 - 1 is a grid.  (Seen as the NEXT
    check's refusal: nothing here may reach a launch.)"""
    last = lambda: _lib.load().mdt_last_error().decode()
    assert prep(ctx_sig=None, sigmas=[1.0, 1.0, -1.0]) == INVALID and "sigmas[2]" in last()
    assert repeat(tok2=None, tok2_o=None, w2=0, wg=0) == INVALID and "wg" in last()
    assert reduce(weights=[0.0, 0.0, -1.0]) == INVALID and "weights[2]" in last()
    assert reduce(B=(1 << 31) - 1, K=1, sd=0.0) == INVALID and "sd" in last()
    # levels and weights beyond the S-th are not read
    assert reduce(S=2, sigmas=[1.0, 1.0, NAN], weights=[1.0, -1.0, NAN]) == INVALID and "weights[1]" in last()


def test_the_checks_come_in_a_fixed_order():
    """Pointers, then extents, then sd, then the levels, then the weights."""
    last = lambda: _lib.load().mdt_last_error().decode()
    assert prep(x0=None, B=0, sd=0.0) == INVALID and "null x0" in last()
    assert prep(B=0, sd=0.0, sigmas=0.0) == INVALID and "B is 0" in last()
    assert prep(sd=0.0, sigmas=0.0) == INVALID and "sd" in last()
    assert reduce(sigmas=0.0, weights=-1.0) == INVALID and "sigmas[0]" in last()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_debug.h")).read(), flags=re.S)


def test_the_symbols_are_exported_with_the_headers_prototypes():
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    ctype = {"float": F, "int32_t": I32, "int64_t": I64}
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    for hook in HOOKS:
        name = "mdt_op_score_" + hook
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m and m.group(1) == "mdt_status", f"{name} is not declared in include/mdt_hip_debug.h"
        want = [V if "*" in a else ctype[a.split()[0]] for a in (" ".join(a.split()) for a in m.group(2).split(","))]
        assert table[name] == (I32, want), name
        assert hasattr(_lib.load(), name)
    args = lambda name: [a.split()[-1].lstrip("*") for a in re.search(name + r"\s*\(([^)]*)\)", _header()).group(1).split(",")]
    assert args("mdt_op_score_prep") == ["x0", "noise", "sigmas", "S", "K", "M", "B", "Ta", "A", "D", "sd", "WaT", "ba", "y", "noised",
                                         "sig_rows", "ctx_sig", "stream"]
    assert args("mdt_op_score_repeat") == ["tok", "tok2", "goal", "B", "S", "w1", "w2", "wg", "tok_o", "tok2_o", "goal_o", "stream"]
    assert args("mdt_op_score_reduce") == ["F", "x0", "noise", "sigmas", "weights", "B", "S", "K", "M", "E", "sd", "score", "stream"]
