"""The four steer-kernel hooks (include/mdt_hip_debug.h: mdt_op_steer_seed, mdt_op_steer_step, mdt_op_steer_first,
mdt_op_steer_plan) as far as they can be seen without a device: exported with the header's prototypes, bound in _lib.SYMBOLS with
matching ctypes, and every refusal -- MDT_ERR_INVALID_ARG before anything is launched, the text naming the hook and the field."""
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


def seed(F=PTR, x=PTR, known=PTR, weight=PTR, sigma=2.0, sd=0.5, N=70, D=PTR, e=PTR, dF=PTR):
    return _lib.load().mdt_op_steer_seed(F, x, known, weight, sigma, sd, N, D, e, dF, None)


def step(small=PTR, e=PTR, D=PTR, x_in=PTR, sigma=2.0, sd=0.5, scale=5.0, ratio=0.25, coef=0.75, lo=None, hi=None, A=7,
         sigma_next=0.5, N=70, R=1, x_out=PTR, sig_rows=PTR):
    return _lib.load().mdt_op_steer_step(small, e, D, x_in, sigma, sd, scale, ratio, coef, lo, hi, A, sigma_next, N, R, x_out,
                                         sig_rows, None)


def first(x_T=PTR, n0=None, cn=0.0, sigma0=80.0, N=70, R=1, X=PTR, Y=PTR, hist=PTR, sig_rows=PTR):
    return _lib.load().mdt_op_steer_first(x_T, n0, cn, sigma0, N, R, X, Y, hist, sig_rows, None)


def plan(ev="row", small=PTR, e=PTR, D=PTR, Y=PTR, X=PTR, x_out=PTR, y_out=None, hist=PTR, noise=None, lo=None, hi=None, rec=None,
         sig_rows=PTR, N=70, R=1, sd=0.5, scale=5.0, n_noise=0, A=7, sigma=2.0):
    row = _lib.SamplerEval()
    row.sigma, row.sigma_next = sigma, 0.5
    return _lib.load().mdt_op_steer_plan(C.byref(row) if ev == "row" else None, small, e, D, Y, X, x_out, y_out, hist, noise, lo, hi,
                                         rec, sig_rows, N, R, sd, scale, n_noise, A, None)


HOOKS = {"seed": seed, "step": step, "first": first, "plan": plan}
SIZES = {"N -1": (dict(N=-1), "N"), "R -1": (dict(R=-1), "R"), "N 0 and R 0": (dict(N=0, R=0), "N + R")}
BOUNDS = {"lo without hi": (dict(lo=PTR), "hi"), "hi without lo": (dict(hi=PTR), "lo"), "A 0": (dict(A=0), "A"),
          "bounds with N no multiple of A": (dict(lo=PTR, hi=PTR, N=69), "N")}


def positive(name, field=None):
    return {f"{name} {v}": ({name: v}, field or name) for v in (0.0, -1.0, NAN, INF)}


def nulls(*names):
    return {f"null {n}": ({n: None}, n) for n in names}


# hook -> cause -> (arguments, the field the message names)
CAUSES = {
    "seed": {**nulls("F", "x", "known", "weight", "D", "e", "dF"), "N 0": (dict(N=0), "N"), "N -1": (dict(N=-1), "N"),
             **positive("sigma"), **positive("sd")},
    "step": {**nulls("small", "e", "D", "x_in", "x_out", "sig_rows"), **SIZES, **BOUNDS, **positive("sigma"), **positive("sd")},
    "first": {**nulls("x_T", "X", "Y", "hist", "sig_rows"), **SIZES, **positive("sigma0")},
    "plan": {**nulls("ev", "small", "e", "D", "Y", "X", "x_out", "hist", "sig_rows"), **SIZES, **BOUNDS,
             "n_noise -1": (dict(n_noise=-1), "n_noise"), **positive("sigma", "ev->sigma"), **positive("sd")},
}
ALL = [(h, c) for h in sorted(CAUSES) for c in sorted(CAUSES[h])]


@pytest.mark.parametrize("hook,cause", ALL, ids=[f"{h}: {c}" for h, c in ALL])
def test_a_refusal_names_the_hook_and_the_field(hook, cause):
    kw, field = CAUSES[hook][cause]
    st = HOOKS[hook](**kw)
    msg = _lib.load().mdt_last_error().decode("utf-8", "replace")
    assert st == INVALID and msg.startswith(f"mdt_op_steer_{hook}: ") and field in msg[len(f"mdt_op_steer_{hook}: "):], (st, msg)


def test_the_messages_say_what_was_wrong():
    last = lambda: _lib.load().mdt_last_error().decode()
    assert seed(known=None) == INVALID and last() == "mdt_op_steer_seed: null known"
    assert step(N=-1) == INVALID and last() == "mdt_op_steer_step: N is -1, must be >= 0"
    assert first(N=0, R=0) == INVALID and last() == "mdt_op_steer_first: N + R is 0: nothing to launch over"
    assert plan(lo=PTR) == INVALID and last() == "mdt_op_steer_plan: null hi: the bounds lo and hi come together"
    assert plan(lo=PTR, hi=PTR, N=69) == INVALID and \
        last() == "mdt_op_steer_plan: N is 69, no multiple of A = 7: the bounds are per column of rows of A"
    assert plan(sigma=0.0) == INVALID and last() == "mdt_op_steer_plan: ev->sigma is 0, must be finite and > 0"
    assert step(sd=INF) == INVALID and last() == "mdt_op_steer_step: sd is inf, must be finite and > 0"


def test_what_is_optional_is_not_asked_for():
    """Without elements no element pointer is read, without sigma rows no sig_rows: those nulls are refused only where they count.
    (Seen as the NEXT check's refusal: nothing here may reach a launch.)"""
    last = lambda: _lib.load().mdt_last_error().decode()
    assert step(small=None, e=None, D=None, x_in=None, x_out=None, N=0, R=5, sd=0.0) == INVALID and "sd" in last()
    assert step(sig_rows=None, R=0, sd=0.0) == INVALID and "sd" in last()
    assert first(x_T=None, X=None, Y=None, hist=None, N=0, R=5, sigma0=0.0) == INVALID and "sigma0" in last()
    assert plan(small=None, e=None, D=None, Y=None, X=None, x_out=None, hist=None, N=0, R=5, sd=0.0) == INVALID and "sd" in last()
    assert plan(y_out=None, noise=None, rec=None, n_noise=3, sd=0.0) == INVALID and "sd" in last()   # null noise with rows: allowed


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip_debug.h")).read(), flags=re.S)


def test_the_symbols_are_exported_with_the_headers_prototypes():
    V, I32, I64, F = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    ctype = {"float": F, "int32_t": I32, "int64_t": I64}
    table = {n: (res, argt) for n, res, argt in _lib.SYMBOLS}
    for hook in HOOKS:
        name = "mdt_op_steer_" + hook
        m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
        assert m and m.group(1) == "mdt_status", f"{name} is not declared in include/mdt_hip_debug.h"
        want = []
        for a in (" ".join(a.split()) for a in m.group(2).split(",")):
            if a.startswith("const mdt_sampler_eval *"):
                want.append(C.POINTER(_lib.SamplerEval))
            elif "*" in a:
                want.append(V)
            else:
                want.append(ctype[a.split()[0]])
        assert table[name] == (I32, want), name
        assert hasattr(_lib.load(), name)
    assert C.sizeof(_lib.SamplerEval) == 4 * (2 + 10 + 11 + 1 + 2 + 1 + 1 + 1 + 1 + 1 + 1)
