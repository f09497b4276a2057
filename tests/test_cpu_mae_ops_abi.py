"""The ops of include/mdt_mae.h as far as they can be seen without a device: the row and batch counts each entry point
refuses (a 32-bit row index, an (int) cast or a grid dimension cannot hold them) and the last it lets past its argument
checks, the four scratch formulas against the header's text, and the null-pointer and range refusals of every op.  Every call
below that may run on a machine with a GPU comes back before anything is enqueued: the pointers are FAKE."""
import ctypes as C
import os
import re

import pytest
import torch

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000   # an aligned address no call may dereference
LIMIT = 2 ** 31 - 1
EPS = C.c_float(1e-8)
ONE = C.c_float(1.0)

# the arguments of every op: "p" a pointer the op needs, "o" one that may be NULL, "M" the row / batch count, the rest as given
OPS = {
    "mdt_op_rms_fwd": ["p", "p", "p", "M", 8, EPS, None],
    "mdt_op_rms_bwd": ["p", "p", "p", "p", 0, "o", 0, "M", 8, EPS, "p", None],
    "mdt_op_rms_bwd_res": ["p", "p", "p", "p", "p", "o", 0, "M", 8, EPS, "p", None],
    "mdt_op_swiglu_fwd": ["p", "p", "M", 8, None],
    "mdt_op_swiglu_bwd": ["p", "p", "p", "M", 8, None],
    "mdt_op_scale_residual_fwd": ["p", "p", "p", "p", "M", 8, None],
    "mdt_op_scale_residual_bwd": ["p", "p", "p", "p", "p", "M", 8, "p", None],
    "mdt_op_scale_residual_rms_fwd": ["p", "p", "p", "p", "p", "p", "M", 8, EPS, None],
    "mdt_op_scale_residual_rms_bwd": ["p", "p", "p", "o", "p", "p", "p", "p", "p", "p", "M", 8, EPS, "p", None],
    "mdt_op_attn_mid_fwd": ["p", 48, "p", 16, "M", 1, 16, 16, ONE, None],
    "mdt_op_attn_mid_bwd": ["p", 48, "p", 16, "p", 16, "p", 48, "M", 1, 16, 16, ONE, None],
    "mdt_op_attn_long_fwd": ["p", 48, "p", 16, "p", "M", 1, 16, 16, ONE, None],
    "mdt_op_attn_long_bwd": ["p", 48, "p", 16, "p", "p", 16, "p", 48, "M", 1, 16, 16, ONE, "p", None],
    "mdt_op_patch_mse_fwd": ["p", "p", "p", "p", "p", "p", "M", 1, 1, 4, 4, None],
    "mdt_op_patch_mse_bwd": ["p", "p", "p", "p", "p", "p", "M", 1, 1, 4, 4, None],
}
SCRATCH = ["mdt_op_rms_bwd_scratch", "mdt_op_scale_residual_bwd_scratch", "mdt_op_scale_residual_rms_bwd_scratch",
           "mdt_op_attn_long_bwd_scratch"]
UNALIGNED_OK = {"mdt_op_scale_residual_bwd": (4,), "mdt_op_scale_residual_rms_bwd": (8, 9)}   # dgamma; d_gamma, d_gnorm: a column sum's outputs


def args(name, M=4, null=None, change=None):
    """The op's arguments with M rows; null: the index of the pointer to pass as NULL; change: {index: value}."""
    out = []
    for i, a in enumerate(OPS[name]):
        v = FAKE if a in ("p", "o") else M if a == "M" else a
        out.append(None if i == null else (change or {}).get(i, v))
    return out


def test_the_table_covers_the_header():
    """The fifteen entry points above and the four scratch functions are what include/mdt_mae.h declares, each bound with as many
    arguments as the table gives."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_mae.h")).read(), flags=re.S)
    declared = {n: len(a.split(",")) for n, a in re.findall(r"\b(?:mdt_status|int64_t)\s+(mdt_op_\w+)\s*\(([^)]*)\)\s*;", src)}
    assert set(declared) == set(OPS) | set(SCRATCH) and len(declared) == 19
    table = {n: a for n, _, a in _lib.SYMBOLS}
    for n, a in OPS.items():
        assert declared[n] == len(a) == len(table[n]), n


@pytest.mark.parametrize("name", sorted(OPS))
def test_one_row_too_many_is_refused_with_a_message_that_names_the_limit(name):
    lib = _lib.load()
    st = getattr(lib, name)(*args(name, M=LIMIT + 1))
    msg = lib.mdt_last_error().decode()
    assert st == (1 if "patch" in name else 2) and name in msg and "2147483647" in msg, (st, msg)
    assert getattr(lib, name)(*args(name, M=2 ** 40)) == st
    assert getattr(lib, name)(*args(name, M=2 ** 63 - 1)) == st


@pytest.mark.parametrize("name", ["mdt_op_swiglu_fwd", "mdt_op_swiglu_bwd"])
def test_swiglu_refuses_more_elements_than_one_grid_dimension_of_blocks(name):
    lib = _lib.load()
    i = OPS[name].index("M") + 1
    assert getattr(lib, name)(*args(name, M=LIMIT, change={i: 257})) == 2
    assert "256 * 2147483647" in lib.mdt_last_error().decode()


@pytest.mark.parametrize("name", ["mdt_op_attn_long_fwd", "mdt_op_attn_long_bwd"])
def test_long_attention_counts_heads_and_query_blocks(name):
    lib = _lib.load()
    i = OPS[name].index("M")
    # B * H * ceil(T / 64) = 2^29 * 2 * 2 = 2^31 workgroups
    assert getattr(lib, name)(*args(name, M=2 ** 29, change={i + 1: 2, i + 3: 65})) == 2
    assert "2147483647" in lib.mdt_last_error().decode()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU: with one, the call would be launched")
@pytest.mark.parametrize("name", sorted(OPS))
def test_the_last_row_count_gets_past_the_argument_checks(name):
    """M = 2^31 - 1 reaches the launch: without a device that is MDT_ERR_HIP (4), not INVALID_ARG (1) or UNSUPPORTED (2)."""
    lib = _lib.load()
    st = getattr(lib, name)(*args(name, M=LIMIT))
    assert st == 4, (name, st, lib.mdt_last_error())


def test_the_scratch_formulas_are_the_headers():
    """include/mdt_mae.h states each as `name(args) = expression` with ceil(a / b); evaluated here and compared with the library
    at row counts around every divisor and at the limit."""
    text = open(os.path.join(ROOT, "include", "mdt_mae.h")).read()
    stated = dict(re.findall(r"\*\s+(mdt_op_\w+_scratch)\([^)]*\)\s+=\s+(.+)", text))
    assert set(stated) == set(SCRATCH)
    lib = _lib.load()

    def value(name, **v):
        expr = re.sub(r"ceil\((\w+) / (\d+)\)", r"(-(-\1 // \2))", stated[name])
        return eval(expr, {"__builtins__": {}}, v)   # noqa: S307 -- the header's own arithmetic, names M D B H T only
    for M in (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4133, LIMIT):
        for D in (1, 4, 500, 512, 1024):
            for name in SCRATCH[:3]:
                assert getattr(lib, name)(M, D) == value(name, M=M, D=D), (name, M, D)
    assert lib.mdt_op_rms_bwd_scratch(5, 8) == 16 and lib.mdt_op_scale_residual_bwd_scratch(65, 8) == 16
    assert lib.mdt_op_scale_residual_rms_bwd_scratch(65, 8) == 32
    for B, H, T in ((1, 1, 1), (2, 2, 129), (3, 8, 4096), (LIMIT, 1, 64)):
        assert lib.mdt_op_attn_long_bwd_scratch(B, H, T) == value(SCRATCH[3], B=B, H=H, T=T) == B * H * T


@pytest.mark.parametrize("name", sorted(OPS))
def test_null_pointers_and_ranges_are_refused(name):
    """Every needed pointer NULL, one at a time; no rows; and the op's own ranges -- D, H, T, hd, the strides, R and P."""
    lib = _lib.load()
    fn = getattr(lib, name)
    for i, a in enumerate(OPS[name]):
        if a == "p":
            assert fn(*args(name, null=i)) == 1, (name, i)
            if "attn" in name and isinstance(OPS[name][i + 1], int):     # a pointer with a stride: both are checked
                assert fn(*args(name, change={i: FAKE + 4})) == 1, (name, i)
                assert fn(*args(name, change={i + 1: OPS[name][i + 1] + 2})) == 1, (name, i)
            elif "scale_residual" in name and i not in UNALIGNED_OK.get(name, ()):
                assert fn(*args(name, change={i: FAKE + 4})) == 1, (name, i)
    m = OPS[name].index("M")
    for M in (0, -1):
        assert fn(*args(name, M=M)) == 1, (name, M)
    if "attn" in name:
        long = "long" in name
        for change, st in (({m + 1: 0}, 1), ({m + 3: 0}, 1), ({m + 3: 4097 if long else 129}, 2), ({m + 2: 12}, 2), ({m + 2: 0}, 2)):
            assert fn(*args(name, change=change)) == st, (name, change)
        if name == "mdt_op_attn_mid_bwd":
            for hd, T, st in ((64, 81, 2), (48, 97, 2)):
                assert fn(*args(name, change={m + 2: hd, m + 3: T, 1: 3 * hd, 3: hd, 5: hd, 7: 3 * hd})) == st
                assert "LDS" in lib.mdt_last_error().decode()
    elif "patch" in name:
        for change in ({m + 1: 0}, {m + 2: 0}, {m + 4: 0}, {m + 3: 10}, {m + 3: 2}):    # X, C, P = 0; R % P; R < P
            assert fn(*args(name, change=change)) == 1, (name, change)
    else:
        wide = {"mdt_op_swiglu_fwd": None, "mdt_op_swiglu_bwd": None, "mdt_op_scale_residual_fwd": 1028,
                "mdt_op_scale_residual_bwd": 1028, "mdt_op_scale_residual_rms_fwd": 516, "mdt_op_scale_residual_rms_bwd": 516}.get(name, 513)
        for D in (0, -4) + ((wide,) if wide else ()) + ((6,) if "scale_residual" in name else ()):
            assert fn(*args(name, change={m + 1: D})) == 1, (name, D)
