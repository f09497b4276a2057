"""The four ``*_multi`` sampler entries (K action chunks per observation, include/mdt_hip.h) as far as they can be seen without a
device: exported with the header's prototypes -- each the ``_opt`` entry of its family with ``int32_t candidates`` after
``batch`` -- bound in _lib.SYMBOLS with matching ctypes, and what they refuse before they touch a device, status and
mdt_last_error text per cause and entry, against a table recorded from the library (as tests/test_cpu_sampler_refusals.py does
for the eighteen other entries).  mdt_sample_opts keeps its two sizes: the refusal that quotes them is in the table."""
import ctypes as C
import os
import re

import pytest

from mdt_policy_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = {"mdt_sample_ddim_multi": "mdt_sample_ddim_opt", "mdt_sample_ddim_dev_multi": "mdt_sample_ddim_dev_opt",
         "mdt_sample_multi": "mdt_sample_opt", "mdt_sample_dev_multi": "mdt_sample_dev_opt"}
HEUN = _lib.SAMPLER_KIND["heun"]
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read
HANDLE = C.addressof(_HANDLE)
SIZE = C.sizeof(_lib.SampleOpts)
SIGMAS = (C.c_float * 4)(80.0, 10.0, 1.0, 0.0)

# recorded from the library; (mdt_status, mdt_last_error) per cause and entry
TABLE = {
    "null handle": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim: bad argument"),
                    "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim: bad argument"),
                    "mdt_sample_multi": (1, "mdt_sample: bad argument"),
                    "mdt_sample_dev_multi": (1, "mdt_sample: bad argument")},
    "null handle, opts.cond_lambda 3": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim_multi: null handle"),
                                        "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim_dev_multi: null handle"),
                                        "mdt_sample_multi": (1, "mdt_sample_multi: null handle"),
                                        "mdt_sample_dev_multi": (1, "mdt_sample_dev_multi: null handle")},
    "null sigmas": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim_multi: null sigmas"),
                    "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim_dev_multi: null sigmas"),
                    "mdt_sample_multi": (1, "mdt_sample_multi: null sigmas"),
                    "mdt_sample_dev_multi": (1, "mdt_sample_dev_multi: null sigmas")},
    "candidates 0": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim_multi: candidates is 0, must be >= 1"),
                     "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim_dev_multi: candidates is 0, must be >= 1"),
                     "mdt_sample_multi": (1, "mdt_sample_multi: candidates is 0, must be >= 1"),
                     "mdt_sample_dev_multi": (1, "mdt_sample_dev_multi: candidates is 0, must be >= 1")},
    "candidates -1": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim_multi: candidates is -1, must be >= 1"),
                      "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim_dev_multi: candidates is -1, must be >= 1"),
                      "mdt_sample_multi": (1, "mdt_sample_multi: candidates is -1, must be >= 1"),
                      "mdt_sample_dev_multi": (1, "mdt_sample_dev_multi: candidates is -1, must be >= 1")},
    "candidates 0, null handle": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim: bad argument"),
                                  "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim: bad argument"),
                                  "mdt_sample_multi": (1, "mdt_sample: bad argument"),
                                  "mdt_sample_dev_multi": (1, "mdt_sample: bad argument")},
    "batch 0": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim: bad argument"),
                "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim: bad argument"),
                "mdt_sample_multi": (1, "mdt_sample: bad argument"),
                "mdt_sample_dev_multi": (1, "mdt_sample: bad argument")},
    "opts.size": {"mdt_sample_ddim_multi": (1, "mdt_sample_ddim_multi: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without "
                                               "the pin)"),
                  "mdt_sample_ddim_dev_multi": (1, "mdt_sample_ddim_dev_multi: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 "
                                                   "without the pin)"),
                  "mdt_sample_multi": (1, "mdt_sample_multi: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without the pin)"),
                  "mdt_sample_dev_multi": (1, "mdt_sample_dev_multi: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without the "
                                              "pin)")},
    "pin_known without pin_keep": {n: (1, f"{n}: opts.pin_known is set and opts.pin_keep is null: a pin needs both") for n in MULTI},
    "record on ddim": {n: (1, f"{n}: opts.record: the DDIM head keeps no per-step record") for n in MULTI if "ddim" in n},
}


def opts(size=SIZE, lam=1.0, lo=None, hi=None, record=None, tree=None, known=None, keep=None):
    return _lib.SampleOpts(size, lam, lo, hi, record, tree, known, keep)


def observe(name, handle=None, sigmas=True, n_steps=3, batch=2, candidates=3, o=None):
    """The entry with the arguments in the header's order; pointers are integers or None: no device is needed."""
    sig = None if not sigmas else (PTR if "_dev" in name else SIGMAS)
    mid = (sig, n_steps) if "ddim" in name else (HEUN, None, sig, n_steps, None, 0)
    st = getattr(_lib.load(), name)(handle, None, None, None, _lib.MODALITY["lang"], PTR, *mid, batch, candidates, PTR, None,
                                    None if o is None else C.byref(o), None)
    return st, _lib.load().mdt_last_error().decode("utf-8", "replace")


CAUSES = {
    "null handle": (list(MULTI), {}),
    "null handle, opts.cond_lambda 3": (list(MULTI), dict(o=opts(lam=3.0))),
    "null sigmas": (list(MULTI), dict(handle=HANDLE, sigmas=False)),
    "candidates 0": (list(MULTI), dict(handle=HANDLE, candidates=0)),
    "candidates -1": (list(MULTI), dict(handle=HANDLE, candidates=-1)),
    "candidates 0, null handle": (list(MULTI), dict(candidates=0)),
    "batch 0": (list(MULTI), dict(handle=HANDLE, batch=0)),
    "opts.size": (list(MULTI), dict(o=opts(size=SIZE - 8))),
    "pin_known without pin_keep": (list(MULTI), dict(o=opts(known=PTR))),
    "record on ddim": ([n for n in MULTI if "ddim" in n], dict(o=opts(record=PTR))),
}


def test_the_table_names_every_entry_and_cause():
    assert set(TABLE) == set(CAUSES)
    for cause, (entries, _) in CAUSES.items():
        assert sorted(TABLE[cause]) == sorted(entries), cause


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_refusals_are_the_recorded_ones(cause):
    entries, kw = CAUSES[cause]
    got = {name: observe(name, **kw) for name in entries}
    assert got == TABLE[cause]


def test_a_refusal_names_the_entry_and_the_field():
    for name in MULTI:
        st, msg = observe(name, handle=HANDLE, candidates=0)
        assert st == 1 and name in msg and "candidates" in msg, msg


def _declared(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/mdt_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_four_symbols_are_exported_with_the_headers_prototypes():
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip.h")).read(), flags=re.S)
    table = {n: argt for n, _, argt in _lib.SYMBOLS}
    for name, base in MULTI.items():
        assert hasattr(lib, name), name
        args, opt = _declared(hdr, name), _declared(hdr, base)
        # the _opt entry's arguments with `int32_t candidates` right after `int64_t batch`
        at = opt.index("int64_t batch")
        assert args == opt[:at + 1] + ["int32_t candidates"] + opt[at + 1:], name
        assert len(table[name]) == len(args), name
        assert table[name] == table[base][:at + 1] + [C.c_int32] + table[base][at + 1:], name


def test_the_options_struct_did_not_grow():
    assert C.sizeof(_lib.SampleOpts) == 56 and _lib.SampleOpts.pin_known.offset == 40
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    body = re.search(r"typedef struct mdt_sample_opts \{(.*?)\} mdt_sample_opts;", hdr, flags=re.S).group(1)
    assert "candidates" not in body
