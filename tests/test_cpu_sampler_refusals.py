"""What every sampler entry point refuses before it touches a device: status and mdt_last_error text of each of the 18 entries,
per cause, against a table recorded from the library before the entries were rebuilt as adapters over one request struct.  The
table pins which entry name a message carries, the plain / guided wording and the order of the checks.

Reachable without a device: a null handle; null sigmas; n_steps out of range on the entries that check it before they read the
handle (the guided twins read it first, for the goal token: not here); every check of mdt_sample_opts alone.  The guided
twins check the handle before the schedule, so their 'null sigmas' rows record the null handle's refusal: null sigmas itself
cannot be observed on them without a device.  A null ``tree`` on
the four mdt_sample_sde_tree* entries is refused only after the handle's action shape was read: tests/test_gpu_sampler_entries.py
holds that one."""
import ctypes as C

import pytest

from mdt_policy_amd import _lib
from tests import raw_sampler as raw

HEUN, SDE = _lib.SAMPLER_KIND["heun"], _lib.SAMPLER_KIND["dpmpp_sde"]
_BUF = C.create_string_buffer(1 << 16)   # host memory behind every non-null pointer: nothing here is ever launched
PTR = (C.addressof(_BUF) + 15) & ~15
_HANDLE = C.create_string_buffer(1 << 20)  # a non-null handle for the checks that come before its first read
HANDLE = C.addressof(_HANDLE)
SIZE = C.sizeof(_lib.SampleOpts)
SIGMAS = (C.c_float * 4)(80.0, 10.0, 1.0, 0.0)
SRC = _lib.BrownianSource(PTR, 1, 0, 0.0, 0.0, 1e-6)

# recorded from the library as it was before this file was added; (mdt_status, mdt_last_error) per cause and entry
TABLE = {'null handle': {'mdt_sample_ddim': (1, 'mdt_sample_ddim: bad argument'),
                 'mdt_sample_ddim_guided': (1, 'mdt_sample_ddim_guided: null handle'),
                 'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim: bad argument'),
                 'mdt_sample_ddim_dev': (1, 'mdt_sample_ddim: bad argument'),
                 'mdt_sample_ddim_dev_guided': (1, 'mdt_sample_ddim_dev_guided: null handle'),
                 'mdt_sample_ddim_dev_opt': (1, 'mdt_sample_ddim: bad argument'),
                 'mdt_sample': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_guided': (1, 'mdt_sample_guided: null handle'),
                 'mdt_sample_opt': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_dev': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_dev_guided': (1, 'mdt_sample_dev_guided: null handle'),
                 'mdt_sample_dev_opt': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_sde_tree': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_sde_tree_guided': (1, 'mdt_sample_sde_tree_guided: null handle'),
                 'mdt_sample_sde_tree_dev': (1, 'mdt_sample: bad argument'),
                 'mdt_sample_sde_tree_dev_guided': (1, 'mdt_sample_sde_tree_dev_guided: null handle'),
                 'mdt_sample_dpm_adaptive': (1, 'mdt_sample_dpm_adaptive: bad argument'),
                 'mdt_sample_dpm_adaptive_guided': (1, 'mdt_sample_dpm_adaptive_guided: null handle')},
 'null handle, lambda 1': {'mdt_sample_ddim_guided': (1, 'mdt_sample_ddim_guided: null handle'),
                           'mdt_sample_ddim_dev_guided': (1, 'mdt_sample_ddim_dev_guided: null handle'),
                           'mdt_sample_guided': (1, 'mdt_sample_guided: null handle'),
                           'mdt_sample_dev_guided': (1, 'mdt_sample_dev_guided: null handle'),
                           'mdt_sample_sde_tree_guided': (1, 'mdt_sample_sde_tree_guided: null handle'),
                           'mdt_sample_sde_tree_dev_guided': (1, 'mdt_sample_sde_tree_dev_guided: null handle'),
                           'mdt_sample_dpm_adaptive_guided': (1, 'mdt_sample_dpm_adaptive_guided: null handle')},
 'null handle, opts.cond_lambda 3': {'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: null handle'),
                                     'mdt_sample_ddim_dev_opt': (1, 'mdt_sample_ddim_dev_opt: null handle'),
                                     'mdt_sample_opt': (1, 'mdt_sample_opt: null handle'),
                                     'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: null handle')},
 'null sigmas': {'mdt_sample_ddim': (1, 'mdt_sample_ddim: null sigmas'),
                 'mdt_sample_ddim_guided': (1, 'mdt_sample_ddim_guided: null handle'),
                 'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: null sigmas'),
                 'mdt_sample_ddim_dev': (1, 'mdt_sample_ddim_dev: null sigmas'),
                 'mdt_sample_ddim_dev_guided': (1, 'mdt_sample_ddim_dev_guided: null handle'),
                 'mdt_sample_ddim_dev_opt': (1, 'mdt_sample_ddim_dev_opt: null sigmas'),
                 'mdt_sample': (1, 'mdt_sample: null sigmas'),
                 'mdt_sample_guided': (1, 'mdt_sample_guided: null handle'),
                 'mdt_sample_opt': (1, 'mdt_sample_opt: null sigmas'),
                 'mdt_sample_dev': (1, 'mdt_sample_dev: null sigmas'),
                 'mdt_sample_dev_guided': (1, 'mdt_sample_dev_guided: null handle'),
                 'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: null sigmas'),
                 'mdt_sample_sde_tree': (1, 'mdt_sample_sde_tree: null sigmas'),
                 'mdt_sample_sde_tree_guided': (1, 'mdt_sample_sde_tree_guided: null handle'),
                 'mdt_sample_sde_tree_dev': (1, 'mdt_sample_sde_tree_dev: null sigmas'),
                 'mdt_sample_sde_tree_dev_guided': (1, 'mdt_sample_sde_tree_dev_guided: null handle')},
 'n_steps 0': {'mdt_sample_ddim': (1, 'n_steps must be 1..64'),
               'mdt_sample_ddim_opt': (1, 'n_steps must be 1..64'),
               'mdt_sample_ddim_dev': (1, 'n_steps must be 1..64'),
               'mdt_sample_ddim_dev_opt': (1, 'n_steps must be 1..64'),
               'mdt_sample': (1, 'mdt_sample: n_steps must be 1..64'),
               'mdt_sample_opt': (1, 'mdt_sample: n_steps must be 1..64'),
               'mdt_sample_dev': (1, 'mdt_sample: n_steps must be 1..64'),
               'mdt_sample_dev_opt': (1, 'mdt_sample: n_steps must be 1..64'),
               'mdt_sample_sde_tree': (1, 'mdt_sample: n_steps must be 1..64'),
               'mdt_sample_sde_tree_dev': (1, 'mdt_sample: n_steps must be 1..64')},
 'n_steps 1000': {'mdt_sample_ddim': (1, 'n_steps must be 1..64'),
                  'mdt_sample_ddim_opt': (1, 'n_steps must be 1..64'),
                  'mdt_sample_ddim_dev': (1, 'n_steps must be 1..64'),
                  'mdt_sample_ddim_dev_opt': (1, 'n_steps must be 1..64'),
                  'mdt_sample': (1, 'mdt_sample: n_steps must be 1..64'),
                  'mdt_sample_opt': (1, 'mdt_sample: n_steps must be 1..64'),
                  'mdt_sample_dev': (1, 'mdt_sample: n_steps must be 1..64'),
                  'mdt_sample_dev_opt': (1, 'mdt_sample: n_steps must be 1..64'),
                  'mdt_sample_sde_tree': (1, 'mdt_sample: n_steps must be 1..64'),
                  'mdt_sample_sde_tree_dev': (1, 'mdt_sample: n_steps must be 1..64')},
 'opts.size': {'mdt_sample_ddim_opt': (1,
                                       'mdt_sample_ddim_opt: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without the '
                                       'pin)'),
               'mdt_sample_ddim_dev_opt': (1,
                                           'mdt_sample_ddim_dev_opt: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without '
                                           'the pin)'),
               'mdt_sample_opt': (1, 'mdt_sample_opt: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without the pin)'),
               'mdt_sample_dev_opt': (1,
                                      'mdt_sample_dev_opt: opts.size is 48, sizeof(mdt_sample_opts) is 56 (40 without the pin)')},
 'opts.cond_lambda nan': {'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: opts.cond_lambda must be finite'),
                          'mdt_sample_ddim_dev_opt': (1, 'mdt_sample_ddim_dev_opt: opts.cond_lambda must be finite'),
                          'mdt_sample_opt': (1, 'mdt_sample_opt: opts.cond_lambda must be finite'),
                          'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: opts.cond_lambda must be finite')},
 'lo without hi': {'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_ddim_dev_opt': (1,
                                               'mdt_sample_ddim_dev_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_opt': (1, 'mdt_sample_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: opts.lo and opts.hi must both be set or both be null')},
 'hi without lo': {'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_ddim_dev_opt': (1,
                                               'mdt_sample_ddim_dev_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_opt': (1, 'mdt_sample_opt: opts.lo and opts.hi must both be set or both be null'),
                   'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: opts.lo and opts.hi must both be set or both be null')},
 'pin_known without pin_keep': {'mdt_sample_ddim_opt': (1,
                                                        'mdt_sample_ddim_opt: opts.pin_known is set and opts.pin_keep is null: a '
                                                        'pin needs both'),
                                'mdt_sample_ddim_dev_opt': (1,
                                                            'mdt_sample_ddim_dev_opt: opts.pin_known is set and opts.pin_keep is '
                                                            'null: a pin needs both'),
                                'mdt_sample_opt': (1,
                                                   'mdt_sample_opt: opts.pin_known is set and opts.pin_keep is null: a pin needs '
                                                   'both'),
                                'mdt_sample_dev_opt': (1,
                                                       'mdt_sample_dev_opt: opts.pin_known is set and opts.pin_keep is null: a '
                                                       'pin needs both')},
 'pin_keep without pin_known': {'mdt_sample_ddim_opt': (1,
                                                        'mdt_sample_ddim_opt: opts.pin_keep is set and opts.pin_known is null: a '
                                                        'pin needs both'),
                                'mdt_sample_ddim_dev_opt': (1,
                                                            'mdt_sample_ddim_dev_opt: opts.pin_keep is set and opts.pin_known is '
                                                            'null: a pin needs both'),
                                'mdt_sample_opt': (1,
                                                   'mdt_sample_opt: opts.pin_keep is set and opts.pin_known is null: a pin needs '
                                                   'both'),
                                'mdt_sample_dev_opt': (1,
                                                       'mdt_sample_dev_opt: opts.pin_keep is set and opts.pin_known is null: a '
                                                       'pin needs both')},
 'record on ddim': {'mdt_sample_ddim_opt': (1, 'mdt_sample_ddim_opt: opts.record: the DDIM head keeps no per-step record'),
                    'mdt_sample_ddim_dev_opt': (1,
                                                'mdt_sample_ddim_dev_opt: opts.record: the DDIM head keeps no per-step record')},
 'tree on ddim': {'mdt_sample_ddim_opt': (1,
                                          'mdt_sample_ddim_opt: opts.tree is the noise of MDT_SAMPLER_DPMPP_SDE; DDIM draws '
                                          'none'),
                  'mdt_sample_ddim_dev_opt': (1,
                                              'mdt_sample_ddim_dev_opt: opts.tree is the noise of MDT_SAMPLER_DPMPP_SDE; DDIM '
                                              'draws none')},
 'tree, kind heun': {'mdt_sample_opt': (1, 'mdt_sample_opt: opts.tree is the noise of MDT_SAMPLER_DPMPP_SDE (kind 2)'),
                     'mdt_sample_dev_opt': (1, 'mdt_sample_dev_opt: opts.tree is the noise of MDT_SAMPLER_DPMPP_SDE (kind 2)')}}


def opts(size=SIZE, lam=1.0, lo=None, hi=None, record=None, tree=None, known=None, keep=None):
    return _lib.SampleOpts(size, lam, lo, hi, record, tree, known, keep)


def observe(name, handle=None, sigmas=True, n_steps=3, lam=3.0, o=None, kind=HEUN):
    sig = None if not sigmas else (PTR if raw.device_schedule(name) else SIGMAS)
    st = raw.status(name, handle, None, None, None, _lib.MODALITY["lang"], PTR, 2, PTR, None, None, sigmas=sig, n_steps=n_steps,
                    kind=kind, tree=SRC, lam=lam, opts=o, sigma_min=1.0, sigma_max=80.0)
    return st, raw.last_error()


def _is(*suffixes):
    return [n for n in raw.ENTRIES if n.endswith(suffixes)]


OPT = _is("_opt")
GUIDED = _is("_guided")
UNGUIDED_FIXED = [n for n in raw.FIXED if n not in GUIDED]
DDIM_OPT = [n for n in OPT if "ddim" in n]
PLAN_OPT = [n for n in OPT if "ddim" not in n]

# cause -> (entries, keyword arguments of observe)
CAUSES = {
    "null handle": (raw.ENTRIES, {}),
    "null handle, lambda 1": (GUIDED, dict(lam=1.0)),
    "null handle, opts.cond_lambda 3": (OPT, dict(o=opts(lam=3.0))),
    "null sigmas": (raw.FIXED, dict(sigmas=False)),
    "n_steps 0": (UNGUIDED_FIXED, dict(handle=HANDLE, n_steps=0)),
    "n_steps 1000": (UNGUIDED_FIXED, dict(handle=HANDLE, n_steps=1000)),
    "opts.size": (OPT, dict(o=opts(size=SIZE - 8))),
    "opts.cond_lambda nan": (OPT, dict(o=opts(lam=float("nan")))),
    "lo without hi": (OPT, dict(o=opts(lo=PTR))),
    "hi without lo": (OPT, dict(o=opts(hi=PTR))),
    "pin_known without pin_keep": (OPT, dict(o=opts(known=PTR))),
    "pin_keep without pin_known": (OPT, dict(o=opts(keep=PTR))),
    "record on ddim": (DDIM_OPT, dict(o=opts(record=PTR))),
    "tree on ddim": (DDIM_OPT, dict(o=opts(tree=C.pointer(SRC)))),
    "tree, kind heun": (PLAN_OPT, dict(o=opts(tree=C.pointer(SRC)))),
}


def test_the_table_names_every_entry_and_cause():
    assert len(raw.ENTRIES) == 18 and set(TABLE) == set(CAUSES)
    for cause, (entries, _) in CAUSES.items():
        assert sorted(TABLE[cause]) == sorted(entries), cause
    assert all(hasattr(_lib.load(), n) for n in raw.ENTRIES)


@pytest.mark.parametrize("cause", sorted(CAUSES))
def test_refusals_are_the_recorded_ones(cause):
    entries, kw = CAUSES[cause]
    got = {name: observe(name, **kw) for name in entries}
    assert got == TABLE[cause]
