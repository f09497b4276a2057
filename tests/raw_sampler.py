"""Any sampler entry point of libmdt_hip.so called by its name with explicit arguments: what a C client's call looks like, for
the tests that compare one entry with another or with the Python facade (which only ever takes the ``_opt`` entries).

``status`` lays the arguments out as include/mdt_hip.h declares them and returns the mdt_status (pointers are integers or None:
it needs no device); ``run`` prepares a model's inputs the way HipEngine does, calls, and returns ``out``."""
import ctypes as C

from mdt_policy_amd import _lib

FIXED = [fam + dev + twin for fam in ("mdt_sample_ddim", "mdt_sample") for dev in ("", "_dev") for twin in ("", "_guided", "_opt")] + \
        ["mdt_sample_sde_tree" + dev + twin for dev in ("", "_dev") for twin in ("", "_guided")]
ADAPTIVE = ["mdt_sample_dpm_adaptive", "mdt_sample_dpm_adaptive_guided"]
ENTRIES = FIXED + ADAPTIVE


def family(name):
    for key, fam in (("dpm_adaptive", "adaptive"), ("sde_tree", "tree"), ("ddim", "ddim")):
        if key in name:
            return fam
    return "plan"


def device_schedule(name):
    return "_dev" in name


def last_error():
    return _lib.load().mdt_last_error().decode("utf-8", "replace")


def _ref(struct):
    return None if struct is None else C.byref(struct)


def status(name, handle, tok, tok2, goal, modality, x_T, batch, out, ctx, stream, sigmas=None, n_steps=0, kind=0, params=None,
           noise=None, n_noise=0, tree=None, lam=None, opts=None, sigma_min=0., sigma_max=0., info=None):
    """The entry ``name`` with the arguments its family takes (the others are not read): ``lam`` goes to a ``_guided`` entry,
    ``opts`` (a _lib.SampleOpts or None) to an ``_opt`` one."""
    fam = family(name)
    mid = {"ddim": (sigmas, n_steps), "plan": (kind, _ref(params), sigmas, n_steps, noise, n_noise),
           "tree": (_ref(params), sigmas, n_steps, _ref(tree)), "adaptive": (sigma_min, sigma_max, _ref(params))}[fam]
    tail = (_ref(opts),) if name.endswith("_opt") else (lam,) if name.endswith("_guided") else ()
    if fam == "adaptive":
        tail += (_ref(info),)
    return getattr(_lib.load(), name)(handle, tok, tok2, goal, modality, x_T, *mid, batch, out, ctx, *tail, stream)


def run(name, model, state, x_T, goal, sigmas, n_steps=None, kind=None, params=None, noise=None, tree=None, lam=None, opts=None):
    """``out`` of the fixed-schedule entry ``name`` on a GCDenoiser's handle: ``kind`` a gc_sampling name, ``params`` its keyword
    arguments, ``noise`` None or (n_noise, B, Ta, A), ``tree`` a _lib.BrownianSource.  The schedule goes to the device for a
    ``_dev`` entry.  Raises _lib.MDTHipError like the facade; synchronises, so nothing it built has to outlive it."""
    import torch
    eng = model._engine(state=state)
    eng.sync_params()
    tok, tok2, B = eng._tokens(state)
    g = eng._goal(model.inner_model._goals(goal, False), B)
    x = eng._in(x_T, (B, eng.Ta, eng.A))
    nz = None if noise is None else eng._in(noise, (-1, B, eng.Ta, eng.A))
    out = torch.empty((B, eng.Ta, eng.A), device=x.device, dtype=torch.float32)
    vals = [float(v) for v in sigmas]
    if device_schedule(name):
        sig = torch.tensor(vals, device=x.device, dtype=torch.float32)
        sig_arg = sig.data_ptr()
    else:
        sig = sig_arg = (C.c_float * len(vals))(*vals)
    eng.ctx_generation += 1
    st = status(name, eng.handle, tok.data_ptr(), None if tok2 is None else tok2.data_ptr(), g.data_ptr(), eng._modality(state),
                x.data_ptr(), B, out.data_ptr(), None, eng._stream(), sigmas=sig_arg,
                n_steps=len(vals) - 1 if n_steps is None else int(n_steps), kind=0 if kind is None else _lib.SAMPLER_KIND[kind],
                params=_lib.sampler_params(**(params or {})), noise=None if nz is None else nz.data_ptr(),
                n_noise=0 if nz is None else nz.shape[0], tree=tree, lam=lam, opts=opts)
    if st != 0:
        raise _lib.MDTHipError(st, last_error())
    torch.cuda.synchronize()
    return out
