"""Action bounds and the per-step record inside the native samplers on the MI355X (pytest -m gpu): mdt_sample_opt /
GCDenoiser.sample_native(bounds=, record=) against the package's host loops run with a scaler that only has ``clip_output`` (it
forces the host loop) and with a ``callback``.

Tolerances are those of the existing native-versus-host-loop tests of the same kind (tests/helpers.assert_close: rtol 1e-3, atol
1e-4 at every batch size; the guided cases test_gpu_guidance.tol; dpm_fast test_gpu_native_dpm._close, whose scaled atol applies
to n <= 5 only -- n = 7 here).

Bounds: the per-dimension 30 % / 70 % quantiles of the unclipped host-loop result of the same seed, so that every clip_output call
of the host loop changes a large share of the elements (asserted: >= 10 % at every call) and the clipped result is far from the
unclipped one (asserted: > 100 x the tolerance).  Two loops never call clip_output -- sample_dpmpp_2m and sample_dpm_fast take a
scaler and do not read it, here as in the reference (gc_sampling.py:699-734, 673-697) -- and sample_dpmpp_sde does not clip its
final step; for those two kinds the test asserts that the host loop made no clip_output call and that the native call with an
ActionBounds scaler still equals it."""
import ctypes as C
import math

import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests import raw_sampler as raw
from tests.helpers import ATOL, RTOL, assert_close, cfg_of, inputs_of, load_fixture, params_of

pytestmark = pytest.mark.gpu

N, SMIN, SMAX, NFE = 4, 1.0, 80.0, 7
KINDS = {"euler": dict(s_churn=1.0), "euler_ancestral": {}, "heun": dict(s_churn=1.0), "dpm_2": dict(s_churn=1.0),
         "dpm_2_ancestral": {}, "lms": {}, "dpmpp_2s": {}, "dpmpp_2s_ancestral": {}, "dpmpp_2m": {}, "dpmpp_sde": {},
         "dpm_fast": {}}
NEVER_CLIPS = ("dpmpp_2m", "dpm_fast")
_MODEL, _REFS = {}, {}


def ActionBounds(*args, **kw):  # noqa: N802 -- imported where it is used: without the feature every case fails on its own
    from mdt_policy_amd.utils.action_bounds import ActionBounds as cls
    return cls(*args, **kw)


def model_of():
    if "m" not in _MODEL:
        from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
        meta, _ = load_fixture("g7_samplers.npz")
        model = GCDenoiser(cfg_of(meta), sigma_data=0.5)
        model.load_state_dict(params_of(meta), strict=True)
        _MODEL["m"], _MODEL["meta"] = model.cuda().eval(), meta
    return _MODEL["m"], _MODEL["meta"]


def inputs(B):
    model, meta = model_of()
    state, goal, noise = inputs_of(dict(meta, B=B, input_seed=700 + B))
    state = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    return model, state, goal.cuda(), noise.cuda() * SMAX


class ClampOnly:
    """The reference's scaler as far as the samplers read it: clip_output (the same torch.clamp) and nothing else -- no
    clip_bounds, so every sampler runs its host loop.  Counts, per call, the share of elements the clamp changed."""

    def __init__(self, lo, hi):
        self.lo, self.hi, self.changed = lo, hi, []

    def clip_output(self, x):
        y = torch.clamp(x, self.lo.to(x.device), self.hi.to(x.device))
        self.changed.append(float((y != x).float().mean()))
        return y


def sched():
    return gs.get_sigmas_exponential(N, SMIN, SMAX)


def run(name, model, state, x, goal, sig, seed=11, **kw):
    """One seeded sampler call through gc_sampling.  dpmpp_sde gets pre-drawn noise rows handed out in call order."""
    g = gs
    torch.manual_seed(seed)
    kw = dict(KINDS[name], **kw)
    if name == "dpmpp_sde" and "noise_sampler" not in kw:
        rows = iter(torch.randn(2 * N, *x.shape, device=x.device))
        kw["noise_sampler"] = lambda s0, s1: next(rows)
    with torch.no_grad():
        if name == "dpm_fast":
            return g.sample_dpm_fast(model, state, x, goal, SMIN, SMAX, NFE, **kw)
        return getattr(g, "sample_" + name)(model, state, x, goal, sig, **kw)


def quantile_bounds(unclipped):
    rows = unclipped.reshape(-1, unclipped.shape[-1]).float().cpu()
    return torch.quantile(rows, 0.3, dim=0), torch.quantile(rows, 0.7, dim=0)


def reference(name, B, extra_args=None, tol=None, **kw):
    """(inputs, lo, hi, host loop result with the bounds) of a kind and batch, computed once: the unclipped host loop gives the
    bounds, the host loop with a ClampOnly scaler the result; the conditions that keep the comparison from being vacuous are
    asserted here, on the host loop alone."""
    key = (name, B, str(extra_args), str(sorted(kw.items())))
    if key not in _REFS:
        model, state, goal, x = inputs(B)
        ea = {} if extra_args is None else dict(extra_args=extra_args)
        free = run(name, model, state, x, goal, sched(), callback=lambda d: None, **ea, **kw)
        lo, hi = quantile_bounds(free)
        scaler = ClampOnly(lo, hi)
        want = run(name, model, state, x, goal, sched(), scaler=scaler, **ea, **kw)
        print(f"{name} B={B}: clip_output changed {scaler.changed}; max |clipped - unclipped| "
              f"{float((want - free).abs().max()):.4f}; max |clipped| {float(want.abs().max()):.4f}")
        if name in NEVER_CLIPS:
            assert scaler.changed == [], f"{name}: the host loop is not expected to read its scaler"
            assert torch.equal(want, free)
        else:
            assert len(scaler.changed) == (N - 1 if name == "dpmpp_sde" else N)
            assert min(scaler.changed) >= 0.10, f"{name}: a clip_output call changed {min(scaler.changed):.3f} of the elements"
            atol, rtol = tol or (ATOL, RTOL)
            gap = float((want - free).abs().max())
            assert gap > 100 * (atol + rtol * float(want.abs().max())), f"{name}: clipped and unclipped differ by {gap:.3e} only"
        _REFS[key] = (model, state, goal, x, lo, hi, want)
    return _REFS[key]


def no_forward(mp):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    def boom(*a, **k):
        raise AssertionError("the per-step denoiser ran: the native path was not taken")
    mp.setattr(GCDenoiser, "forward", boom)


# ---- 1, 2: every kind against its host loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_native_call_with_bounds_equals_the_host_loop(name, B, monkeypatch):
    model, state, goal, x, lo, hi, want = reference(name, B)
    no_forward(monkeypatch)
    got = run(name, model, state, x, goal, sched(), scaler=ActionBounds(lo, hi))
    assert_close(got.cpu(), want.cpu(), what=f"{name} B={B}")


@pytest.mark.parametrize("name", ["heun", "dpmpp_2m", "lms"])  # lms: a clipping multistep kind (history push and clamp)
def test_bounds_on_the_split_launches(name, monkeypatch):
    model, state, goal, x, lo, hi, want = reference(name, 80)
    no_forward(monkeypatch)
    got = run(name, model, state, x, goal, sched(), scaler=ActionBounds(lo, hi))
    assert_close(got.cpu(), want.cpu(), what=f"{name} B=80")


# ---- 3: no bounds in effect -> the bits of the call without ------------------------------------------------------------------
def _rows(name, x):
    torch.manual_seed(5)
    n = {"euler_ancestral": N - 1, "dpmpp_sde": 2 * (N - 1), "lms": 0}.get(name, N)
    return torch.randn(n, *x.shape, device=x.device) if n else None


@pytest.mark.parametrize("name", ["euler_ancestral", "heun", "lms", "dpmpp_sde"])
def test_infinite_bounds_and_null_opts_change_no_bit(name):
    model, state, goal, x = inputs(2)
    sig, noise, kw = sched(), _rows(name, x), KINDS[name]
    inf = torch.full((x.shape[-1],), math.inf)
    with torch.no_grad():
        base = raw.run("mdt_sample", model, state, x, goal, sig, kind=name, params=kw, noise=noise)  # the entry without options
        plain = model.sample_native(name, state, x, goal, sig, noise=noise, **kw)
        wide = model.sample_native(name, state, x, goal, sig, noise=noise, bounds=(-inf, inf), **kw)
        null_opts = raw.run("mdt_sample_opt", model, state, x, goal, sig, kind=name, params=kw, noise=noise, opts=None)
    assert torch.equal(plain, base), "sample_native without options is not mdt_sample"
    assert torch.equal(wide, base), "bounds of (-inf, +inf) changed the result"
    assert torch.equal(null_opts, base), "mdt_sample_opt(opts = NULL) is not mdt_sample"


# ---- 4: guidance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["euler", "dpmpp_2s_ancestral"])
def test_guided_call_with_bounds_equals_the_guided_host_loop(name, monkeypatch):
    lam = 3.0
    tol = dict(rtol=1e-3, atol=1e-4 * (abs(lam) + abs(1 - lam)))  # test_gpu_guidance.tol
    model, state, goal, x, lo, hi, want = reference(name, 2, extra_args={"cond_lambda": lam}, tol=(tol["atol"], tol["rtol"]))
    no_forward(monkeypatch)
    got = run(name, model, state, x, goal, sched(), scaler=ActionBounds(lo, hi), extra_args={"cond_lambda": lam})
    assert_close(got.cpu(), want.cpu(), what=f"guided {name}", **tol)


# ---- 5: tree noise ----------------------------------------------------------------------------------------------------------
def test_dpmpp_sde_with_tree_noise_and_bounds(monkeypatch):
    model, state, goal, x = inputs(2)
    sig = sched()
    tree = gs.NativeBrownianTreeNoiseSampler(x, sig[sig > 0].min(), sig.max(), seed=[17, 18])
    model, state, goal, x, lo, hi, want = reference("dpmpp_sde", 2, noise_sampler=tree)
    no_forward(monkeypatch)
    got = run("dpmpp_sde", model, state, x, goal, sig, scaler=ActionBounds(lo, hi), noise_sampler=tree)
    assert_close(got.cpu(), want.cpu(), what="dpmpp_sde, tree noise")


# ---- 6: schedule placement --------------------------------------------------------------------------------------------------
def test_host_and_device_schedule_with_bounds(monkeypatch):
    """Bit-identity between the two is what the existing tests assert for dpm_fast (test_gpu_native_dpm); for the other kinds
    they hold each against the host loop, as here."""
    no_forward(monkeypatch)
    for name in ("heun", "euler_ancestral"):
        model, state, goal, x, lo, hi, want = reference(name, 2)
        for s in (sched(), sched().cuda()):
            got = run(name, model, state, x, goal, s, scaler=ActionBounds(lo, hi))
            assert_close(got.cpu(), want.cpu(), what=f"{name}, sigmas on {s.device}")
    model, state, goal, x, lo, hi, want = reference("dpm_fast", 2)
    b = ActionBounds(lo, hi)
    with torch.no_grad():
        host = model.sample_native("dpm_fast", state, x, goal, [SMAX, SMIN], n_steps=NFE, eta=0., bounds=b)
        dev = model.sample_native("dpm_fast", state, x, goal, torch.tensor([SMAX, SMIN], device="cuda"), n_steps=NFE, eta=0.,
                                  bounds=b)
    assert torch.equal(host, dev)
    assert_close(host.cpu(), want.cpu(), what="dpm_fast")


# ---- 7: graph replay --------------------------------------------------------------------------------------------------------
def test_rollout_sized_calls_with_bounds_replay_a_graph_that_reads_the_current_bounds(monkeypatch):
    model, state, goal, x, lo, hi, want = reference("heun", 1, s_churn=0.)
    no_forward(monkeypatch)
    model.__dict__.pop("_graphed_native", None)
    model.__dict__.pop("_graph_seen", None)
    scaler = ActionBounds(lo, hi)
    outs = [run("heun", model, state, x, goal, sched(), scaler=scaler, s_churn=0.) for _ in range(5)]
    graphs = model.__dict__.get("_graphed_native")
    assert graphs and graphs[-1]._lo is not None, "the third identical call with bounds did not build a graph"
    n_graphs = len(graphs)
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "a replay differs from the eager call"
    assert_close(outs[0].cpu(), want.cpu(), what="heun B=1")
    mid = (lo + hi) / 2
    other = ActionBounds(lo - 0.25, mid)  # agent.scaler = another object
    sixth = run("heun", model, state, x, goal, sched(), scaler=other, s_churn=0.)
    assert len(model.__dict__["_graphed_native"]) == n_graphs, "new bounds must replay the same graph"
    with torch.no_grad():
        fresh = model.sample_native("heun", state, x, goal, sched(), bounds=other, s_churn=0.)
    assert torch.equal(sixth, fresh), "the replay did not read the new bounds"
    assert not torch.equal(sixth, outs[0])
    model.__dict__.pop("_graphed_native", None)
    model.__dict__.pop("_graph_seen", None)


# ---- 8: record --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["heun", "lms"])
def test_record_is_what_a_callback_sees(name):
    model, state, goal, x, lo, hi, _ = reference(name, 2)
    g, sig, kw = gs, sched(), KINDS[name]
    seen = []
    scaler = ClampOnly(lo, hi)
    run(name, model, state, x, goal, sig, scaler=scaler, callback=lambda d: seen.append({k: (v.clone() if torch.is_tensor(v) else v)
                                                                                           for k, v in d.items()}))
    assert len(seen) == N
    torch.manual_seed(11)  # run()'s seed: the rows the host loop drew
    noise = g._randn_rows(x, N) if name == "heun" else None
    with torch.no_grad():
        plain = model.sample_native(name, state, x, goal, sig, noise=noise, bounds=(lo, hi), **kw)
        out, rec = model.sample_native(name, state, x, goal, sig, noise=noise, bounds=ActionBounds(lo, hi), record=True, **kw)
        out_dev, rec_dev = model.sample_native(name, state, x, goal, sig.cuda(), noise=noise, bounds=(lo, hi), record=True, **kw)
    assert torch.equal(out, plain), "record=True changed the actions"
    assert rec["x"].shape == (N,) + tuple(x.shape) and rec["denoised"].shape == (N,) + tuple(x.shape)
    for i, d in enumerate(seen):
        assert_close(rec["x"][i].cpu(), d["x"].cpu(), what=f"{name} x[{i}]")
        assert_close(rec["denoised"][i].cpu(), d["denoised"].cpu(), what=f"{name} denoised[{i}]")
        assert_close(rec["sigma"][i], float(d["sigma"]), rtol=1e-6, atol=0, what=f"{name} sigma[{i}]")
        assert_close(rec["sigma_hat"][i], float(d["sigma_hat"]), rtol=1e-6, atol=0, what=f"{name} sigma_hat[{i}]")
    assert_close(out_dev.cpu(), out.cpu(), what=f"{name}, device schedule")
    assert_close(rec_dev["x"].cpu(), rec["x"].cpu(), what=f"{name} record, device schedule")
    assert_close(rec_dev["denoised"].cpu(), rec["denoised"].cpu(), what=f"{name} record of D, device schedule")
    assert_close(rec_dev["sigma"].cpu(), rec["sigma"], rtol=1e-6, atol=0, what="sigma, device schedule")
    assert_close(rec_dev["sigma_hat"].cpu(), rec["sigma_hat"], rtol=1e-6, atol=0, what="sigma_hat, device schedule")
    got = []
    g.replay_callback(rec, got.append)
    assert len(got) == N and all(set(d) == {"x", "i", "sigma", "sigma_hat", "denoised"} for d in got)
    assert set(got[0]) == set(seen[0]) and [d["i"] for d in got] == list(range(N))
    with pytest.raises(NotImplementedError):
        model.sample_ddim(state, x, goal, sig, record=True)


def test_record_of_dpm_fast_has_one_slot_per_solver_step():
    model, state, goal, x = inputs(2)
    seen = []
    run("dpm_fast", model, state, x, goal, None, callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
    with torch.no_grad():
        out, rec = model.sample_native("dpm_fast", state, x, goal, [SMAX, SMIN], n_steps=NFE, eta=0., record=True)
    assert rec["x"].shape[0] == NFE // 3 + 1 == len(seen) and rec["sigma"].shape == (NFE // 3 + 1,)
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs.cpu(), what=f"dpm_fast x[{i}]")
        assert_close(rec["denoised"][i].cpu(), den.cpu(), what=f"dpm_fast denoised[{i}]")
    with torch.no_grad():  # a device schedule: the rows are placed by the structure alone, sigma is computed with torch
        out_dev, rec_dev = model.sample_native("dpm_fast", state, x, goal, torch.tensor([SMAX, SMIN], device="cuda"),
                                               n_steps=NFE, eta=0., record=True)
    assert torch.equal(out_dev, out) and torch.equal(rec_dev["x"], rec["x"]) and torch.equal(rec_dev["denoised"], rec["denoised"])
    assert_close(rec_dev["sigma"].cpu(), rec["sigma"], rtol=1e-5, atol=0, what="dpm_fast sigma, device schedule")
    assert_close(rec_dev["sigma_hat"].cpu(), rec["sigma_hat"], rtol=1e-5, atol=0, what="dpm_fast sigma_hat, device schedule")


def test_guided_record_holds_the_combined_denoiser():
    lam = 3.0
    tol = dict(rtol=1e-3, atol=1e-4 * (abs(lam) + abs(1 - lam)))  # test_gpu_guidance.tol
    model, state, goal, x, lo, hi, want = reference("euler", 2, extra_args={"cond_lambda": lam}, tol=(tol["atol"], tol["rtol"]))
    seen = []
    run("euler", model, state, x, goal, sched(), scaler=ClampOnly(lo, hi), extra_args={"cond_lambda": lam},
        callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
    torch.manual_seed(11)  # run()'s seed
    noise = gs._randn_rows(x, N)
    with torch.no_grad():
        out, rec = model.sample_native("euler", state, x, goal, sched().cuda(), noise=noise, bounds=(lo, hi), record=True,
                                       cond_lambda=lam, **KINDS["euler"])
    assert_close(out.cpu(), want.cpu(), what="guided euler", **tol)
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs.cpu(), what=f"guided x[{i}]", **tol)
        assert_close(rec["denoised"][i].cpu(), den.cpu(), what=f"guided D_lambda[{i}]", **tol)


# ---- 9: refusals ------------------------------------------------------------------------------------------------------------
def _raw(model, state, x, goal, kind, opts):
    return raw.run("mdt_sample_opt", model, state, x, goal, sched(), kind=kind, opts=opts)


def test_bad_options_are_refused_and_the_handle_keeps_working():
    model, state, goal, x, lo, hi, want = reference("lms", 2)
    lo_d, hi_d = lo.cuda(), hi.cuda()
    size = C.sizeof(_lib.SampleOpts)
    src = _lib.BrownianSource(torch.tensor([3], dtype=torch.int64, device="cuda").data_ptr(), 1, 0, 0.0, 0.0, 1e-6)
    bad = {"opts.lo": _lib.SampleOpts(size, 1.0, lo_d.data_ptr(), None, None, None),
           "opts.hi": _lib.SampleOpts(size, 1.0, None, hi_d.data_ptr(), None, None),
           "opts.size": _lib.SampleOpts(size - 8, 1.0, lo_d.data_ptr(), hi_d.data_ptr(), None, None),
           "opts.tree": _lib.SampleOpts(size, 1.0, None, None, None, C.pointer(src)),
           "opts.cond_lambda": _lib.SampleOpts(size, float("nan"), None, None, None, None)}
    for field, opts in bad.items():
        with pytest.raises(_lib.MDTHipError) as err:
            with torch.no_grad():
                _raw(model, state, x, goal, "lms", opts)
        assert err.value.status == 1 and field in str(err.value), f"{field}: {err.value}"
        with torch.no_grad():
            got = _raw(model, state, x, goal, "lms", _lib.SampleOpts(size, 1.0, lo_d.data_ptr(), hi_d.data_ptr(), None, None))
        assert_close(got.cpu(), want.cpu(), what=f"lms after the refused {field}")


def test_bounds_may_be_a_slice_of_a_larger_tensor():
    """lo and hi need a float's alignment only: here they sit 4 bytes into one statistics tensor."""
    model, state, goal, x, lo, hi, want = reference("lms", 2)
    stats = torch.cat([torch.zeros(1), lo, hi]).cuda()
    A = lo.numel()
    assert (stats.data_ptr() + 4) % 16 != 0
    opts = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0, stats.data_ptr() + 4, stats.data_ptr() + 4 + 4 * A, None, None)
    with torch.no_grad():
        got = _raw(model, state, x, goal, "lms", opts)
    assert_close(got.cpu(), want.cpu(), what="lms, bounds in a slice")


# ---- the shipped schedule, and a pass evaluation on a device schedule -------------------------------------------------------
@pytest.mark.parametrize("name", ["heun", "euler_ancestral"])
def test_bounds_on_the_shipped_schedule(name, monkeypatch):
    """Ten steps down to sigma_min = 0.001, what a rollout runs: the last steps move the state by ~sigma, so their clip_output
    calls change few elements -- the 10 % condition is asserted on the steps where the host loop meets it (the first ones), and
    every call must still change something, so the clamp at small sigma is compared too."""
    g = gs
    model, state, goal, x = inputs(2)
    sig = g.get_sigmas_exponential(10, 0.001, SMAX)
    kw = dict(KINDS[name])
    fn = getattr(g, "sample_" + name)
    with torch.no_grad():
        torch.manual_seed(3)
        free = fn(model, state, x, goal, sig, callback=lambda d: None, **kw)
        lo, hi = quantile_bounds(free)
        scaler = ClampOnly(lo, hi)
        torch.manual_seed(3)
        want = fn(model, state, x, goal, sig, scaler=scaler, **kw)
        print(f"{name}, shipped schedule: clip_output changed {scaler.changed}")
        assert len(scaler.changed) == 10 and min(scaler.changed[:3]) >= 0.10 and min(scaler.changed) > 0
        assert float((want - free).abs().max()) > 100 * (ATOL + RTOL * float(want.abs().max()))
        no_forward(monkeypatch)
        for s in (sig, sig.cuda()):
            torch.manual_seed(3)
            got = fn(model, state, x, goal, s, scaler=ActionBounds(lo, hi), **kw)
            assert_close(got.cpu(), want.cpu(), what=f"{name}, shipped schedule, sigmas on {s.device}")


def test_record_with_pass_evaluations_on_a_device_schedule():
    """A schedule so steep that sigma_down rounds to 0 before the last step: the loop skips the second evaluation there, the
    plan pads it with a pass evaluation, and on a device schedule the record's rows are placed by the structure alone."""
    g = gs
    model, state, goal, x = inputs(2)
    sig = torch.tensor([SMAX, 1e-30, 1e-31, 0.0])
    plan = _lib.sampler_plan("dpm_2_ancestral", sig)
    assert plan.n_evals == 5 and any(plan.e[k].cx[0] == 1.0 and not any(plan.e[k].cx[1:]) for k in range(plan.n_evals)), \
        "no pass evaluation: the case checks nothing"
    lo, hi = torch.full((x.shape[-1],), -0.3), torch.full((x.shape[-1],), 0.4)
    seen = []
    with torch.no_grad():
        want = g.sample_dpm_2_ancestral(model, state, x, goal, sig, scaler=ClampOnly(lo, hi),
                                        callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
        noise = torch.zeros(2, *x.shape, device="cuda")  # the structural row count; the plan reads none of them
        out, rec = model.sample_native("dpm_2_ancestral", state, x, goal, sig.cuda(), noise=noise, bounds=(lo, hi), record=True)
    assert len(seen) == 3 and rec["x"].shape[0] == 3
    assert_close(out.cpu(), want.cpu(), what="pass evaluations, device schedule")
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs.cpu(), what=f"x[{i}]")
        assert_close(rec["denoised"][i].cpu(), den.cpu(), what=f"denoised[{i}]")
