"""Pinned actions inside the native samplers on the MI355X (pytest -m gpu): mdt_sample_opts.pin_known / pin_keep, the pinned
action heads and GCDenoiser.sample_ddim / sample_native(pin=) against the package's host loops, which apply the pin in
GCDenoiser.forward (forced with a no-op ``callback``), and those against the float64 oracle loop of tests/test_action_pin.py.

Built like tests/test_gpu_sampler_bounds.py, with its model, inputs and schedule.  Tolerances are the existing ones:
tests/helpers rtol 1e-3 / atol 1e-4, the guided cases test_gpu_guidance.tol, dpm_fast test_gpu_native_dpm._close.  ``known`` is the
unpinned host-loop result of another noise seed, negated (dpm_fast: times 64, see tests/test_action_pin.py); ``keep`` is 1 on
tokens 0..2, 0.5 on token 3 and 0 elsewhere; the conditions that keep the comparisons from being vacuous
(test_action_pin.conditions) are asserted in ``reference``, on the host loop alone."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.utils.action_pin import ActionPin
from tests import raw_sampler as raw
from tests import test_action_pin as cpu
from tests import test_gpu_guidance as guid
from tests.helpers import ATOL, RTOL, assert_close, inputs_of
from tests.test_gpu_native_dpm import _close
from tests.test_gpu_sampler_bounds import KINDS, N, NFE, SMAX, SMIN, ClampOnly, gs, inputs, model_of, no_forward, quantile_bounds, sched

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ddim"] + sorted(KINDS)
LAM = 2.5
_REFS = {}


def noop(d):
    return None


def other_noise(B):
    """x_T of the other noise seed (tests/test_action_pin.oracle_case's)."""
    _, meta = model_of()
    return inputs_of(dict(meta, B=B, input_seed=900 + B))[2].cuda() * SMAX


def close(name, got, want, what, **tol):
    if name == "dpm_fast":
        return _close(got, want, NFE, what)
    assert_close(got.cpu(), want.cpu(), what=what, **tol)


def reference(name, B, extra_args=None, tol=None, **kw):
    """(model, state, goal, x_T, pin, pinned host-loop result, unpinned one) of a kind and batch, computed once; the conditions
    are asserted here, on the host loop alone."""
    key = (name, B, str(extra_args), str(sorted(kw.items())))
    if key not in _REFS:
        model, state, goal, x = inputs(B)
        ea = dict(extra_args or {})
        free = cpu.run(name, model, state, x, goal, callback=noop, extra_args=dict(ea), **kw)
        known = -cpu.KNOWN_SCALE.get(name, 1.0) * cpu.run(name, model, state, other_noise(B), goal, callback=noop,
                                                          extra_args=dict(ea), **kw)
        pin = ActionPin(known, cpu.keep_of(x.shape[1]))
        want = cpu.run(name, model, state, x, goal, callback=noop, extra_args=dict(ea, pin=pin), **kw)
        atol, rtol = tol or (ATOL, RTOL)
        cpu.conditions(f"{name} B={B}", free, want, known, cpu.keep_of(x.shape[1]), x, atol=atol, rtol=rtol)
        _REFS[key] = (model, state, goal, x, pin, want, free)
    return _REFS[key]


def test_the_kinds_are_those_of_the_cpu_tier():
    assert KINDS == cpu.KINDS and (N, SMIN, SMAX, NFE) == (cpu.N, cpu.SMIN, cpu.SMAX, cpu.NFE)


# ---- 1: every kind and DDIM against the host loop ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_native_call_with_a_pin_equals_the_host_loop(name, B, monkeypatch):
    model, state, goal, x, pin, want, _ = reference(name, B)
    no_forward(monkeypatch)
    got = cpu.run(name, model, state, x, goal, extra_args={"pin": pin})
    close(name, got, want, f"{name} B={B}")


# ---- 2: the host loop against the float64 pinned oracle loop -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "euler", "dpmpp_2m"])
def test_host_loop_equals_the_float64_oracle_loop(name):
    """The pin of the oracle loop (its ``known``), no churn: the generator streams of the two devices differ."""
    kw = dict(s_churn=0.) if name == "euler" else {}
    omodel, ostate, ogoal, ox, _ = cpu.oracle_case(2)
    _, known, pin, _ = cpu.oracle_loops(name, 2)
    want = cpu.run(name, omodel, ostate, ox, ogoal, extra_args={"pin": pin}, **kw)
    free = cpu.run(name, omodel, ostate, ox, ogoal, **kw)
    cpu.conditions(name, free, want, known, cpu.keep_of(ox.shape[1]), ox)
    model, state, goal, x = inputs(2)
    assert torch.equal(x.cpu(), ox.float())
    got = cpu.run(name, model, state, x, goal, callback=noop, extra_args={"pin": pin}, **kw)
    assert_close(got.cpu(), want, what=f"{name}: host loop against float64")


# ---- 3: guidance, then the pin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "euler"])
def test_guided_native_call_with_a_pin_equals_the_guided_host_loop(name, monkeypatch):
    tol = guid.tol(LAM)
    model, state, goal, x, pin, want, _ = reference(name, 2, extra_args={"cond_lambda": LAM}, tol=(tol["atol"], tol["rtol"]))
    no_forward(monkeypatch)
    got = cpu.run(name, model, state, x, goal, extra_args={"cond_lambda": LAM, "pin": pin})
    assert_close(got.cpu(), want.cpu(), what=f"guided {name}", **tol)


# ---- 4: tree noise ---------------------------------------------------------------------------------------------------------------
def test_dpmpp_sde_with_tree_noise_and_a_pin(monkeypatch):
    model, state, goal, x = inputs(2)
    sig = sched()
    tree = gs.NativeBrownianTreeNoiseSampler(x, sig[sig > 0].min(), sig.max(), seed=[17, 18])
    model, state, goal, x, pin, want, _ = reference("dpmpp_sde", 2, noise_sampler=tree)
    no_forward(monkeypatch)
    got = cpu.run("dpmpp_sde", model, state, x, goal, extra_args={"pin": pin}, noise_sampler=tree)
    assert_close(got.cpu(), want.cpu(), what="dpmpp_sde, tree noise")


# ---- 5: bounds, pin and record together ------------------------------------------------------------------------------------------
def test_bounds_pin_and_record_together_on_euler():
    model, state, goal, x, pin, pinned, _ = reference("euler", 2)
    lo, hi = quantile_bounds(pinned)
    seen = []
    scaler = ClampOnly(lo, hi)
    want = cpu.run("euler", model, state, x, goal, scaler=scaler, extra_args={"pin": pin},
                   callback=lambda d: seen.append((d["x"].clone(), d["denoised"].clone())))
    assert len(seen) == N and min(scaler.changed) >= 0.10, scaler.changed
    assert float((want - pinned).abs().max()) > 100 * (ATOL + RTOL * float(want.abs().max()))
    torch.manual_seed(11)  # run()'s seed: the rows the host loop drew
    noise = gs._randn_rows(x, N)
    with torch.no_grad():
        out, rec = model.sample_native("euler", state, x, goal, sched(), noise=noise, bounds=(lo, hi), record=True, pin=pin,
                                       **KINDS["euler"])
        plain = model.sample_native("euler", state, x, goal, sched(), noise=noise, bounds=(lo, hi), pin=pin, **KINDS["euler"])
    assert torch.equal(out, plain), "record=True changed the actions"
    assert_close(out.cpu(), want.cpu(), what="euler with bounds and a pin")
    known, keep = pin.on(x.device, x.shape)
    for i, (xs, den) in enumerate(seen):
        assert_close(rec["x"][i].cpu(), xs.cpu(), what=f"x[{i}]")
        assert_close(rec["denoised"][i].cpu(), den.cpu(), what=f"denoised[{i}]")
        assert torch.equal(rec["denoised"][i][keep == 1], known[keep == 1]), "the recorded denoised is not D'"
        assert torch.equal(den[keep == 1], known[keep == 1])


# ---- 6: a device schedule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "heun"])
def test_device_schedule_with_a_pin(name, monkeypatch):
    model, state, goal, x, pin, want, _ = reference(name, 2)
    no_forward(monkeypatch)
    torch.manual_seed(11)
    with torch.no_grad():
        got = getattr(gs, "sample_" + name)(model, state, x, goal, sched().cuda(), extra_args={"pin": pin}, **KINDS.get(name, {}))
    assert_close(got.cpu(), want.cpu(), what=f"{name}, sigmas on the device")


# ---- 7: no pin in effect -> the bits of the call without -------------------------------------------------------------------------
def _raw(model, state, x, goal, family, lead, opts):
    """The ``_opt`` entry of a family with ``opts`` (None: NULL); ``lead``: the plan family's kind and parameters."""
    return raw.run({"ddim_opt": "mdt_sample_ddim_opt", "plan_opt": "mdt_sample_opt"}[family], model, state, x, goal, sched(),
                   opts=opts, **lead)


def _legacy(model, state, x, goal, name):
    """The entry without options (mdt_sample_ddim / mdt_sample): what an ``_opt`` entry without a pin must equal, bit for bit."""
    if name == "ddim":
        return raw.run("mdt_sample_ddim", model, state, x, goal, sched())
    return raw.run("mdt_sample", model, state, x, goal, sched(), **_plan_lead(name))


def _plan_lead(name):
    return dict(kind=name, params=KINDS[name])


@pytest.mark.parametrize("name", ["ddim", "lms", "dpmpp_2m"])
def test_a_zero_keep_and_an_absent_pin_change_no_bit(name):
    model, state, goal, x, pin, _, _ = reference(name, 2)
    zero = ActionPin(pin.known, torch.zeros(x.shape[1]))
    size = C.sizeof(_lib.SampleOpts)
    with torch.no_grad():
        base = _legacy(model, state, x, goal, name)
        if name == "ddim":
            plain = model.sample_ddim(state, x, goal, sched())
            none = model.sample_ddim(state, x, goal, sched(), pin=zero)
            null = _raw(model, state, x, goal, "ddim_opt", {}, None)
            empty = _raw(model, state, x, goal, "ddim_opt", {}, _lib.SampleOpts(size, 1.0, None, None, None, None, None, None))
        else:
            plain = model.sample_native(name, state, x, goal, sched(), **KINDS[name])
            none = model.sample_native(name, state, x, goal, sched(), pin=zero, **KINDS[name])
            null = _raw(model, state, x, goal, "plan_opt", _plan_lead(name), None)
            empty = _raw(model, state, x, goal, "plan_opt", _plan_lead(name), _lib.SampleOpts(size, 1.0, None, None, None, None))
    assert torch.equal(plain, base), "the facade without a pin is not the plain entry"
    assert torch.equal(none, base), "an all-zero keep changed the result"
    assert torch.equal(null, base) and torch.equal(empty, base), "the opts entry without a pin is not the plain call"


# ---- 8: the head's instantiations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [76, 77])
def test_pin_where_the_rows_arrive_as_slabs(B, monkeypatch):
    """B = 77 on the fixture model: the split launches leave the decoder rows as slabs the head sums (XP > 1); 76 beside it.
    The plain, plan, guided and plan-guided head each, on the inputs and under the conditions of ``reference``."""
    tol = guid.tol(LAM)
    for name, ea, t in (("ddim", None, {}), ("dpmpp_2m", None, {}), ("ddim", {"cond_lambda": LAM}, tol),
                        ("dpmpp_2m", {"cond_lambda": LAM}, tol)):
        model, state, goal, x, pin, want, _ = reference(name, B, extra_args=ea, tol=(t["atol"], t["rtol"]) if t else None)
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = cpu.run(name, model, state, x, goal, extra_args=dict(ea or {}, pin=pin))
        assert_close(got.cpu(), want.cpu(), what=f"{name} {ea} B={B}", **t)


def test_pin_with_an_action_dim_above_eight(monkeypatch):
    """An envelope configuration with action_dim = 16: the AMAX = 16 heads, plain, plan, guided and plan-guided.  ``known`` is
    the unpinned host-loop result of another noise seed, negated, and the conditions are asserted on the host loop, as in
    ``reference``."""
    name = "a16_ctx16"
    model, _ = guid.model_of(name)
    B = 3
    state, goal, noise = guid.inputs(name, B, 31)
    state, goal, x = guid.cuda(state), goal.cuda(), noise.cuda() * SMAX
    x_other = guid.inputs(name, B, 32)[2].cuda() * SMAX
    keep = cpu.keep_of(x.shape[1])
    tol = guid.tol(LAM)
    for kind, ea, t in (("ddim", {}, {}), ("heun", {}, {}), ("ddim", {"cond_lambda": LAM}, tol), ("heun", {"cond_lambda": LAM}, tol)):
        free = cpu.run(kind, model, state, x, goal, callback=noop, extra_args=dict(ea))
        known = -cpu.run(kind, model, state, x_other, goal, callback=noop, extra_args=dict(ea))
        pin = ActionPin(known, keep)
        want = cpu.run(kind, model, state, x, goal, callback=noop, extra_args=dict(ea, pin=pin))
        cpu.conditions(f"a16 {kind} {ea}", free, want, known, keep, x, atol=t.get("atol", ATOL), rtol=t.get("rtol", RTOL))
        with monkeypatch.context() as mp:
            no_forward(mp)
            got = cpu.run(kind, model, state, x, goal, extra_args=dict(ea, pin=pin))
        assert_close(got.cpu(), want.cpu(), what=f"a16 {kind} {ea}", **t)


# ---- 9: graph replay -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ddim", "heun"])
def test_rollout_sized_calls_replay_a_graph_that_reads_the_current_pin(name, monkeypatch):
    model, state, goal, x, pin, want, _ = reference(name, 1, **({"s_churn": 0.} if name == "heun" else {}))
    kw = {"s_churn": 0.} if name == "heun" else {}
    cache = "_graphed_samplers" if name == "ddim" else "_graphed_native"
    for k in (cache, "_graph_seen"):
        model.__dict__.pop(k, None)
    no_forward(monkeypatch)
    outs = [cpu.run(name, model, state, x, goal, extra_args={"pin": pin}, **kw) for _ in range(5)]
    graphs = model.__dict__.get(cache)
    assert graphs and graphs[-1]._pin is not None, "the third identical call with a pin did not build a graph"
    n_graphs = len(graphs)
    for o in outs[1:]:
        assert torch.equal(o, outs[0]), "a replay differs from the eager call"
    close(name, outs[0], want, f"{name} B=1")
    keep = torch.zeros(x.shape[1])
    keep[2:6] = torch.tensor([0.25, 1.0, 1.0, 0.5])
    for other in (ActionPin(pin.known * 0.5 + 0.1, keep), ActionPin.overlap(outs[0], executed=4, hard=2, soft=3)):
        replay = cpu.run(name, model, state, x, goal, extra_args={"pin": other}, **kw)
        assert len(model.__dict__[cache]) == n_graphs, "a new pin must replay the same graph"
        with torch.no_grad():
            if name == "ddim":
                fresh = model.sample_ddim(state, x, goal, sched(), pin=other)
            else:
                fresh = model.sample_native(name, state, x, goal, sched(), pin=other, **dict(KINDS[name], **kw))
        assert torch.equal(replay, fresh), "the replay did not read the new pin"
        assert not torch.equal(replay, outs[0])
    for k in (cache, "_graph_seen"):
        model.__dict__.pop(k, None)


# ---- 10: the adaptive solver keeps its host loop ---------------------------------------------------------------------------------
def test_dpm_adaptive_with_a_pin_runs_the_host_loop_and_matches_float64(monkeypatch):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    omodel, ostate, ogoal, ox, _ = cpu.oracle_case(2)
    _, known, pin, _ = cpu.oracle_loops("ddim", 2)
    with torch.no_grad():
        want, winfo = gs.sample_dpm_adaptive(omodel, ostate, ox, ogoal, SMIN, SMAX, extra_args={"pin": pin}, return_info=True)
        free = gs.sample_dpm_adaptive(omodel, ostate, ox, ogoal, SMIN, SMAX)
    assert float((want - free)[:, :cpu.HARD].abs().max()) > 100 * (ATOL + RTOL * float(want.abs().max()))
    model, state, goal, x = inputs(2)
    calls, fwd = [], GCDenoiser.forward
    monkeypatch.setattr(GCDenoiser, "forward", lambda self, *a, **k: calls.append(k.get("pin")) or fwd(self, *a, **k))
    monkeypatch.setattr(GCDenoiser, "sample_dpm_adaptive_native", lambda *a, **k: pytest.fail("the native call takes no pin"))
    with torch.no_grad():
        got, info = gs.sample_dpm_adaptive(model, state, x, goal, SMIN, SMAX, extra_args={"pin": pin}, return_info=True)
    print(f"dpm_adaptive: {info} on the GPU, {winfo} in float64")
    assert calls and calls[0] is pin, "the host loop did not hand the pin to forward"
    assert info == winfo
    assert_close(got.cpu(), want, what="dpm_adaptive with a pin")


# ---- 11: refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_pin_options_are_refused_and_the_handle_keeps_working():
    model, state, goal, x, pin, want, _ = reference("ddim", 2)
    _, _, _, _, pin_l, want_l, _ = reference("lms", 2)
    known, keep = pin.on(x.device, x.shape)
    size = C.sizeof(_lib.SampleOpts)
    rec = torch.empty(N, 2, *x.shape, device="cuda")
    src = _lib.BrownianSource(torch.tensor([3], dtype=torch.int64, device="cuda").data_ptr(), 1, 0, 0.0, 0.0, 1e-6)
    Opts = _lib.SampleOpts
    bad = {"opts.pin_keep": Opts(size, 1.0, None, None, None, None, known.data_ptr(), None),
           "opts.pin_known": Opts(size, 1.0, None, None, None, None, None, keep.data_ptr()),
           "opts.record": Opts(size, 1.0, None, None, rec.data_ptr(), None, known.data_ptr(), keep.data_ptr()),
           "opts.tree": Opts(size, 1.0, None, None, None, C.pointer(src), None, None),
           "opts.size": Opts(size - 8, 1.0, None, None, None, None, known.data_ptr(), keep.data_ptr())}
    good = Opts(size, 1.0, None, None, None, None, known.data_ptr(), keep.data_ptr())
    for field, opts in bad.items():
        for family, lead in (("ddim_opt", {}), ("plan_opt", _plan_lead("lms"))):
            if family == "plan_opt" and field in ("opts.record", "opts.tree"):
                continue  # the plan entry takes a record; its tree refusal is test_gpu_sampler_bounds'
            with pytest.raises(_lib.MDTHipError) as err:
                with torch.no_grad():
                    _raw(model, state, x, goal, family, lead, opts)
            assert err.value.status == 1 and field in str(err.value), f"{family} {field}: {err.value}"
        with torch.no_grad():
            got = _raw(model, state, x, goal, "ddim_opt", {}, good)
        assert_close(got.cpu(), want.cpu(), what=f"ddim after the refused {field}")
    # the struct's size before the pin was appended: accepted, the two fields read as NULL whatever lies behind
    old = Opts(Opts.pin_known.offset, 1.0, None, None, None, None, 0xdead0, 0xbeef0)
    with torch.no_grad():
        assert torch.equal(_raw(model, state, x, goal, "ddim_opt", {}, old), _legacy(model, state, x, goal, "ddim"))
        assert torch.equal(_raw(model, state, x, goal, "plan_opt", _plan_lead("lms"), old), _legacy(model, state, x, goal, "lms"))
        kl, ql = pin_l.on(x.device, x.shape)
        got = _raw(model, state, x, goal, "plan_opt", _plan_lead("lms"), Opts(size, 1.0, None, None, None, None, kl.data_ptr(),
                                                                              ql.data_ptr()))
    assert_close(got.cpu(), want_l.cpu(), what="lms through the raw entry")
    # lo / hi on the DDIM entry are accepted and not read
    lo = torch.zeros(x.shape[-1], device="cuda")
    with torch.no_grad():
        got = _raw(model, state, x, goal, "ddim_opt", {}, Opts(size, 1.0, lo.data_ptr(), lo.data_ptr(), None, None, known.data_ptr(),
                                                                keep.data_ptr()))
    assert_close(got.cpu(), want.cpu(), what="ddim, bounds not read")


def test_a_pin_may_be_a_slice_of_a_larger_tensor():
    """pin_known and pin_keep need a float's alignment only."""
    model, state, goal, x, pin, want, _ = reference("ddim", 2)
    known, keep = pin.on(x.device, x.shape)
    both = torch.cat([torch.zeros(1, device="cuda"), known.reshape(-1), keep.reshape(-1)])
    assert (both.data_ptr() + 4) % 16 != 0
    opts = _lib.SampleOpts(C.sizeof(_lib.SampleOpts), 1.0, None, None, None, None, both.data_ptr() + 4,
                           both.data_ptr() + 4 + 4 * known.numel())
    with torch.no_grad():
        got = _raw(model, state, x, goal, "ddim_opt", {}, opts)
    assert_close(got.cpu(), want.cpu(), what="ddim, pin in a slice")


# ---- 12: a plain C client --------------------------------------------------------------------------------------------------------
def test_plain_c_client_with_a_pin_matches_the_facade(tmp_path):
    exe = tmp_path / "pin_client"
    lib = _lib.library_path()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run([shutil.which("gcc") or "gcc", "-std=c11", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(ROOT, "tests", "c_client", "pin_client.c"), "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(rocm, "include"), "-o", str(exe), lib, "-L", os.path.join(rocm, "lib"), "-lamdhip64",
                    "-lm", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    model, _ = guid.model_of("mdtv_default")
    cfg = model.inner_model._hip_config(0.5)
    B, n_steps = 2, 5
    state, goal, noise = guid.inputs("mdtv_default", B, 27)
    sig = gs.get_sigmas_exponential(n_steps, 0.01, 80.0)
    x_T = noise * 80.0
    prev = guid.inputs("mdtv_default", B, 28)[2]
    pin = ActionPin.overlap(prev, executed=4, hard=2, soft=3)
    known, keep = pin.on("cpu", x_T.shape)
    blob = tmp_path / "blob.bin"
    allf = [n for n, _ in _lib.MDTConfig._fields_]
    names = allf[:allf.index("sigma_data")]
    with open(blob, "wb") as f:
        f.write(struct.pack("<i", len(names)))
        f.write(struct.pack(f"<{len(names)}i", *[getattr(cfg, n) for n in names]))
        f.write(struct.pack("<f", 0.5))
        sd = {"inner_model." + k: v for k, v in model.inner_model.state_dict().items()}
        wanted = list(model.inner_model.hip_engine(0.5).expected)
        f.write(struct.pack("<i", len(wanted)))
        for k in wanted:
            t = sd[k].detach().cpu().float().contiguous().numpy()
            f.write(struct.pack("<i", len(k)) + k.encode() + struct.pack("<q", t.size) + t.tobytes())
        f.write(struct.pack("<ii", B, n_steps) + sig.numpy().astype(np.float32).tobytes())
        f.write(state["state_images"].numpy().tobytes() + goal.numpy().tobytes() + x_T.numpy().tobytes())
        f.write(known.numpy().tobytes() + keep.numpy().tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(blob), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "gfx950" in r.stdout
    got = np.fromfile(out, dtype=np.float32).reshape(tuple(x_T.shape))
    with torch.no_grad():
        want = model.sample_ddim(guid.cuda(state), x_T.cuda(), goal.cuda(), sig, pin=pin).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got[:, :2], known.numpy()[:, :2], rtol=1e-3, atol=1e-4)  # the hard tokens arrive at the old chunk
