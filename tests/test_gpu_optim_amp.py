"""FusedAdamW's device-driven step and the multi-tensor norm reduction on the GPU (pytest -m gpu): torch.amp.GradScaler +
clip_grad_norm_ + torch.optim.AdamW as the reference sequence, float64 on the CPU as the judge of both."""
import contextlib
import copy
import math

import pytest
import torch

from mdt_policy_amd import _lib
from tests.helpers import assert_close
from tests.test_gpu_optim import _params
from tests.test_optim_amp import control_block

pytestmark = pytest.mark.gpu


def _unaligned(t):
    """The same values in a contiguous CUDA tensor whose first element is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _base(seed):
    """tests/test_gpu_optim.py::_params (1, 4097 and 9216 x 384 elements among them) plus one tensor that ends up unaligned."""
    g = torch.Generator().manual_seed(seed + 7)
    return _params(seed) + [torch.randn(5001, generator=g)]


def _cuda_params(base):
    ps = [torch.nn.Parameter(t.clone().cuda()) for t in base[:-1]]
    return ps + [torch.nn.Parameter(_unaligned(base[-1]))]


def _groups(ps):
    return [{"params": ps[:4], "weight_decay": 0.05}, {"params": ps[4:], "weight_decay": 0.0, "lr": 3e-4}]


def _sync_debug_supported():
    """Does this build of torch raise on a synchronising call under set_sync_debug_mode("error")?"""
    x = torch.ones((), device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        x.item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


@contextlib.contextmanager
def _no_sync():
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_scaler_step_with_clipping_follows_torchs_own_sequence_within_twice_its_error():
    """8 steps of GradScaler.step(FusedAdamW(max_grad_norm=1)) against unscale_ + clip_grad_norm_ + GradScaler.step(AdamW), one of
    them with an inf gradient (skipped by both, the scale halves) and one with a parameter that has no gradient.  step and the
    scale agree exactly after every step.  The tensors are judged against the same steps in float64 on the CPU: the fused
    path's error may be at most twice the error of torch's fp32 sequence (one extra rounding: g * g_mult against torch's two
    separate multiplications), above the absolute floors of test_fused_adamw_matches_torch_adamw_over_steps_and_groups."""
    from mdt_policy_amd.optim import FusedAdamW
    base = _base(0)
    pa, pb = _cuda_params(base), _cuda_params(base)
    pr = [torch.nn.Parameter(t.clone().double()) for t in base]
    oa = FusedAdamW(_groups(pa), lr=1e-3, betas=(0.9, 0.95), max_grad_norm=1.0)
    ob = torch.optim.AdamW(_groups(pb), lr=1e-3, betas=(0.9, 0.95))
    orf = torch.optim.AdamW(_groups(pr), lr=1e-3, betas=(0.9, 0.95))
    sa = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    sb = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    for s in (sa, sb):
        s.scale(torch.zeros((), device="cuda"))  # creates the scale tensor, as the first scaler.scale(loss) does
    floors = {"param": 2e-7, "exp_avg": 5e-7, "exp_avg_sq": 1e-9}
    worst = {k: [0.0, 0.0] for k in floors}  # [fused, torch] error against float64, for the record
    for step in range(8):
        scale = sb.get_scale()
        assert sa.get_scale() == scale
        grads = [g * scale for g in _base(100 + step)]  # the gradients of a scaled loss
        if step == 3:
            grads[2][5] = float("inf")
        for i, (a, b, r, g) in enumerate(zip(pa, pb, pr, grads)):
            if step == 5 and i == 1:  # keeps its step count; its cohort splits
                a.grad = b.grad = r.grad = None
                continue
            a.grad = _unaligned(g) if i == len(grads) - 1 else g.cuda()
            b.grad = g.cuda().clone()
            r.grad = g.double() / scale
        # float64: what unscale_ + clip_grad_norm_(max_norm=1) + AdamW compute, skipped as a whole on overflow
        live = [r.grad for r in pr if r.grad is not None]
        norm = math.sqrt(sum(float((g * g).sum()) for g in live))
        if math.isfinite(norm):
            coef = min(1.0, 1.0 / (norm + 1e-6))
            for g in live:
                g.mul_(coef)
            orf.step()
        sa.step(oa)
        sa.update()
        sb.unscale_(ob)
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        sb.step(ob)
        sb.update()
        assert sa.get_scale() == sb.get_scale(), step
        if math.isfinite(norm):
            got = float(oa.grad_norm)
            assert abs(got - norm) <= 1e-6 * norm, (step, got, norm)  # the bound of the reduction test
        else:
            assert not math.isfinite(float(oa.grad_norm))
        sta, stb, stf = oa.state_dict()["state"], ob.state_dict()["state"], orf.state_dict()["state"]
        assert set(sta) == set(stb)
        for k in stb:
            assert float(sta[k]["step"]) == float(stb[k]["step"]) == float(stf[k]["step"]), (step, k)
        triples = [("param", a.detach(), b.detach(), r.detach()) for a, b, r in zip(pa, pb, pr)]
        for k in stb:
            for name in ("exp_avg", "exp_avg_sq"):
                triples.append((name, sta[k][name], stb[k][name], stf[k][name]))
        for name, a, b, r in triples:
            err_a = float((a.cpu().double() - r).abs().max())
            err_b = float((b.cpu().double() - r).abs().max())
            worst[name] = [max(worst[name][0], err_a), max(worst[name][1], err_b)]
            assert err_a <= max(2.0 * err_b, floors[name]), (step, name, tuple(a.shape), err_a, err_b)
    print("max error against float64 [fused, torch]:", worst)
    assert sa.get_scale() != 1024.0  # the overflow and the growth interval both moved it
    torch.optim.AdamW(_groups(pb), lr=1e-3, betas=(0.9, 0.95)).load_state_dict(oa.state_dict())  # the state layout is torch's


def _amp_step(opt, ps, grads, found_inf, scale=4.0):
    """One device-path step as GradScaler.step drives it: the two attributes around step()."""
    for p, g in zip(ps, grads):
        p.grad = g.cuda() * scale
    opt.grad_scale = torch.full((), scale, device="cuda")
    opt.found_inf = torch.full((), float(found_inf), device="cuda")
    try:
        opt.step()
    finally:
        del opt.grad_scale, opt.found_inf


def test_a_skipped_step_changes_nothing_and_the_next_one_continues_the_count():
    from mdt_policy_amd.optim import FusedAdamW
    base = _base(3)
    pa, pb = _cuda_params(base), _cuda_params(base)
    oa = FusedAdamW(_groups(pa), lr=1e-2, max_grad_norm=2.0)
    ob = FusedAdamW(_groups(pb), lr=1e-2, max_grad_norm=2.0)
    for step in range(2):
        _amp_step(oa, pa, _base(50 + step), 0)
        _amp_step(ob, pb, _base(50 + step), 0)
    before = [p.detach().clone() for p in pa]
    st = oa.state_dict()["state"]
    mv = {k: (st[k]["exp_avg"].clone(), st[k]["exp_avg_sq"].clone()) for k in st}
    assert all(float(st[k]["step"]) == 2.0 for k in st)
    _amp_step(oa, pa, _base(60), 1)  # overflow: the update kernel leaves, the counter stays
    st = oa.state_dict()["state"]
    for p, b in zip(pa, before):
        assert torch.equal(p.detach(), b)
    for k in st:
        assert torch.equal(st[k]["exp_avg"], mv[k][0]) and torch.equal(st[k]["exp_avg_sq"], mv[k][1])
        assert float(st[k]["step"]) == 2.0
    _amp_step(oa, pa, _base(52), 0)
    _amp_step(ob, pb, _base(52), 0)  # the twin never skipped: its third step is t = 3
    assert all(float(v["step"]) == 3.0 for v in oa.state_dict()["state"].values())
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())


def test_one_device_step_is_the_control_block_applied_to_adamw():
    """The float64 restatement of k_opt_ctl (tests/test_optim_amp.py) and AdamW's formulas on one tensor, two steps."""
    from mdt_policy_amd.optim import FusedAdamW
    g = torch.Generator().manual_seed(21)
    w = torch.randn(6000, generator=g)
    p = torch.nn.Parameter(w.clone().cuda())
    lr, b1, b2, eps, wd, scale, max_norm = 1e-2, 0.9, 0.95, 1e-8, 0.1, 8.0, 3.0
    opt = FusedAdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_grad_norm=max_norm)
    ref, m, v, t = w.double(), torch.zeros(6000, dtype=torch.float64), torch.zeros(6000, dtype=torch.float64), 0.0
    for step in range(2):
        grad = torch.randn(6000, generator=g) * scale
        _amp_step(opt, [p], [grad / scale], 0, scale=scale)
        c = control_block(t, b1, b2, grad_scale=scale, found_inf=0.0, grad_sumsq=float((grad.double() ** 2).sum()), max_norm=max_norm)
        t = c["step"]
        assert c["g_mult"] < 1.0 / scale  # clipped: the norm of 6000 normals is about 77
        assert abs(float(opt.grad_norm) - c["grad_norm"]) <= 1e-6 * c["grad_norm"]
        gd = grad.double() * c["g_mult"]
        ref = ref * (1.0 - lr * wd)
        m = b1 * m + (1.0 - b1) * gd
        v = b2 * v + (1.0 - b2) * gd * gd
        ref = ref - lr / c["bc1"] * (m / (v.sqrt() / c["bc2_sqrt"] + eps))
    assert t == 2.0 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    assert_close(p.detach().cpu(), ref, rtol=2e-6, atol=2e-7, what="parameter")


def test_without_scaler_and_clipping_the_step_is_todays_launch_bit_for_bit():
    from mdt_policy_amd.optim import FusedAdamW
    base = _base(5)
    pa, pb = _cuda_params(base), _cuda_params(base)
    oa = FusedAdamW(pa, lr=2e-3, betas=(0.9, 0.95), weight_decay=0.03)
    lib = _lib.load()
    m = [torch.zeros_like(p) for p in pb]
    v = [torch.zeros_like(p) for p in pb]
    for step in range(1, 4):
        grads = [g.cuda() for g in _base(70 + step)]
        for p, g in zip(pa, grads):
            p.grad = g
        oa.step()
        tab = (_lib.OptTensor * len(pb))()
        for i, p in enumerate(pb):
            tab[i] = _lib.OptTensor(p=p.data_ptr(), g=grads[i].data_ptr(), m=m[i].data_ptr(), v=v[i].data_ptr(), ema=None,
                                    numel=p.numel())
        _lib.check(lib.mdt_op_multi_adamw(tab, len(pb), 2e-3, 0.9, 0.95, 1e-8, 0.03, step,
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert oa.grad_norm is None and not oa._dev  # never left the host-counted path
    for a, b in zip(pa, pb):
        assert torch.equal(a.detach(), b.detach())
    st = oa.state_dict()["state"]
    for k in st:
        assert float(st[k]["step"]) == 3.0
        assert torch.equal(st[k]["exp_avg"], m[k]) and torch.equal(st[k]["exp_avg_sq"], v[k])


def test_a_plain_step_after_device_steps_takes_the_count_back():
    """GradScaler(enabled=False) calls step() without the attributes: the host path resumes at the device's count."""
    from mdt_policy_amd.optim import FusedAdamW
    base = _base(6)
    pa, pb = _cuda_params(base), _cuda_params(base)
    oa, ob = FusedAdamW(pa, lr=1e-3), torch.optim.AdamW(pb, lr=1e-3)
    for step in range(4):
        grads = _base(80 + step)
        for b, g in zip(pb, grads):
            b.grad = g.cuda()
        ob.step()
        if step < 2:
            _amp_step(oa, pa, grads, 0, scale=1.0)
        else:
            for a, g in zip(pa, grads):
                a.grad = g.cuda()
            oa.step()
    assert all(float(s["step"]) == 4.0 for s in oa.state_dict()["state"].values())
    for a, b in zip(pa, pb):
        assert_close(a.detach().cpu(), b.detach().cpu(), rtol=2e-6, atol=2e-7, what="parameter")


def _sumsq(tensors, which, partials="torch"):
    lib = _lib.load()
    tab = (_lib.OptTensor * len(tensors))()
    for i, t in enumerate(tensors):
        tab[i] = _lib.OptTensor(p=t.data_ptr() if which else None, g=None if which else t.data_ptr(), m=None, v=None, ema=None,
                                numel=t.numel())
    out = torch.empty(2, device="cuda")
    need = lib.mdt_op_multi_sumsq_scratch(tab, len(tensors))
    assert need == 2 * sum((t.numel() + 4095) // 4096 for t in tensors)
    scratch = torch.empty(need, device="cuda") if partials == "torch" else None
    _lib.check(lib.mdt_op_multi_sumsq(tab, len(tensors), which, out.data_ptr(), None if scratch is None else scratch.data_ptr(),
                                      need if scratch is not None else 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_multi_sumsq_is_reproducible_accurate_and_counts_non_finite_values(which):
    """Relative error of the norm <= 1e-6, derived: an fp32 tree over the 4096 squares of a chunk carries about
    13 * 2^-24 ~ 8e-7, the tail in double adds nothing, the square root halves it."""
    base = _base(11)
    ts = [t.cuda() for t in base[:-1]] + [_unaligned(base[-1])]
    first = _sumsq(ts, which)
    assert torch.equal(first, _sumsq(ts, which))
    assert torch.equal(first, _sumsq(ts, which, partials="library"))  # the library's own partial buffer: the same bits
    want = float(torch.linalg.vector_norm(torch.cat([t.double().reshape(-1) for t in base])))
    got = math.sqrt(float(first[0]))
    print(f"multi_sumsq which={which}: relative error of the norm {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-6 * want
    assert float(first[1]) == 0.0
    ts[5][4096] = float("inf")       # the scalar tail of the 4097-element tensor
    ts[6][5000, 17] = float("nan")   # a whole chunk of the big one
    ts[4][0] = float("-inf")         # the one-element tensor
    ts[7][5000] = float("nan")       # the unaligned one
    bad = _sumsq(ts, which)
    assert float(bad[1]) == 4.0 and not math.isfinite(float(bad[0]))
    empty = _sumsq([torch.empty(0, device="cuda")], which)
    assert float(empty[0]) == 0.0 and float(empty[1]) == 0.0


def test_scaler_step_on_the_device_path_makes_no_synchronising_torch_call():
    """GradScaler.step(FusedAdamW) under torch's sync debug mode: no .item(), no blocking copy -- in the first step (state and
    device counters are created) and in a later one.  This sees torch's own calls; the library's two entry points are read in
    tests/test_optim_amp.py.  state_dict() may synchronise and is called outside the guarded region."""
    from mdt_policy_amd.optim import FusedAdamW
    if not _sync_debug_supported():
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag .item() on this ROCm build of torch")
    ps = _cuda_params(_base(8))
    opt = FusedAdamW(_groups(ps), lr=1e-3, max_grad_norm=1.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
    scaler.scale(torch.zeros((), device="cuda"))
    for step in range(3):
        for p, g in zip(ps, _base(90 + step)):
            p.grad = g.cuda() * 256.0
        with _no_sync():
            scaler.step(opt)
            scaler.update()
            norm = opt.grad_norm
        assert norm.dim() == 0 and norm.is_cuda
    assert all(float(s["step"]) == 3.0 for s in opt.state_dict()["state"].values())


def _tiny_setup(B=6):
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    cfg = configs.mdtv_tiny()
    torch.manual_seed(0)
    model = GCDenoiser(cfg, 0.5).cuda().eval()
    inp = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, 1).items()}
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, 2).items()}
    return cfg, model, inp, li


def test_six_amp_training_steps_follow_torchs_unscale_clip_adamw_sequence():
    """End to end under autocast + GradScaler: FusedAdamW(max_grad_norm=0.5) against unscale_ + clip_grad_norm_ + AdamW on a deep
    copy, by the criteria of test_five_training_steps_follow_the_oracle_trajectory; then the forward on the stepped
    parameters against the oracle, so the weight cache saw every device-side step."""
    from mdt_policy_amd.optim import FusedAdamW
    from oracle import mdt_oracle as O
    cfg, ma, inp, li = _tiny_setup()
    mb = copy.deepcopy(ma)
    state = {"state_images": inp["state_images"], "modality": "lang"}
    oa = FusedAdamW(ma.parameters(), lr=1e-3, weight_decay=0.05, max_grad_norm=0.5)
    ob = torch.optim.AdamW(mb.parameters(), lr=1e-3, weight_decay=0.05)
    sa, sb = torch.amp.GradScaler("cuda", init_scale=1024.0), torch.amp.GradScaler("cuda", init_scale=1024.0)

    def loss_of(model):
        with torch.autocast("cuda", dtype=torch.float16):
            return model.loss(state, li["actions"], inp["goal"], li["noise_train"], li["sigma"])[0]

    for step in range(6):
        oa.zero_grad(set_to_none=True)
        la = loss_of(ma)
        sa.scale(la).backward()
        sa.step(oa)
        sa.update()
        ob.zero_grad(set_to_none=True)
        lb = loss_of(mb)
        sb.scale(lb).backward()
        sb.unscale_(ob)
        want_norm = float(torch.nn.utils.clip_grad_norm_(mb.parameters(), 0.5))
        sb.step(ob)
        sb.update()
        assert abs(la.item() - lb.item()) <= 2e-3 * abs(lb.item()), f"step {step}: {la.item()} vs {lb.item()}"
        assert abs(float(oa.grad_norm) - want_norm) <= 2e-3 * want_norm, (step, float(oa.grad_norm), want_norm)
        assert sa.get_scale() == sb.get_scale()
    got, want = ma.state_dict(), mb.state_dict()
    moved = 0
    for k, v in want.items():
        if not v.dtype.is_floating_point:
            continue
        d = (got[k].double() - v.double()).abs()
        assert float(d.max()) <= 5.1e-3, k  # 5 steps x lr, as there
        assert float((d > 2e-5 + 2e-3 * v.double().abs()).double().mean()) <= 2e-3, f"{k}: too many elements off"
        moved += 1
    assert moved > 10
    assert all(float(s["step"]) == 6.0 for s in oa.state_dict()["state"].values())
    x = li["actions"] + li["noise_train"] * li["sigma"][:, None, None]
    with torch.no_grad():
        out = ma(state, x, inp["goal"], li["sigma"])
    P = {k: v.detach().cpu() for k, v in ma.state_dict().items()}
    st = {"state_images": inp["state_images"].cpu(), "modality": "lang"}
    ref = O.denoise(P, cfg, st, x.cpu(), inp["goal"].cpu(), li["sigma"].cpu(), 0.5, "mdtv")
    assert_close(out.cpu(), ref, what="forward after six device-driven optimizer steps")


def test_total_norms_equal_the_logging_hooks_loop_without_a_read_back():
    """mdt/models/mdtv_agent.py:201-212 on the MDT-V default denoiser after one backward, to 1e-6 relative."""
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.optim import total_norms
    cfg = configs.mdtv_default()
    torch.manual_seed(0)
    model = GCDenoiser(cfg, 0.5).cuda().eval()
    B = 4
    inp = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, 1).items()}
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, 2).items()}
    state = {"state_images": inp["state_images"], "modality": "lang"}
    model.loss(state, li["actions"], inp["goal"], li["noise_train"], li["sigma"])[0].backward()
    ps = list(model.parameters())
    guard = _no_sync() if _sync_debug_supported() else contextlib.nullcontext()
    with guard:
        gn, pn = total_norms(ps)
    assert gn.dim() == 0 and pn.dim() == 0 and gn.is_cuda and pn.is_cuda
    total_grad_norm = total_param_norm = 0.0
    for p in ps:  # the hook's loop, one read-back per tensor
        if p.grad is not None:
            total_grad_norm += p.grad.norm().item() ** 2
        total_param_norm += p.norm().item() ** 2
    total_grad_norm, total_param_norm = total_grad_norm ** 0.5, total_param_norm ** 0.5
    assert total_grad_norm > 0
    assert abs(gn.item() - total_grad_norm) <= 1e-6 * total_grad_norm, (gn.item(), total_grad_norm)
    assert abs(pn.item() - total_param_norm) <= 1e-6 * total_param_norm, (pn.item(), total_param_norm)
