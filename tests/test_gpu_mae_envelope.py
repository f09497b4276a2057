"""The masked generative foresight head across the configurations it accepts (tests/envelope_configs.py MAE_ENVELOPE) on the
GPU: inference and a training step of every case against float64 autograd through the oracle (oracle/mae_oracle.py) at the
gates of tests/test_mae_long.py, the recorded cases against the reference's own results (tests/golden/g15_mae_e_*.npz), which
attention op ran (the table's rule is restated from include/mdt_mae.h), two steps around an optimizer step, two forwards
before one backward, the refusals -- and the ops at the shapes these cases send them."""

import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mae_oracle as O
from tests import envelope_configs as E
from tests.helpers import assert_close, mae_envelope_fixture, mae_inputs, mae_params
from tests.test_mae import check_summaries, summary

pytestmark = pytest.mark.gpu

ACCEPTED = sorted(n for n, c in E.MAE_ENVELOPE.items() if not c["refused"])
REFUSED = sorted(n for n, c in E.MAE_ENVELOPE.items() if c["refused"])


def _ops():
    from mdt_policy_amd.models.img_generation import _hip_ops as ops
    return ops


def _lib():
    from mdt_policy_amd import _lib as L
    return L, L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _head(name, load=True):
    from mdt_policy_amd.models.img_generation.masked_transformer_decoder import MaskedTransformerImgDecoder
    kw = E.MAE_ENVELOPE[name]["kwargs"]
    m = MaskedTransformerImgDecoder(**kw)
    P = None
    if load:
        P = mae_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], kw)
        m.load_state_dict(P, strict=True)
    return kw, P, m.cuda()


def _hd(kw):
    return kw["decoder_embed_dim"] // kw["decoder_n_heads"]


def _oracle_step(P, kw, ctx, img, shuffle):
    """float64 forward, loss and autograd -> (rec, mask, restore, visible, loss, d_ctx, {name: gradient})"""
    torch.set_num_threads(min(16, max(8, torch.get_num_threads())))
    P64 = {k: v.detach().double().requires_grad_(k != "decoder_pe") for k, v in P.items()}
    c64 = ctx.double().requires_grad_()
    r, m, restore, vis = O.forward(P64, kw, c64, img.double(), shuffle)
    loss = O.compute_loss(kw, img.double(), r, m)
    loss.backward()
    return r.detach(), m, restore, vis.detach(), loss.item(), c64.grad, {k: v.grad for k, v in P64.items() if v.requires_grad}


def _check_step(m, what, rec, mask, loss, d_ctx, ref, grads=None):
    """The gates of test_mae_long._run_against_oracle.  A parameter whose exact gradient is zero (patch2embed when no patch is
    visible) gets the 1e-9 the bound leaves: it must be zero."""
    r64, m64, _, _, l64, c64, g64 = ref
    assert np.array_equal(mask.cpu().numpy(), m64.numpy()), what
    assert abs(loss - l64) <= 1e-3 * abs(l64), (what, loss, l64)
    assert_close(rec.detach().cpu(), r64, what=f"{what} reconstructions")
    assert_close(d_ctx.cpu(), c64, rtol=2e-3, atol=2e-3 * float(c64.abs().max()), what=f"{what} d_context")
    n = 0
    for k, p in m.named_parameters():
        if p.requires_grad:
            g = p.grad if grads is None else grads[k]
            assert g is not None, f"{what} {k}: no gradient"
            want = g64[k] if g64[k] is not None else torch.zeros_like(p, dtype=torch.float64, device="cpu")
            assert_close(g.cpu(), want, rtol=2e-3, atol=2e-3 * float(want.abs().max()) + 1e-9, what=f"{what} {k}")
            n += 1
    return n


# ------------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", ACCEPTED)
def test_inference_matches_the_float64_oracle(name):
    c = E.MAE_ENVELOPE[name]
    kw, P, m = _head(name)
    ops = _ops()
    for B in c["batches"]:
        ctx, img, noise = mae_inputs(kw, B, c["ctx"], c["seed"] + 10)
        before = dict(ops.ATTN_LAUNCHES)
        with torch.no_grad():
            rec, mask, restore, vis = m(ctx.cuda(), img.cuda(), noise=noise.cuda())
        torch.cuda.synchronize()
        route = E.mae_route(_hd(kw), c["T"], False)
        ran = {k: ops.ATTN_LAUNCHES[k] - before[k] for k in before}
        assert ran == {"mid": 0, "long": 0, route: kw["decoder_depth"]}, (name, B, ran)
        shuffle = torch.argsort(noise, dim=1)
        with torch.no_grad():
            r64, m64, re64, v64 = O.forward({k: v.double() for k, v in P.items()}, kw, ctx.double(), img.double(), shuffle)
        assert tuple(rec.shape) == (B, 2, (c["T"] - c["ctx"]) // 2, kw["patch_size"] ** 2 * kw["in_channels"])
        assert_close(rec.cpu(), r64, what=f"{name} B={B} reconstructions")
        assert np.array_equal(mask.cpu().numpy(), m64.numpy()) and np.array_equal(restore.cpu().numpy(), re64.numpy()), (name, B)
        assert tuple(vis.shape) == (B, 2 * c["n_keep"], kw["decoder_embed_dim"])
        assert_close(vis.cpu(), v64, what=f"{name} B={B} visible patches")


@pytest.mark.parametrize("name", ACCEPTED)
def test_training_step_matches_float64_autograd_and_runs_the_documented_attention(name):
    c = E.MAE_ENVELOPE[name]
    kw, P, m = _head(name)
    ops = _ops()
    ctx, img, noise = mae_inputs(kw, c["train_b"], c["ctx"], c["seed"])
    x = ctx.cuda().requires_grad_()
    before = dict(ops.ATTN_LAUNCHES)
    rec, mask, restore, _ = m(x, img.cuda(), noise=noise.cuda())
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    loss.backward()
    torch.cuda.synchronize()
    # the routing: the mid op wherever its backward fits (the shipped hd 24 x 102 tokens included), else the long one
    route = E.mae_route(_hd(kw), c["T"], True)
    ran = {k: ops.ATTN_LAUNCHES[k] - before[k] for k in before}
    assert ran == {"mid": 0, "long": 0, route: kw["decoder_depth"]}, (name, ran)
    n = _check_step(m, name, rec, mask, loss.item(), x.grad, _oracle_step(P, kw, ctx, img, torch.argsort(noise, dim=1)))
    assert n == 9 + 12 * kw["decoder_depth"]
    if c["n_keep"] == 0:
        assert not m.patch2embed.proj.weight.grad.any() and not m.patch2embed.proj.bias.grad.any()


def test_the_shipped_shape_keeps_its_route():
    """hd 24 at 102 tokens: the mid op, with and without a gradient; and the nodes of a long-routed training forward carry the
    log-sum-exp the long backward needs."""
    ops = _ops()
    assert ops.attention_route(24, 102, True) == ops.attention_route(24, 102, False) == "mid"
    for hd, T, want in ((24, 102, 2), (48, 97, 3), (64, 81, 3), (48, 96, 2), (64, 80, 2)):
        qkv = torch.randn(1, T, 3 * 2 * hd, device="cuda", requires_grad=True)
        out = ops.HipSelfAttention.apply(qkv, 2, hd ** -0.5)
        assert len(out.grad_fn.saved_tensors) == want, (hd, T)


@pytest.mark.parametrize("name", E.MAE_GOLDEN)
def test_head_matches_the_reference_at_the_recorded_cases(name):
    meta, fx, P, ctx, img, shuffle = mae_envelope_fixture(name)
    kw, _, m = _head(name, load=False)
    m.load_state_dict(P, strict=True)
    x = ctx.cuda().requires_grad_()
    noise = torch.from_numpy(fx["restore"]).float().cuda()   # argsort(noise) == the fixture's shuffle
    rec, mask, restore, vis = m(x, img.cuda(), noise=noise)
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    loss.backward()
    torch.cuda.synchronize()
    assert_close(rec.detach().cpu(), fx["rec"], what="reconstructions vs reference")
    assert np.array_equal(mask.cpu().numpy(), fx["mask"]) and np.array_equal(restore.cpu().numpy(), fx["restore"])
    assert tuple(vis.shape) == tuple(fx["visible"].shape)
    assert_close(vis.detach().cpu(), fx["visible"], what="visible patches vs reference")
    ref_loss = float(fx["loss"].reshape(-1)[0])
    assert abs(loss.item() - ref_loss) <= 1e-3 * abs(ref_loss)
    assert_close(x.grad.cpu(), fx["d_ctx"], rtol=2e-3, atol=2e-3 * float(np.abs(fx["d_ctx"]).max()), what="d_context vs reference")
    check_summaries({k: summary(p.grad) for k, p in m.named_parameters() if p.grad is not None}, meta["grads"], name + " vs reference")
    with torch.no_grad():   # the same values without a graph
        rec2, mask2, _, vis2 = m(ctx.cuda(), img.cuda(), noise=noise)
    assert torch.equal(mask2, mask)
    assert_close(rec2.cpu(), fx["rec"], what="no_grad reconstructions vs reference")


# ------------------------------------------------------------------------------------------------------ twice over
def test_two_steps_around_an_optimizer_step():
    """Forward + backward, FusedAdamW.step(), forward + backward again on the same module at d = 96 (hidden 240): the second
    step must see the updated weights in every packed image.  The update itself against float64 AdamW (every entry within the
    2 lr a noise-level gradient can cost, the clearly non-zero entries in the same direction); the second step against the
    oracle on the weights the module now holds."""
    from mdt_policy_amd.optim import FusedAdamW
    name, lr = "e_ratio_2p5", 1e-2
    c = E.MAE_ENVELOPE[name]
    kw, P, m = _head(name)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=lr, weight_decay=0.05)
    ctx, img, noise = mae_inputs(kw, 3, c["ctx"], 411)
    x = ctx.cuda().requires_grad_()
    rec, mask, restore, _ = m(x, img.cuda(), noise=noise.cuda())
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    loss.backward()
    ref = _oracle_step(P, kw, ctx, img, torch.argsort(noise, dim=1))
    _check_step(m, "step 0", rec, mask, loss.item(), x.grad, ref)
    opt.step()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    P64 = {k: v.double().requires_grad_(k != "decoder_pe") for k, v in P.items()}
    for k, g in ref[6].items():
        P64[k].grad = g
    torch.optim.AdamW([v for v in P64.values() if v.requires_grad], lr=lr, weight_decay=0.05).step()
    moved = 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        d_hip = (p.detach().cpu().double() - P[k].double()).flatten()
        d_ref = (P64[k].detach() - P[k].double()).flatten()
        assert float((d_hip - d_ref).abs().max()) <= 2.2 * lr, k
        g = ref[6][k].flatten().abs()
        sure = g >= 0.02 * g.max()
        if float(g.max()) >= 1e-7 and int(sure.sum()) >= 8:
            assert float(torch.dot(d_hip[sure], d_ref[sure]) / (d_hip[sure].norm() * d_ref[sure].norm())) > 0.99, k
            moved += 1
    assert moved >= 20
    P1 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    ctx, img, noise = mae_inputs(kw, 3, c["ctx"], 421)
    x = ctx.cuda().requires_grad_()
    rec, mask, restore, _ = m(x, img.cuda(), noise=noise.cuda())
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    loss.backward()
    torch.cuda.synchronize()
    ref1 = _oracle_step(P1, kw, ctx, img, torch.argsort(noise, dim=1))
    _check_step(m, "step 1", rec, mask, loss.item(), x.grad, ref1)
    stale = _oracle_step(P, kw, ctx, img, torch.argsort(noise, dim=1))   # the step moved the result by more than the gate
    assert float((stale[0] - ref1[0]).abs().max()) > 10 * (1e-4 + 1e-3 * float(ref1[0].abs().max()))


def test_two_forwards_before_one_backward_keep_the_weight_gradients_on_the_chain():
    """Two grad-enabled forwards of one module, one backward of the summed loss: every parameter has two gradients in that
    backward, so none may go beside (SIDE_LAUNCHES unchanged); the accumulated gradients against the oracle's.  The next
    single step goes beside again."""
    ops = _ops()
    name = "e_c1_p8"
    c = E.MAE_ENVELOPE[name]
    kw, P, m = _head(name)
    ins = [mae_inputs(kw, 2, c["ctx"], s) for s in (431, 441)]
    xs = [i[0].cuda().requires_grad_() for i in ins]
    losses = []
    for x, (ctx, img, noise) in zip(xs, ins):
        rec, mask, restore, _ = m(x, img.cuda(), noise=noise.cuda())
        losses.append(m.compute_loss(img.cuda(), rec, mask, restore))
    side0 = ops.SIDE_LAUNCHES
    (losses[0] + losses[1]).backward()
    torch.cuda.synchronize()
    assert ops.SIDE_LAUNCHES == side0
    refs = [_oracle_step(P, kw, ctx, img, torch.argsort(noise, dim=1)) for ctx, img, noise in ins]
    for k, p in m.named_parameters():
        if p.requires_grad:
            want = refs[0][6][k] + refs[1][6][k]
            assert_close(p.grad.cpu(), want, rtol=2e-3, atol=2e-3 * float(want.abs().max()) + 1e-9, what=k)
    for x, r in zip(xs, refs):
        assert_close(x.grad.cpu(), r[5], rtol=2e-3, atol=2e-3 * float(r[5].abs().max()), what="d_context")
    m.zero_grad(set_to_none=True)
    ctx, img, noise = ins[0]
    rec, mask, restore, _ = m(ctx.cuda(), img.cuda(), noise=noise.cuda())
    m.compute_loss(img.cuda(), rec, mask, restore).backward()
    assert ops.SIDE_LAUNCHES > side0


# ------------------------------------------------------------------------------------------------------ refusals
def _side_launches_of_a_step(m, kw, c, seed, P):
    ops = _ops()
    ctx, img, noise = mae_inputs(kw, 2, c["ctx"], seed)
    x = ctx.cuda().requires_grad_()
    m.zero_grad(set_to_none=True)
    rec, mask, restore, _ = m(x, img.cuda(), noise=noise.cuda())
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    side0 = ops.SIDE_LAUNCHES
    loss.backward()
    torch.cuda.synchronize()
    _check_step(m, "after a refusal", rec, mask, loss.item(), x.grad, _oracle_step(P, kw, ctx, img, torch.argsort(noise, dim=1)))
    return ops.SIDE_LAUNCHES - side0


def test_refusals_name_their_limit_and_leave_the_next_call_intact():
    ops = _ops()
    good = "e_glu256_d128"
    gc = E.MAE_ENVELOPE[good]
    gkw, gP, gm = _head(good)
    clean = _side_launches_of_a_step(gm, gkw, gc, 451, gP)
    assert clean >= 2 + 3 * gkw["decoder_depth"]   # every Linear's weight gradient went beside
    for name in REFUSED:
        c = E.MAE_ENVELOPE[name]
        kw, _, m = _head(name, load=False)
        kind, pattern = c["refused"]
        R = 16 if name == "x_tokens_8196" else kw["resolution"]   # (the token count is the module's: no 512 x 512 images needed)
        with pytest.raises(NotImplementedError if kind == "NotImplementedError" else ValueError, match=pattern) as e:
            m(torch.zeros(1, c["ctx"], kw["context_dim"], device="cuda", requires_grad=True),
              torch.zeros(1, 2, kw["in_channels"], R, R, device="cuda"))
        assert "multiples of 16 and lda" not in str(e.value) and "libmdt_hip status" not in str(e.value), (name, str(e.value))
        assert not ops._USES, name
        del m
    # a forward that raises half-way (images with a channel too few: the host-side shape check of the patch gather raises after
    # the context projection has run and been counted) ...
    with pytest.raises(RuntimeError):
        gm(torch.zeros(2, gc["ctx"], gkw["context_dim"], device="cuda", requires_grad=True),
           torch.zeros(2, 2, gkw["in_channels"] - 1, gkw["resolution"], gkw["resolution"], device="cuda"))
    assert not ops._USES
    # ... and the op's own refusal inside a backward (the mid backward asked for a shape it cannot hold)
    L, lib = _lib()
    q = torch.zeros(1, 97, 3 * 96, device="cuda")
    assert lib.mdt_op_attn_mid_bwd(q.data_ptr(), 288, q.data_ptr(), 96, q.data_ptr(), 96, q.data_ptr(), 288, 1, 2, 48, 97, 1.0, _s()) != 0
    assert _side_launches_of_a_step(gm, gkw, gc, 461, gP) == clean


# ------------------------------------------------------------------------------------------------------ the ops at these shapes
def _attn_ref(qkv, H, hd):
    B, T, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D), s.logsumexp(-1)


def _attn_case(B, H, hd, T):
    D = H * hd
    qkv = torch.from_numpy(synthetic.normal("qkv", (B, T, 3 * D), 471))
    do = torch.from_numpy(synthetic.normal("do", (B, T, D), 472))
    q64 = qkv.double().requires_grad_()
    ref, lse = _attn_ref(q64, H, hd)
    ref.backward(do.double())
    return D, qkv.cuda(), do.cuda(), ref.detach(), lse.detach(), q64.grad


@pytest.mark.parametrize("B,H,hd,T,bwd", [(3, 2, 64, 80, True), (3, 2, 48, 96, True), (2, 3, 64, 128, False), (2, 2, 48, 128, False)])
def test_attention_mid_at_the_last_shapes_its_lds_holds(B, H, hd, T, bwd):
    L, lib = _lib()
    D, qd, dod, ref, _, dref = _attn_case(B, H, hd, T)
    out = torch.full((B, T, D), float("nan"), device="cuda")
    L.check(lib.mdt_op_attn_mid_fwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, B, H, hd, T, hd ** -0.5, _s()))
    assert_close(out.cpu(), ref, what="attention output")
    dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
    st = lib.mdt_op_attn_mid_bwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, dod.data_ptr(), D, dq.data_ptr(), 3 * D, B, H, hd, T,
                                 hd ** -0.5, _s())
    torch.cuda.synchronize()
    assert E.mae_mid_lds_bytes(hd, T, True) <= E.MAE_MID_LDS_BUDGET if bwd else E.mae_mid_lds_bytes(hd, T, True) > E.MAE_MID_LDS_BUDGET
    if bwd:
        assert st == 0
        assert_close(dq.cpu(), dref, rtol=1e-3, atol=1e-4, what="d_qkv")
    else:
        assert st != 0 and torch.isnan(dq).all()


@pytest.mark.parametrize("hd,T", [(64, 81), (48, 97)])
def test_attention_mid_backward_refuses_the_first_shape_past_its_lds_with_nothing_launched(hd, T):
    """The op's contract: non-zero status, d_qkv untouched; the forward of the same shape runs.  Routing around it is the head's
    job (attention_route)."""
    L, lib = _lib()
    B, H = 2, 2
    D, qd, dod, ref, _, _ = _attn_case(B, H, hd, T)
    out = torch.full((B, T, D), float("nan"), device="cuda")
    L.check(lib.mdt_op_attn_mid_fwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, B, H, hd, T, hd ** -0.5, _s()))
    assert_close(out.cpu(), ref, what="attention output")
    dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
    assert lib.mdt_op_attn_mid_bwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, dod.data_ptr(), D, dq.data_ptr(), 3 * D, B, H, hd, T,
                                   hd ** -0.5, _s()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(dq).all()
    assert "LDS" in lib.mdt_last_error().decode()


@pytest.mark.parametrize("hd", [48, 64])
@pytest.mark.parametrize("T", [81, 97, 102])
def test_attention_long_at_the_shapes_the_head_now_sends_it(hd, T):
    L, lib = _lib()
    B, H = 3, 2
    D, qd, dod, ref, ref_lse, dref = _attn_case(B, H, hd, T)
    out = torch.full((B, T, D), float("nan"), device="cuda")
    lse = torch.full((B, H, T), float("nan"), device="cuda")
    L.check(lib.mdt_op_attn_long_fwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), B, H, hd, T, hd ** -0.5, _s()))
    assert_close(out.cpu(), ref, what="attention output")
    assert_close(lse.cpu(), ref_lse, what="log-sum-exp")
    dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
    scratch = torch.empty(lib.mdt_op_attn_long_bwd_scratch(B, H, T), device="cuda")
    L.check(lib.mdt_op_attn_long_bwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), dod.data_ptr(), D, dq.data_ptr(), 3 * D,
                                     B, H, hd, T, hd ** -0.5, scratch.data_ptr(), _s()))
    assert_close(dq.cpu(), dref, rtol=1e-3, atol=1e-4, what="d_qkv")


def _swiglu_mlp(M, K, H, seed=481):
    ops = _ops()
    t = [torch.from_numpy(a).cuda().requires_grad_() for a in (
        synthetic.normal("g_x", (M, K), seed), synthetic.normal("g_w0", (2 * H, K), seed + 1, std=K ** -0.5),
        synthetic.normal("g_b0", (2 * H,), seed + 2, std=0.3), synthetic.normal("g_w1", (K, H), seed + 3, std=H ** -0.5),
        synthetic.normal("g_b1", (K,), seed + 4, std=0.3))]
    wy = torch.from_numpy(synthetic.normal("g_wy", (M, K), seed + 5))
    y = ops.HipSwiGLUMLP.apply(*t, ops.PackedWeights())
    (y * wy.cuda()).sum().backward()
    torch.cuda.synchronize()
    return t, wy, y


@pytest.mark.parametrize("M", [37, 4100])
@pytest.mark.parametrize("K,H", [(512, 512), (400, 208), (512, 1024)])
def test_swiglu_mlp_at_the_k_limit_of_its_epilogues(M, K, H):
    """K = 512: the epilogue GEMMs' limit (one K chunk of 512: mdt_gemm_kchunk splits only above that), dx_act_u at N = 512;
    K = 400: no multiple of 64; 2H = 1024 / 2048 on the <2,4,4,3> tiling, 416 on <2,2,4,3>; against float64
    Linear -> SwishGLU -> Linear."""
    t, wy, y = _swiglu_mlp(M, K, H)
    r = [v.detach().cpu().double().requires_grad_() for v in t]
    p, g = (r[0] @ r[1].T + r[2]).tensor_split(2, dim=-1)
    ref = (p * torch.nn.functional.silu(g)) @ r[3].T + r[4]
    (ref * wy.double()).sum().backward()
    assert_close(y.detach().cpu(), ref.detach(), what="fused SwishGLU MLP output")
    for name, got, want in zip(("dx", "dW0", "db0", "dW1", "db1"), t, r):
        assert_close(got.grad.cpu(), want.grad, rtol=2e-3, atol=2e-3 * float(want.grad.abs().max()), what=name)


def test_swiglu_mlp_refuses_k_528_and_runs_the_next_call():
    from mdt_policy_amd._lib import MDTHipError
    with pytest.raises(MDTHipError):
        _swiglu_mlp(37, 528, 64)
    torch.cuda.synchronize()
    t, wy, y = _swiglu_mlp(37, 512, 64)
    r = [v.detach().cpu().double() for v in t]
    p, g = (r[0] @ r[1].T + r[2]).tensor_split(2, dim=-1)
    assert_close(y.detach().cpu(), (p * torch.nn.functional.silu(g)) @ r[3].T + r[4], what="the call after the refusal")


@pytest.mark.parametrize("C_,R,P,single", [(1, 32, 8, False), (4, 16, 4, False), (3, 64, 32, False), (3, 64, 32, True), (1, 32, 8, True)])
def test_patch_loss_at_other_channel_counts_and_patch_sizes(C_, R, P, single):
    """compute_loss's kernel at channel stride 1 and 4, patches of 4 / 8 / 32 pixels (3072 values per patch), and with a mask
    that holds a single 1; element order (row, column, channel) inside a patch; value and gradient in float64."""
    ops = _ops()
    B, X, g_ = 3, 2, R // P
    n, Ee = g_ * g_, P * P * C_
    rec = torch.from_numpy(synthetic.normal("rec", (B, X, n, Ee), 491))
    imgs = torch.from_numpy(synthetic.normal("imgs", (B, X, C_, R, R), 492))
    mask = torch.from_numpy((synthetic.uniform("mask", (B, n), 493) < 0.6).astype(np.float32))
    if single:
        mask = torch.zeros(B, n)
    mask[1, n - 1] = 1.0
    patches = imgs.double().reshape(B, X, C_, g_, P, g_, P).permute(0, 1, 3, 5, 4, 6, 2).reshape(B, X, n, Ee)
    r64 = rec.double().requires_grad_()
    per_patch = ((r64 - patches) ** 2).mean(-1)
    ref = sum((per_patch[:, x] * mask.double()).sum() / mask.double().sum() for x in range(X)) / X
    ref.backward()
    rd = rec.cuda().requires_grad_()
    loss = ops.HipPatchMSE.apply(rd, imgs.cuda(), mask.cuda(), P)
    loss.backward()
    assert_close(loss.detach().cpu().reshape(()), ref.detach().reshape(()), rtol=1e-5, atol=1e-6, what="loss")
    assert_close(rd.grad.cpu(), r64.grad, rtol=1e-4, atol=1e-8, what="d_rec")
    assert (rd.grad.cpu()[mask[:, None, :, None].expand(B, X, n, Ee) == 0] == 0).all()
