"""The masked generative foresight head above 128 decoder tokens: the flash-style self-attention (mdt_op_attn_long_fwd / _bwd,
include/mdt_mae.h) against float64 PyTorch attention, its determinism and its refusals, and the head end to end at
resolutions / patch sizes whose token count the mid-length attention cannot hold, against float64 autograd through the
oracle (oracle/mae_oracle.py)."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mae_oracle as O
from tests.helpers import assert_close


def _lib():
    from mdt_policy_amd import _lib as L
    return L, L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ref(qkv, H, hd, scale):
    """float64 attention (output, per-row log-sum-exp (B, H, T)) with autograd on qkv"""
    B, T, D3 = qkv.shape
    D = D3 // 3
    q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
    s = q @ k.transpose(-1, -2) * scale
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D), s.logsumexp(-1)


def _long(L, lib, qkv, ld, out, ldo, B, H, hd, T, scale):
    lse = torch.full((B, H, T), float("nan"), device="cuda")
    L.check(lib.mdt_op_attn_long_fwd(qkv.data_ptr(), ld, out.data_ptr(), ldo, lse.data_ptr(), B, H, hd, T, scale, _s()))
    return lse


def _long_bwd(L, lib, qkv, ld, out, ldo, lse, do, ldd, dq, ldg, B, H, hd, T, scale):
    scratch = torch.empty(lib.mdt_op_attn_long_bwd_scratch(B, H, T), device="cuda")
    L.check(lib.mdt_op_attn_long_bwd(qkv.data_ptr(), ld, out.data_ptr(), ldo, lse.data_ptr(), do.data_ptr(), ldd, dq.data_ptr(), ldg,
                                     B, H, hd, T, scale, scratch.data_ptr(), _s()))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,hd,T", [(3, 8, 24, 132), (2, 8, 24, 396), (1, 4, 32, 1572), (1, 2, 64, 4096), (2, 3, 16, 129),
                                      (2, 2, 48, 257), (2, 2, 24, 1), (4, 8, 24, 102), (1, 2, 64, 200), (2, 2, 16, 64)])
def test_attention_long_forward_and_backward(B, H, hd, T):
    L, lib = _lib()
    D = H * hd
    scale = hd ** -0.5
    qkv = torch.from_numpy(synthetic.normal("qkv", (B, T, 3 * D), 261))
    do = torch.from_numpy(synthetic.normal("do", (B, T, D), 262))
    q64 = qkv.double().requires_grad_()
    ref, ref_lse = _ref(q64, H, hd, scale)
    ref.backward(do.double())
    qd, dod = qkv.cuda(), do.cuda()
    out = torch.full((B, T, D), float("nan"), device="cuda")
    lse = _long(L, lib, qd, 3 * D, out, D, B, H, hd, T, scale)
    assert_close(out.cpu(), ref.detach(), what="attention output")
    assert_close(lse.cpu(), ref_lse.detach(), what="log-sum-exp")
    dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
    _long_bwd(L, lib, qd, 3 * D, out, D, lse, dod, D, dq, 3 * D, B, H, hd, T, scale)
    assert_close(dq.cpu(), q64.grad, rtol=1e-3, atol=1e-4, what="d_qkv")
    if T <= 128:   # where both ops run, they agree
        mid = torch.full((B, T, D), float("nan"), device="cuda")
        L.check(lib.mdt_op_attn_mid_fwd(qd.data_ptr(), 3 * D, mid.data_ptr(), D, B, H, hd, T, scale, _s()))
        assert_close(out.cpu(), mid.cpu().double(), what="long vs mid forward")


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,hd,T", [(64, 8, 24, 396), (16, 6, 32, 200)])
def test_attention_long_strided_views(B, H, hd, T):
    """qkv, out, d_out and d_qkv as row views of wider buffers (the model passes the qkv projection's output, and a caller may
    write into a wider buffer): the same bits as the packed layout, the extra columns untouched."""
    L, lib = _lib()
    D = H * hd
    scale = hd ** -0.5
    g = torch.Generator(device="cuda").manual_seed(4321 + B)
    qkv = torch.randn(B, T, 3 * D, device="cuda", generator=g) * 1.5
    do = torch.randn(B, T, D, device="cuda", generator=g)
    out = torch.empty(B, T, D, device="cuda")
    lse = _long(L, lib, qkv, 3 * D, out, D, B, H, hd, T, scale)
    ref, _ = _ref(qkv.double(), H, hd, scale)
    assert_close(out.cpu(), ref.cpu(), what="attention output")
    dq = torch.empty(B, T, 3 * D, device="cuda")
    _long_bwd(L, lib, qkv, 3 * D, out, D, lse, do, D, dq, 3 * D, B, H, hd, T, scale)
    wide_in = torch.randn(B, T, 3 * D + 8, device="cuda", generator=g)
    wide_in[..., :3 * D] = qkv
    wide_out = torch.full((B, T, D + 4), float("nan"), device="cuda")
    lse2 = _long(L, lib, wide_in, 3 * D + 8, wide_out, D + 4, B, H, hd, T, scale)
    assert torch.equal(wide_out[..., :D], out) and torch.equal(lse2, lse)
    assert torch.isnan(wide_out[..., D:]).all()
    wide_do = torch.randn(B, T, D + 12, device="cuda", generator=g)
    wide_do[..., :D] = do
    wide_dq = torch.full((B, T, 3 * D + 4), float("nan"), device="cuda")
    _long_bwd(L, lib, wide_in, 3 * D + 8, wide_out, D + 4, lse2, wide_do, D + 12, wide_dq, 3 * D + 4, B, H, hd, T, scale)
    assert torch.equal(wide_dq[..., :3 * D], dq)
    assert torch.isnan(wide_dq[..., 3 * D:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,hd,T", [(2, 8, 24, 396), (256, 8, 24, 132)])
def test_attention_long_is_bitwise_reproducible(B, H, hd, T):
    L, lib = _lib()
    D = H * hd
    g = torch.Generator(device="cuda").manual_seed(99 + T)
    qkv = torch.randn(B, T, 3 * D, device="cuda", generator=g)
    do = torch.randn(B, T, D, device="cuda", generator=g)
    runs = []
    for _ in range(2):
        out = torch.empty(B, T, D, device="cuda")
        lse = _long(L, lib, qkv, 3 * D, out, D, B, H, hd, T, hd ** -0.5)
        dq = torch.empty(B, T, 3 * D, device="cuda")
        _long_bwd(L, lib, qkv, 3 * D, out, D, lse, do, D, dq, 3 * D, B, H, hd, T, hd ** -0.5)
        runs.append((out, lse, dq))
    for a, b, what in zip(runs[0], runs[1], ("out", "lse", "d_qkv")):
        assert torch.equal(a, b), what


@pytest.mark.gpu
def test_attention_long_rejects_what_it_cannot_run():
    L, lib = _lib()
    x = torch.zeros(1, 4097, 3 * 48 + 4, device="cuda")
    o = torch.zeros(1, 4097, 52, device="cuda")
    lse = torch.zeros(1, 4, 4097, device="cuda")
    s = _s()
    assert lib.mdt_op_attn_long_fwd(x.data_ptr(), 144, o.data_ptr(), 48, lse.data_ptr(), 1, 4, 12, 200, 1.0, s) != 0   # head dim 12
    assert lib.mdt_op_attn_long_fwd(x.data_ptr(), 144, o.data_ptr(), 48, lse.data_ptr(), 1, 2, 24, 4097, 1.0, s) != 0  # T > 4096
    assert lib.mdt_op_attn_long_fwd(x.data_ptr(), 146, o.data_ptr(), 48, lse.data_ptr(), 1, 2, 24, 200, 1.0, s) != 0   # odd stride
    assert lib.mdt_op_attn_long_fwd(x.data_ptr() + 4, 144, o.data_ptr(), 48, lse.data_ptr(), 1, 2, 24, 200, 1.0, s) != 0  # misaligned
    scratch = torch.zeros(lib.mdt_op_attn_long_bwd_scratch(1, 2, 4097), device="cuda")
    for hd, T, ld in ((12, 200, 144), (24, 4097, 144), (24, 200, 146)):
        assert lib.mdt_op_attn_long_bwd(x.data_ptr(), ld, o.data_ptr(), 48, lse.data_ptr(), o.data_ptr(), 48, x.data_ptr(), 144, 1, 2,
                                        hd, T, 1.0, scratch.data_ptr(), s) != 0
    torch.cuda.synchronize()
    assert not x.any()   # nothing was launched


# ---------------------------------------------------------------------------------------------------------- the head
KW = {"decoder_depth": 6, "decoder_embed_dim": 192, "decoder_n_heads": 8, "context_dim": 384, "mlp_ratio": 4, "in_channels": 3,
      "norm_pixel_loss": True, "num_images": 2, "mask_ratio": 0.75, "symmetric_mask": True, "img_gen_frame_diff": 3}


def _head(resolution, patch_size, **over):
    from mdt_policy_amd.models.img_generation.masked_transformer_decoder import MaskedTransformerImgDecoder
    kw = dict(KW, resolution=resolution, patch_size=patch_size, **over)
    m = MaskedTransformerImgDecoder(**kw)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items() if k != "decoder_pe"]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, 151, "rich").items()}
    P["decoder_pe"] = m.decoder_pe.detach().clone()
    m.load_state_dict(P, strict=True)
    return kw, P, m.cuda()


def _run_against_oracle(resolution, patch_size, B, seed, what, **over):
    kw, P, m = _head(resolution, patch_size, **over)
    n = (resolution // patch_size) ** 2
    ctx = torch.from_numpy(synthetic.normal("ctx", (B, 4, kw["context_dim"]), seed))
    img = torch.from_numpy(synthetic.normal("img", (B, 2, 3, resolution, resolution), seed + 1))
    noise = torch.from_numpy(synthetic.uniform("mask_noise", (B, n) if kw["symmetric_mask"] else (B, 2, n), seed + 2))
    c = ctx.cuda().requires_grad_()
    rec, mask, restore, _ = m(c, img.cuda(), noise=noise.cuda())
    loss = m.compute_loss(img.cuda(), rec, mask, restore)
    loss.backward()
    torch.cuda.synchronize()
    shuffle = torch.argsort(noise, dim=1)
    torch.set_num_threads(min(32, max(8, torch.get_num_threads())))
    P64 = {k: v.double().requires_grad_(k != "decoder_pe") for k, v in P.items()}
    c64 = ctx.double().requires_grad_()
    r64, m64, _, _ = O.forward(P64, kw, c64, img.double(), shuffle)
    l64 = O.compute_loss(kw, img.double(), r64, m64)
    l64.backward()
    assert np.array_equal(mask.cpu().numpy(), m64.numpy()), what
    assert abs(loss.item() - l64.item()) <= 1e-3 * abs(l64.item()), what
    assert_close(rec.detach().cpu(), r64.detach(), what=f"{what} reconstructions")
    assert_close(c.grad.cpu(), c64.grad, rtol=2e-3, atol=2e-3 * float(c64.grad.abs().max()), what=f"{what} d_context")
    for k, p in m.named_parameters():
        if p.requires_grad:
            ref = P64[k].grad
            assert_close(p.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-9, what=f"{what} {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("resolution,patch_size,symmetric", [(128, 16, True), (224, 16, True), (112, 8, True), (128, 16, False)])
def test_hip_head_above_128_tokens_against_float64_autograd(resolution, patch_size, symmetric):
    """132 / 396 / 396 decoder tokens: the head's attention on the long op; forward, loss and every gradient against float64
    autograd through the oracle."""
    _run_against_oracle(resolution, patch_size, 3, 281, f"{resolution}/{patch_size} symmetric={symmetric}", symmetric_mask=symmetric)


@pytest.mark.gpu
def test_hip_head_training_batch_at_224_against_the_oracle_on_gpu_fp64():
    """A training-sized batch at 224 x 224 / 16 (B = 64: 25 344 decoder rows of 396 tokens) against float64 autograd through
    the oracle."""
    _run_against_oracle(224, 16, 64, 291, "B=64 224/16")


@pytest.mark.gpu
def test_hip_head_refuses_more_than_4096_tokens():
    _, _, m = _head(512, 8)   # 4 + 2 x 4096 tokens
    with pytest.raises(NotImplementedError, match="4096"):
        m(torch.zeros(1, 4, 384, device="cuda"), torch.zeros(1, 2, 3, 512, 512, device="cuda"))
