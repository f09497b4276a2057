"""CPU tier of the masked-image head's envelope (tests/envelope_configs.py MAE_ENVELOPE): every accepted case constructs with
the reference's parameter tree and Linears the weight packer takes, the oracle the GPU tier compares against is pinned to the
REFERENCE's own outputs, loss and gradients at the recorded cases (tests/golden/g15_mae_e_*.npz, make_golden.py g15), and the
table is checked against the limits it claims to sit on (include/mdt_mae.h)."""
import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from tests import envelope_configs as E
from tests.helpers import assert_close, mae_envelope_fixture
from tests.test_mae import check_summaries, summary

ACCEPTED = sorted(n for n, c in E.MAE_ENVELOPE.items() if not c["refused"])
REFUSED = sorted(n for n, c in E.MAE_ENVELOPE.items() if c["refused"])


def _head(name):
    from mdt_policy_amd.models.img_generation.masked_transformer_decoder import MaskedTransformerImgDecoder
    return MaskedTransformerImgDecoder(**E.MAE_ENVELOPE[name]["kwargs"])


@pytest.mark.parametrize("name", ACCEPTED)
def test_accepted_case_constructs_with_packable_linears_and_the_oracles_position_table(name):
    c = E.MAE_ENVELOPE[name]
    kw = c["kwargs"]
    m = _head(name)
    assert m._refusal is None, m._refusal
    d, p, Cn = kw["decoder_embed_dim"], kw["patch_size"], kw["in_channels"]
    n = (kw["resolution"] // p) ** 2
    want = {"mask_token": (1, 1, d), "ctx_dec_pe": (1, 2, 1, d), "decoder_pe": (1, n, d), "patch2embed.proj.weight": (d, Cn, p, p),
            "patch2embed.proj.bias": (d,), "encoder2decoder.weight": (d, kw["context_dim"]), "encoder2decoder.bias": (d,),
            "decoder_norm.g": (d,), "decoder_patch_prediction.weight": (p * p * Cn, d), "decoder_patch_prediction.bias": (p * p * Cn,)}
    hidden = int(kw["mlp_ratio"] * d)
    for l in range(kw["decoder_depth"]):
        pre = f"decoder_blocks.{l}."
        want.update({pre + "pre_norm_attn.g": (d,), pre + "attn.qkv.weight": (3 * d, d), pre + "attn.qkv.bias": (3 * d,),
                     pre + "attn.proj.weight": (d, d), pre + "attn.proj.bias": (d,), pre + "layer_scale_attn.gamma": (d,),
                     pre + "pre_norm_mlp.g": (d,), pre + "mlp.0.project.weight": (2 * hidden, d), pre + "mlp.0.project.bias": (2 * hidden,),
                     pre + "mlp.1.weight": (d, hidden), pre + "mlp.1.bias": (d,), pre + "layer_scale_mlp.gamma": (d,)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    np.testing.assert_allclose(m.decoder_pe[0].numpy(), O.position_table(d, kw["resolution"] // p), atol=1e-6)
    assert not m.decoder_pe.requires_grad
    for mod in m.modules():   # the packer's rule (PackedWeights.refresh): both dimensions of every Linear multiples of 16
        if isinstance(mod, (torch.nn.Linear, torch.nn.Conv2d)):
            N, K = mod.weight.reshape(mod.weight.shape[0], -1).shape
            assert N % 16 == 0 and K % 16 == 0, (name, N, K)
    assert int(n * (1 - kw["mask_ratio"])) == c["n_keep"] and c["ctx"] + 2 * n == c["T"] <= E.MAE_LONG_TMAX
    assert m._mask_indices(n, 2, "cpu", ctx_len=2)[3] == c["n_keep"]


@pytest.mark.parametrize("name", REFUSED)
def test_refused_case_still_constructs_and_names_its_limit(name):
    """The constructor takes what the reference's takes (state dicts load); the refusal is the call's.  On the CPU only the
    recorded reason can be checked (the call itself: tests/test_gpu_mae_envelope.py)."""
    import re
    m = _head(name)
    kind, pattern = E.MAE_ENVELOPE[name]["refused"]
    if name in ("x_num_images3", "x_tokens_8196"):   # refused by the call's own checks of the inputs
        assert m._refusal is None
    else:
        assert kind == "NotImplementedError" and re.search(pattern, m._refusal), m._refusal
        assert "multiples of 16 and lda" not in m._refusal


@pytest.mark.parametrize("name", E.MAE_GOLDEN)
def test_oracle_matches_the_reference_at_the_envelope(name):
    """The gates of test_mae.test_oracle_matches_the_reference_forward_loss_and_gradients."""
    meta, fx, P, ctx, img, shuffle = mae_envelope_fixture(name)
    kw = meta["kwargs"]
    assert kw == E.MAE_ENVELOPE[name]["kwargs"] and meta["B"] == E.MAE_GOLDEN_B and meta["Tc"] == E.MAE_ENVELOPE[name]["ctx"]
    np.testing.assert_allclose(P["decoder_pe"].numpy(), fx["decoder_pe"], atol=1e-6)
    P64 = {k: v.double().requires_grad_(k != "decoder_pe") for k, v in P.items()}
    c64 = ctx.double().requires_grad_()
    rec, mask, restore, vis = O.forward(P64, kw, c64, img.double(), shuffle)
    loss = O.compute_loss(kw, img.double(), rec, mask)
    loss.backward()
    assert_close(rec.detach(), fx["rec"], what="reconstructions")
    assert np.array_equal(mask.numpy(), fx["mask"]) and np.array_equal(restore.numpy(), fx["restore"])
    assert_close(vis.detach(), fx["visible"], what="visible patches")
    assert vis.shape[1] == 2 * E.MAE_ENVELOPE[name]["n_keep"]
    assert abs(loss.item() - float(fx["loss"].reshape(-1)[0])) <= 1e-5 * abs(loss.item())
    assert_close(c64.grad, fx["d_ctx"], rtol=2e-3, atol=1e-8, what="d_context")
    check_summaries({k: summary(v.grad) for k, v in P64.items() if v.grad is not None}, meta["grads"], name)
    if E.MAE_ENVELOPE[name]["n_keep"] == 0:   # the reference embeds every patch and gathers none: exactly zero
        assert meta["grads"]["patch2embed.proj.weight"][0] == 0.0 and meta["grads"]["patch2embed.proj.bias"][0] == 0.0


def test_the_table_sits_on_the_documented_mid_attention_limits():
    """include/mdt_mae.h: 160 KiB per workgroup; the backward of hd 64 holds up to 80 tokens, of hd 48 up to 96, the forward
    every head dim up to 128 tokens."""
    bwd = lambda hd, T: E.mae_mid_lds_bytes(hd, T, True) <= E.MAE_MID_LDS_BUDGET
    assert bwd(64, 80) and not bwd(64, 81) and bwd(48, 96) and not bwd(48, 97)
    assert all(E.mae_mid_lds_bytes(hd, 128, False) <= E.MAE_MID_LDS_BUDGET for hd in (16, 24, 32, 48, 64))
    assert all(bwd(hd, 128) for hd in (16, 24, 32))
    hd_T = lambda n: (E.MAE_ENVELOPE[n]["kwargs"]["decoder_embed_dim"] // E.MAE_ENVELOPE[n]["kwargs"]["decoder_n_heads"], E.MAE_ENVELOPE[n]["T"])
    assert [hd_T(n) for n in ("e_hd64_t80", "e_hd64_t81", "e_hd48_t96", "e_hd48_t97", "e_t128", "e_t129")] == \
        [(64, 80), (64, 81), (48, 96), (48, 97), (24, 128), (24, 129)]
    train = {n: E.mae_route(*hd_T(n), True) for n in ACCEPTED}
    assert {n for n, r in train.items() if r == "long"} == {"e_d384_hd48_t102", "e_d512_hd64_t102", "e_hd64_t81", "e_hd48_t97", "e_t129"}
    assert {n for n in ACCEPTED if E.mae_route(*hd_T(n), False) == "long"} == {"e_t129"}
    assert E.mae_route(24, 102, True) == "mid"   # the shipped shape stays where it was


def test_the_routing_function_agrees_with_the_header_rule():
    """_hip_ops.attention_route (what HipSelfAttention asks) against the rule restated from the header, over every head dim and
    token count both ops take."""
    from mdt_policy_amd.models.img_generation import _hip_ops as ops
    for hd in ops.HEAD_DIMS:
        for T in list(range(1, 140)) + [4096]:
            for train in (False, True):
                assert ops.attention_route(hd, T, train) == E.mae_route(hd, T, train), (hd, T, train)
                if T <= 128:
                    assert ops.mid_attention_lds_bytes(hd, T, train) == E.mae_mid_lds_bytes(hd, T, train)
