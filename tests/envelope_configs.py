"""Model configurations at the edges of what mdt_create accepts (embed_dim a multiple of 16 up to 512, head dims 16 / 32 / 48 /
64, action_dim and action_seq_len 1..16, up to 16 context tokens, RoPE from head dim 32, both architectures).  Shared by the
GPU envelope test (tests/test_gpu_config_envelope.py) and the CPU check that mdt_create's validation accepts every one of
them (tests/test_cpu_abi.py).

RESAMPLER_ENVELOPE and MAP_ENVELOPE do the same for the two other handle modules, the Perceiver resampler (mdt_resampler_*)
and the MAP pooling block (mdt_map_pool_*): tests/test_gpu_module_envelope.py runs them, tests/test_cpu_abi.py checks the
constructors' validation, tests/golden/make_golden.py g18 records the reference's results for the cases named in
RESAMPLER_GOLDEN / MAP_GOLDEN.

MAE_ENVELOPE is the same for the masked-image head (MaskedTransformerImgDecoder): tests/test_mae_envelope.py (CPU) and
tests/test_gpu_mae_envelope.py run it, make_golden.py g15 records the reference's results for the cases in MAE_GOLDEN."""
from mdt_policy_amd import configs


def _case(cfg, arch="mdtv", proprio=False):
    return dict(cfg=cfg, arch=arch, proprio=proprio)


def envelope_of(spec):
    """{name: cfg, arch, proprio} of a SPEC table {name: (arch, factory of configs.NAMED, overrides, proprio)}."""
    return {name: _case(configs.NAMED[factory](**ov), arch=arch, proprio=prop) for name, (arch, factory, ov, prop) in spec.items()}


# the shipped MDT-V as mdt_config fields: what the *_REFUSED_AT_CREATE tables of the families vary
SHIPPED_MDT_CONFIG = dict(arch=0, embed_dim=384, n_heads=8, n_enc_layers=1, n_dec_layers=2, action_dim=7, obs_dim=384, goal_dim=512, n_obs_token=3,
                          goal_seq_len=1, action_seq_len=10, use_mlp_goal=1, use_modality_encoder=1, use_abs_pos_emb=1, use_rot_embed=0,
                          use_ada_conditioning=1, use_noise_encoder=0, linear_output=1, bias=0, sigma_data=0.5)


# name -> configuration, architecture, whether the calls carry state["state_obs"] (the proprioceptive token, switched on
# at run time)
ENVELOPE = {
    # k_attn at H * Tq * lanes = 10 * 10 * 3 = 300 > 256; two heads per workgroup of the training attention
    "h10_d480": _case(configs.mdtv_default(embed_dim=480, obs_dim=480, n_heads=10)),
    # RoPE attention at Tq = 16 (8 * 16 * 3 = 384); the training forward runs k_attn (no MFMA form with RoPE)
    "rope_ta16": _case(configs.mdtv_default(use_rot_embed=True, action_seq_len=16)),
    # the plain decoder's explicit cross-attention at Tq = 16
    "plain_ta16": _case(configs.mdtv_default(use_ada_conditioning=False, action_seq_len=16)),
    # head dim 16 x 32 heads (32 * 10 = 320)
    "h32_d512": _case(configs.mdtv_default(embed_dim=512, obs_dim=512, n_heads=32)),
    # odd H; d not a multiple of 128 (no fused MLP launch)
    "h3_d144": _case(configs.mdtv_default(embed_dim=144, obs_dim=144, n_heads=3)),
    # the smallest shapes
    "h1_d64_min": _case(configs.mdtv_default(embed_dim=64, obs_dim=64, n_heads=1, action_dim=1, action_seq_len=1)),
    # the 16-wide action head (A > 8) and a 16-token encoder
    "a16_ctx16": _case(configs.mdtv_default(action_dim=16, n_obs_token=15)),
    # MDT with H = 6 (head dim 64), A > 8, biases
    "mdt_h6_a12": _case(configs.mdt_default(embed_dim=384, n_heads=6, action_dim=12, bias=True), arch="mdt"),
    # the proprioceptive row at the context limit: goal + 14 state tokens + proprio = 16
    "proprio_ctx16": _case(configs.mdtv_default(proprio_dim=16, n_obs_token=14), proprio=True),
}


# ------------------------------------------------------------------------------------------------------------------
# Perceiver resampler and MAP block.  The LDS budgets are restated here from the headers' text (include/mdt_resampler.h,
# include/mdt_map_pool.h), NOT read from the library: a boundary the two disagree on is a finding.
# ------------------------------------------------------------------------------------------------------------------
RESAMPLER_LDS_BUDGET = 160 * 1024
MAP_LDS_BUDGET = 64 * 1024


def resampler_lds_bytes(num_latents, dim_head, keys, train):
    """LDS of one (sample, head) workgroup of the resampler's attention: scaled queries (Q, hd), scores (Q, keys rounded up to
    4), 16 reciprocal sums, (256 / hd) partial P.V sums of (Q, hd) = 256 * Q floats; training keeps dO beside the queries and
    dS beside the scores."""
    kp = (keys + 3) // 4 * 4
    k = 2 if train else 1
    return 4 * (k * num_latents * dim_head + k * num_latents * kp + 16 + 256 * num_latents)


def map_lds_bytes(n_latents, output_dim, n_heads, tokens, train):
    """LDS of one sample's workgroup of the MAP attention (2 * n_heads heads): q (Q, D), k|v (N, 2D), scores (Q, H, N);
    training keeps dO beside q and dS beside the scores."""
    H = 2 * n_heads
    k = 2 if train else 1
    return 4 * (k * n_latents * output_dim + 2 * tokens * output_dim + k * n_latents * H * tokens)


def resampler_mask(kind, B, T):
    """None, or a (B, T) list of 0/1.  "mixed": a pattern that differs per sample and frame, frame 2 masked in EVERY sample
    (its time_pos_emb row gets an exactly zero gradient) and -- from two samples on -- sample 1 with every frame masked."""
    if kind is None:
        return None
    assert kind == "mixed"
    m = [[int((5 * b + 3 * t) % 4 != 0) for t in range(T)] for b in range(B)]
    for b in range(B):
        if T > 2:
            m[b][2] = 0
    if B > 1:
        m[1] = [0] * T
    return m


def _r(dim, dim_head, heads, latents, T, n, batches, train_b, depth=1, ff_mult=1, time_embeds=None, mask=None, infer=True,
       train=True):
    """kwargs of PerceiverResampler; the (T frames, n tokens) to run; inference batches; the batch of the training step;
    infer / train False: that entry point must refuse the shape (LDS budget)."""
    kw = dict(dim=dim, depth=depth, dim_head=dim_head, heads=heads, num_latents=latents, num_time_embeds=time_embeds or T,
              ff_mult=ff_mult)
    return dict(kwargs=kw, T=T, n=n, batches=batches, train_b=train_b, mask=mask, infer=infer, train=train)


_WIDE = dict(dim=512, dim_head=64, heads=2, latents=16, time_embeds=4)  # one model (16 latents x dim_head 64), many key counts

RESAMPLER_ENVELOPE = {
    # the smallest model: 2 keys (one media token + the latent), every loop at its first trip; B = 8200: media GEMM >= 8192 rows
    "r_min_2keys": _r(16, 16, 1, 1, 1, 1, [1, 70, 8200], 3),
    # inner = 48 < dim = 80, K|V product 96 wide, 7 latents, 262 keys (2 mod 4, one full stride + a clamped tail of 6), a frame
    # masked everywhere and a sample masked entirely, more time embeddings than frames; B = 33: 8415 media / 231 latent rows
    "r_inner_lt_dim": _r(80, 16, 3, 7, 5, 51, [1, 4, 33], 4, depth=2, ff_mult=3, time_embeds=6, mask="mixed"),
    # dim 400: LayerNorm prologue at K not a multiple of 64 / 128, k_frame_sums' c < D guard (400 = 6 * 64 + 16); three unmasked
    # frames of five time embeddings
    "r_d400_hd32": _r(400, 32, 5, 4, 3, 37, [1, 5], 3, ff_mult=2, time_embeds=5),
    # dim 208 = 3 * 64 + 16 with 9 latents (three queries per wave and one left over), masked
    "r_d208_hd32": _r(208, 32, 2, 9, 4, 30, [1, 6], 3, ff_mult=3, mask="mixed"),
    # 16 latents x dim_head 64 around the 256-key stride: 255 (3 mod 4, one short stride), 256 (exactly one), 257 (1 mod 4, a
    # second stride of one key), 258 (2 mod 4), 512 (two full strides)
    "r_wide_k255": _r(T=1, n=239, batches=[1, 3], train_b=2, **_WIDE),
    "r_wide_k256": _r(T=2, n=120, batches=[1, 3], train_b=2, **_WIDE),
    "r_wide_k257": _r(T=1, n=241, batches=[1, 3], train_b=2, **_WIDE),
    "r_wide_k258": _r(T=2, n=121, batches=[1, 3], train_b=2, **_WIDE),
    "r_wide_k512": _r(T=4, n=124, batches=[1, 3], train_b=2, **_WIDE),
    # above 64 KiB of LDS in forward (83 KiB) and backward (149 KiB): 16 latents x 1000 keys, 8 heads, two layers, masked
    "r_lds_k1000": _r(512, 64, 8, 16, 3, 328, [1, 3], 2, depth=2, mask="mixed"),
    # the training boundary of (16 latents, dim_head 64): 1084 keys is the last shape the backward's budget holds ...
    "r_wide_k1084_train_edge": _r(T=2, n=534, batches=[1, 2], train_b=2, **_WIDE),
    # ... 1085 keys is refused for training and still runs (and is checked) for inference
    "r_wide_k1085_infer_only": _r(T=1, n=1069, batches=[1, 2], train_b=2, train=False, **_WIDE),
    # the inference boundary: 2236 keys is the last shape the forward's budget holds, 2237 is refused by both entry points
    "r_wide_k2236_infer_edge": _r(T=1, n=2220, batches=[1, 2], train_b=1, train=False, **_WIDE),
    "r_wide_k2237_refused": _r(T=1, n=2221, batches=[1], train_b=1, infer=False, train=False, **_WIDE),
    # the top of the key range: 4096 keys x 3 latents; the forward stays under 64 KiB (52), only the backward (101 KiB) raises
    # the limit; 4093 media tokens: 16 strides, the last clamped
    "r_q3_k4096": _r(128, 64, 2, 3, 1, 4093, [1, 2], 2),
}

# recorded from the reference by make_golden.py g18: name -> batch of the fixture
RESAMPLER_GOLDEN = {"r_min_2keys": 3, "r_inner_lt_dim": 4, "r_d400_hd32": 2, "r_wide_k257": 2, "r_lds_k1000": 2, "r_q3_k4096": 2}


def _m(n_latents, embed_dim, n_heads, output_dim, mlp_ratio, tokens, batches, train_b, infer=True, train=True):
    kw = dict(n_latents=n_latents, embed_dim=embed_dim, n_heads=n_heads, output_dim=output_dim, mlp_ratio=mlp_ratio)
    return dict(kwargs=kw, N=tokens, batches=batches, train_b=train_b, infer=infer, train=train)


MAP_ENVELOPE = {
    # 16 latents x 16 tokens, no squeeze, 2 heads of 24 channels, embed_dim != output_dim, a fractional mlp_ratio that int()
    # truncates (2.34 * 48 = 112.32 -> 112 = 7 * 16); B = 520: 8320 token rows and 8320 latent rows.
    # (The ratio 2.5 gives mlp_hidden = 120, not a multiple of 16: that shape is MAP_REFUSED_AT_CREATE below.)
    "m_q16_e96_d48": _m(16, 96, 1, 48, 2.34, 16, [1, 40, 520], 5),
    # embed_dim 1024 > 512 into 48 channels, ONE token (softmax over a single key), 5 latents, 6 heads of 8
    "m_q5_e1024_n1": _m(5, 1024, 3, 48, 1.0, 1, [1, 50, 330], 6),
    # the smallest block: 16 channels everywhere, 2 latents, 7 tokens
    "m_q2_min": _m(2, 16, 1, 16, 1.0, 7, [1, 33, 1200], 7),
    # 64 heads of 8 channels at the width limit, mlp_hidden = 256 < output_dim, 3 latents x 9 tokens
    "m_q3_e640_h32": _m(3, 640, 32, 512, 0.5, 9, [1, 24, 310], 4),
    # head dim 3 (48 / 16 heads): channel loops that are not a multiple of 4
    "m_hd3": _m(4, 64, 8, 48, 2.0, 5, [1, 30, 400], 5),
    # head dim 1 (16 / 16 heads), 16 tokens
    "m_hd1": _m(3, 32, 8, 16, 3.0, 16, [1, 30, 600], 5),
    # exactly 65536 bytes of LDS for inference (accepted by <=), 98304 for training (refused)
    "m_lds_edge_infer_only": _m(16, 256, 8, 256, 4.0, 16, [1, 20], 2, train=False),
    # 16 latents x 512 channels x 16 tokens: 114688 bytes, refused for inference too
    "m_refused": _m(16, 512, 8, 512, 1.0, 16, [1], 1, infer=False, train=False),
}

MAP_GOLDEN = {"m_q16_e96_d48": 3, "m_q5_e1024_n1": 4, "m_q2_min": 5, "m_q3_e640_h32": 3, "m_hd3": 3, "m_hd1": 3}

# constructor arguments the libraries document as refused (include/mdt_resampler.h, include/mdt_map_pool.h) -> status
# (1 = MDT_ERR_INVALID_ARG, 2 = MDT_ERR_UNSUPPORTED)
_RBASE = dict(dim=64, depth=1, dim_head=16, heads=4, num_latents=2, num_time_embeds=1, ff_mult=4, activation=0)
RESAMPLER_REFUSED_AT_CREATE = [
    (dict(_RBASE, dim=24), 2), (dict(_RBASE, dim=528), 2), (dict(_RBASE, dim_head=48), 2), (dict(_RBASE, num_latents=0), 2),
    (dict(_RBASE, num_latents=17), 2), (dict(_RBASE, activation=1), 2), (dict(_RBASE, ff_mult=0), 1),
]
_MBASE = dict(n_latents=1, embed_dim=128, output_dim=128, n_heads=8, mlp_hidden=512)
MAP_REFUSED_AT_CREATE = [
    (dict(_MBASE, output_dim=528, n_heads=1), 2), (dict(_MBASE, output_dim=48, n_heads=5), 1), (dict(_MBASE, mlp_hidden=120), 2),
    # MAPBlock(16, 96, 1, 48, mlp_ratio=2.5): int(2.5 * 48) = 120
    (dict(n_latents=16, embed_dim=96, output_dim=48, n_heads=1, mlp_hidden=120), 2),
    (dict(_MBASE, n_latents=0), 2), (dict(_MBASE, n_latents=17), 2), (dict(_MBASE, embed_dim=100), 2),
]


# ------------------------------------------------------------------------------------------------------------------
# Masked-image head.  The mid attention's LDS rule is restated here from the text of include/mdt_mae.h, NOT read from the
# library or from the Python routing function: a boundary on which they disagree is a finding.
# ------------------------------------------------------------------------------------------------------------------
MAE_MID_LDS_BUDGET = 160 * 1024
MAE_MID_TMAX, MAE_LONG_TMAX = 128, 4096


def mae_mid_lds_bytes(hd, T, backward):
    """include/mdt_mae.h: T16 = T rounded up to 16; forward (3 T16 (hd + 4) + 64 (T16 + 4) + 16) floats, backward
    (5 T16 (hd + 4) + T16 (T16 + 4) + 144) floats."""
    T16 = -(-T // 16) * 16
    floats = 5 * T16 * (hd + 4) + T16 * (T16 + 4) + 144 if backward else 3 * T16 * (hd + 4) + 64 * (T16 + 4) + 16
    return 4 * floats


def mae_route(hd, T, train):
    """The op the head's attention must run ("mid" / "long") as the header documents it."""
    if T > MAE_MID_TMAX or mae_mid_lds_bytes(hd, T, False) > MAE_MID_LDS_BUDGET:
        return "long"
    return "long" if train and mae_mid_lds_bytes(hd, T, True) > MAE_MID_LDS_BUDGET else "mid"


# the shipped head (conf/model/img_gen/masked_transformer.yaml at gen_img_res 112) and the `tiny` fixture's kwargs
MAE_SHIPPED = dict(resolution=112, patch_size=16, decoder_depth=6, decoder_embed_dim=192, decoder_n_heads=8, context_dim=384,
                   mlp_ratio=4, in_channels=3, norm_pixel_loss=True, num_images=2, mask_ratio=0.75, symmetric_mask=True,
                   img_gen_frame_diff=3)
MAE_TINY = dict(MAE_SHIPPED, resolution=64, decoder_depth=2, decoder_embed_dim=64, decoder_n_heads=4, context_dim=128, mask_ratio=0.5)


def _e(base=MAE_TINY, ctx=4, batches=(1, 3), train_b=2, n_keep=None, T=None, refused=None, seed=301, **over):
    """kwargs of MaskedTransformerImgDecoder; context tokens; inference batches; the batch of the training step; the number of
    visible patches per frame and of decoder tokens the comment claims (checked by the CPU tier); refused: (exception type name,
    pattern its message must match) when the call must raise; seed: of the inputs (weights: 151, "rich")."""
    return dict(kwargs=dict(base, **over), ctx=ctx, batches=list(batches), train_b=train_b, n_keep=n_keep, T=T, refused=refused,
                seed=seed)


def _w(d, heads, **over):
    return dict(decoder_embed_dim=d, decoder_n_heads=heads, context_dim=over.pop("context_dim", 64), decoder_depth=over.pop("decoder_depth", 2), **over)


MAE_ENVELOPE = {
    # every loop at its first trip: d 16, one head of 16, 8/4 (n = 4, E = 16), one channel, one block, hidden 16, one context
    # token; mask 0.5 keeps 2: T = 1 + 2 * 4 = 9
    "e_min": _e(ctx=1, n_keep=2, T=9, resolution=8, patch_size=4, in_channels=1, mlp_ratio=1, mask_ratio=0.5,
                **_w(16, 1, context_dim=16, decoder_depth=1)),
    # the shipped head twice as wide: 8 heads of 48 at 102 tokens -- the mid backward holds hd 48 up to 96 (training: long op)
    "e_d384_hd48_t102": _e(MAE_SHIPPED, n_keep=12, T=102, **_w(384, 8)),
    # 8 heads of 64 at 102 tokens (mid backward up to 80); SwishGLU epilogues at K = 512, the limit of aux_mode (one K chunk:
    # mdt_gemm_kchunk splits only above 512), the backward's dx_act_u at N = 512, row kernels at the D limit (all column groups live)
    "e_d512_hd64_t102": _e(MAE_SHIPPED, n_keep=12, T=102, mlp_ratio=2, **_w(512, 8)),
    # hd 64: 80 tokens is the last shape on the mid backward, 81 the first off it (96/16: n = 36, + 8 / 9 context tokens)
    "e_hd64_t80": _e(ctx=8, n_keep=18, T=80, resolution=96, **_w(128, 2)),
    "e_hd64_t81": _e(ctx=9, n_keep=18, T=81, resolution=96, **_w(128, 2)),
    # hd 48: 96 | 97
    "e_hd48_t96": _e(ctx=24, n_keep=18, T=96, resolution=96, **_w(96, 2)),
    "e_hd48_t97": _e(ctx=25, n_keep=18, T=97, resolution=96, **_w(96, 2)),
    # the hand-over between the two ops inside the head: 128 tokens (mid, 8 tiles) | 129 (long); 112/16 + 30 / 31 context tokens
    "e_t128": _e(ctx=30, n_keep=24, T=128, resolution=112, **_w(96, 4)),
    "e_t129": _e(ctx=31, n_keep=24, T=129, resolution=112, **_w(96, 4)),
    # 32 heads of 16 at d 512 (64/16: T = 36, three tiles); the forward walks hpw heads per workgroup once B * H / hpw reaches
    # 1024 workgroups: B = 3 hpw 1 (96 workgroups), B = 64 hpw 2 (1024), B = 130 hpw 4 (1040)
    "e_h32_d512": _e(batches=(1, 3, 64, 130), n_keep=8, T=36, mlp_ratio=1, **_w(512, 32)),
    # one channel, 32/8 (n = 16, E = 64): channel stride 1 in the patch loss's image index
    "e_c1_p8": _e(n_keep=8, T=36, resolution=32, patch_size=8, in_channels=1, **_w(64, 4)),
    # four channels, 16/4 (n = 16, E = 64), the reference's other masking branch, 2 heads of 24
    "e_c4_p4_asym": _e(n_keep=8, T=36, resolution=16, patch_size=4, in_channels=4, symmetric_mask=False, **_w(48, 2)),
    # 64/32 (n = 4): the patch embedding is a product with K = 3072 (deep-K pipe), the prediction one with N = 3072
    "e_p32": _e(n_keep=2, T=12, resolution=64, patch_size=32, **_w(64, 4)),
    # no blocks: the plain HipRMSNorm branch of forward
    "e_depth0": _e(n_keep=8, T=36, **_w(64, 4, decoder_depth=0)),
    # hidden 240, 2H = 480: SwishGLU forward tiling <2,2,4,3> (N % 32 only), backward <2,2,4,4> (240 % 192 != 0)
    "e_ratio_2p5": _e(n_keep=8, T=36, mlp_ratio=2.5, **_w(96, 4)),
    # 2H = 1024: SwishGLU forward tiling <2,4,4,3> away from K = 192
    "e_glu256_d128": _e(n_keep=8, T=36, mlp_ratio=4, **_w(128, 4)),
    # the constructor's default mask_ratio at the shipped shape: int(49 * (1 - 0.9)) = 4 visible patches
    "e_shipped_mask09": _e(MAE_SHIPPED, n_keep=4, T=102, mask_ratio=0.9),
    # 32/16 (n = 4), mask 0.25: one patch removed per sample, mask.sum() = B
    "e_one_masked": _e(n_keep=3, T=12, resolution=32, mask_ratio=0.25, **_w(64, 4)),
    # 48/16 (n = 9) at the default mask 0.9: int(9 * 0.1) = 0 visible patches -- an empty patch-embedding product, zero
    # gradients for patch2embed (the reference embeds all patches and gathers none)
    "e_keep0": _e(n_keep=0, T=22, resolution=48, mask_ratio=0.9, **_w(64, 4)),
    # the tiny kwargs at B = 240: 240 * 36 = 8640 decoder rows, the >= 8192-row GEMM dispatch at K = 64 / 256 and the
    # bf16-split dW products
    "e_rows8192": _e(batches=(240,), train_b=240, n_keep=8, T=36),
    # ---- refused: a Python exception that names the limit
    "x_d528": _e(refused=("NotImplementedError", "512"), **_w(528, 11)),                       # norms stop at 512
    "x_hd12": _e(refused=("NotImplementedError", "head dim"), **_w(48, 4)),                    # 4 heads of 12
    "x_hidden120": _e(refused=("NotImplementedError", "120"), mlp_ratio=1.5, **_w(80, 5)),     # int(1.5 * 80) = 120
    "x_num_images3": _e(refused=("NotImplementedError", "num_images"), num_images=3),
    "x_tokens_8196": _e(MAE_SHIPPED, refused=("NotImplementedError", "4096"), resolution=512, patch_size=8, decoder_depth=1),
}

# recorded from the reference by make_golden.py g15 at B = 2 (tests/golden/g15_mae_<name>.npz)
MAE_GOLDEN = ["e_min", "e_c1_p8", "e_c4_p4_asym", "e_p32", "e_keep0", "e_one_masked", "e_depth0"]
MAE_GOLDEN_B = 2
