"""Model configurations at the edges of what mdt_create accepts (embed_dim a multiple of 16 up to 512, head dims 16 / 32 / 48 /
64, action_dim and action_seq_len 1..16, up to 16 context tokens, RoPE from head dim 32, both architectures).  Shared by the
GPU envelope test (tests/test_gpu_config_envelope.py) and the CPU check that mdt_create's validation accepts every one of
them (tests/test_cpu_abi.py)."""
from mdt_policy_amd import configs


def _case(cfg, arch="mdtv", proprio=False):
    return dict(cfg=cfg, arch=arch, proprio=proprio)


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
