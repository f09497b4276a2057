"""Model configurations with contexts of 17 .. 64 tokens (mdt_create accepts them at head dims 32 / 48 / 64), in the style of
tests/long_chunk_configs.py.  The context of MDT-V is [sigma token] + goal + n_obs_token state tokens + [proprio token].  Shared by
the GPU tests (tests/test_gpu_long_context.py, tests/test_gpu_long_context_options.py), the CPU check that mdt_create's validation
accepts every one of them (tests/test_cpu_long_context_abi.py) and the recorder tests/golden/make_golden_ctx.py."""
from tests.envelope_configs import SHIPPED_MDT_CONFIG as _BASE, envelope_of

_ROPE_HD64 = dict(embed_dim=256, obs_dim=256, goal_dim=384, n_heads=4)   # goal_dim 384: 512 = 2 * obs_dim is the goal truncation mdt_create refuses

# name -> (architecture, configs factory, overrides, proprio): the form the golden fixtures' meta records (tests/helpers.py: cfg_of)
CTX_SPEC = {
    # goal + 16: one key into a second 16-row tile; the decoder sees Tv = 10 of them
    "ctx17_hd48": ("mdtv", "mdtv_default", dict(n_obs_token=16), False),
    # four full tiles at the shipped width
    "ctx64_hd48": ("mdtv", "mdtv_default", dict(n_obs_token=63), False),
    # odd H; one row short of two tiles
    "ctx31_h3_d144": ("mdtv", "mdtv_default", dict(embed_dim=144, obs_dim=144, n_heads=3, n_obs_token=30), False),
    # rotary positions past 16 and 32 in the encoder
    "ctx33_rope_hd64": ("mdtv", "mdtv_default", dict(_ROPE_HD64, use_rot_embed=True, n_obs_token=32), False),
    # RoPE at the top of the range
    "ctx64_rope_hd32": ("mdtv", "mdtv_default", dict(embed_dim=128, obs_dim=128, n_heads=4, use_rot_embed=True, n_obs_token=63), False),
    # the plain decoder: sigma + goal + 30, the sigma token is key 0 (d 192, head dim 48: the recorded fixture stays small)
    "ctx32_plain": ("mdtv", "mdtv_default", dict(embed_dim=192, obs_dim=192, n_heads=4, use_ada_conditioning=False, n_obs_token=30), False),
    # NoiseBlock decoder
    "ctx24_noise": ("mdtv", "mdtv_default", dict(use_noise_encoder=True, n_obs_token=23), False),
    # Te < Ta: Tv = 40, query rows >= 39 see every key (d 192, head dim 48)
    "ctx40_ta48": ("mdtv", "mdtv_default", dict(embed_dim=192, obs_dim=192, n_heads=4, n_obs_token=39, action_seq_len=48), False),
    # the largest LDS figure of both kernels
    "ctx64_ta64_hd64": ("mdtv", "mdtv_default", dict(_ROPE_HD64, n_obs_token=63, action_seq_len=64), False),
    # goal + two cameras x 16 latents + proprio, the MLP head
    "ctx34_proprio_mlp_head": ("mdtv", "mdtv_default", dict(linear_output=False, n_obs_token=32), True),
    # goal_conditioned=False: the goal token sits behind the 39 state tokens, where no decoder query sees it (d 128, head dim 32)
    "ctx40_no_goal": ("mdtv", "mdtv_default", dict(embed_dim=128, obs_dim=128, n_heads=4, goal_conditioned=False, n_obs_token=39), False),
    # the wide head beside a long context
    "ctx18_a64": ("mdtv", "mdtv_default", dict(action_dim=64, n_obs_token=17), False),
}

CTX_ENVELOPE = envelope_of(CTX_SPEC)


def context_len(name, envelope=CTX_ENVELOPE):
    """Te of a case: [sigma token] + goal_seq_len + state tokens (n_obs_token; MDT: static and gripper) + [proprio] -- every case of
    the tables keeps its goal."""
    e = envelope[name]
    cfg = e["cfg"]
    return int(not cfg["use_ada_conditioning"]) + cfg["goal_seq_len"] + (cfg["n_obs_token"] if e["arch"] == "mdtv" else 2) + int(e["proprio"])


# (Ta, Te, head dim) of every case
CTX_SHAPES = {name: (e["cfg"]["action_seq_len"], context_len(name), e["cfg"]["embed_dim"] // e["cfg"]["n_heads"]) for name, e in CTX_ENVELOPE.items()}

# recorded from the reference by tests/golden/make_golden_ctx.py at B = 2 (tests/golden/g21_ctx_<name>.npz)
CTX_GOLDEN = ["ctx17_hd48", "ctx33_rope_hd64", "ctx32_plain", "ctx40_ta48", "ctx40_no_goal"]
CTX_GOLDEN_B = 2

# mdt_config fields mdt_create refuses -> status (1 = MDT_ERR_INVALID_ARG, 2 = MDT_ERR_UNSUPPORTED)
CTX_REFUSED_AT_CREATE = [
    (dict(_BASE, embed_dim=128, obs_dim=128, n_obs_token=16), 2),                      # head dim 16 keeps 1..16 tokens
    (dict(_BASE, n_obs_token=64), 2),                                                  # goal + 64 = 65 tokens
    (dict(_BASE, embed_dim=128, obs_dim=128, n_obs_token=16, use_rot_embed=1), 1),     # RoPE at head dim 16, as at any length
]


def attn_chunk_lds(hd, Tq, Tv, bwd):
    """The LDS rule of the chunk attention kernels, restated from the text of include/mdt_hip_debug.h (NOT read from the library: a
    boundary the two disagree on is a finding).  Tv: the keys a launch stages -- the visible prefix min(Ta, Te) of the decoder's
    cross-attention, Tk otherwise; T16 = T rounded up to 16."""
    q16, v16 = (Tq + 15) // 16 * 16, (Tv + 15) // 16 * 16
    if bwd:
        return 4 * ((2 * q16 + 2 * v16) * (hd + 4) + 2 * q16 * (v16 + 4))
    return 4 * ((q16 + v16) * (hd + 4) + hd * (v16 + 4))
