"""Model configurations with action chunks of 17 .. 64 steps (mdt_create accepts them at head dims 32 / 48 / 64), in the style of
tests/envelope_configs.py.  Shared by the GPU tests (tests/test_gpu_long_chunks.py), the CPU check that mdt_create's
validation accepts every one of them (tests/test_cpu_long_chunks_abi.py) and the recorder tests/golden/make_golden_long.py."""
from tests.envelope_configs import SHIPPED_MDT_CONFIG as _BASE, envelope_of

# name -> (architecture, configs factory, overrides, proprio): the form the golden fixtures' meta records (tests/helpers.py: cfg_of)
LONG_SPEC = {
    # one row into a second 16-row tile
    "ta17_hd48": ("mdtv", "mdtv_default", dict(action_seq_len=17), False),
    # four full tiles
    "ta64_hd48": ("mdtv", "mdtv_default", dict(action_seq_len=64), False),
    # odd H; one row short of two tiles
    "ta31_h3_d144": ("mdtv", "mdtv_default", dict(embed_dim=144, obs_dim=144, n_heads=3, action_seq_len=31), False),
    # rotary positions past 16 and 32 (goal_dim 384: at obs_dim 256 the default 512 = 2 * obs_dim is the goal truncation mdt_create refuses)
    "ta33_rope_hd64": ("mdtv", "mdtv_default", dict(embed_dim=256, obs_dim=256, goal_dim=384, n_heads=4, use_rot_embed=True, action_seq_len=33),
                       False),
    # RoPE at the top of the range
    "ta64_rope_hd32": ("mdtv", "mdtv_default", dict(embed_dim=128, obs_dim=128, n_heads=4, use_rot_embed=True, action_seq_len=64), False),
    # the plain decoder (sigma token): cross-attention 48 x 5, causal top-left
    "ta48_plain": ("mdtv", "mdtv_default", dict(use_ada_conditioning=False, action_seq_len=48), False),
    # NoiseBlock decoder at a tile-aligned chunk
    "ta32_noise": ("mdtv", "mdtv_default", dict(use_noise_encoder=True, action_seq_len=32), False),
    # the other architecture at its shipped width (d 512, head dim 64)
    "mdt_ta40_hd64": ("mdt", "mdt_default", dict(action_seq_len=40), False),
    # cross-attention 64 x 16 (a 16-token context), the 16-wide action head
    "ta64_ctx16_a16": ("mdtv", "mdtv_default", dict(action_dim=16, n_obs_token=15, action_seq_len=64), False),
    # MLP head and the proprioceptive token
    "ta20_mlp_head_proprio": ("mdtv", "mdtv_default", dict(linear_output=False, action_seq_len=20), True),
}

LONG_ENVELOPE = envelope_of(LONG_SPEC)

# recorded from the reference by tests/golden/make_golden_long.py at B = 2 (tests/golden/g19_long_<name>.npz)
LONG_GOLDEN = ["ta17_hd48", "ta33_rope_hd64", "ta48_plain", "mdt_ta40_hd64"]
LONG_GOLDEN_B = 2

# mdt_config fields mdt_create refuses -> status (1 = MDT_ERR_INVALID_ARG, 2 = MDT_ERR_UNSUPPORTED)
LONG_REFUSED_AT_CREATE = [
    (dict(_BASE, embed_dim=128, obs_dim=128, action_seq_len=17), 2),                      # head dim 16 keeps 1..16
    (dict(_BASE, action_seq_len=65), 2),                                                  # past the top of the range
    (dict(_BASE, embed_dim=128, obs_dim=128, action_seq_len=64, use_rot_embed=1), 1),     # RoPE at head dim 16, as at any length
]
