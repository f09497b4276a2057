"""Model configurations with action vectors of 17 .. 64 elements (mdt_create accepts 1 .. 64), in the style of
tests/long_chunk_configs.py.  Shared by the GPU tests (tests/test_gpu_wide_actions.py, tests/test_gpu_wide_action_options.py), the
CPU check that mdt_create's validation accepts every one of them (tests/test_cpu_wide_actions_abi.py) and the recorder
tests/golden/make_golden_wide.py."""
from tests.envelope_configs import SHIPPED_MDT_CONFIG as _BASE, envelope_of

# name -> (architecture, configs factory, overrides, proprio): the form the golden fixtures' meta records (tests/helpers.py: cfg_of)
WIDE_SPEC = {
    # one column into the second 16-column tile
    "a17": ("mdtv", "mdtv_default", dict(action_dim=17), False),
    # two full column tiles
    "a32": ("mdtv", "mdtv_default", dict(action_dim=32), False),
    # odd H, narrow D; one column into the third tile
    "a33_h3_d144": ("mdtv", "mdtv_default", dict(embed_dim=144, obs_dim=144, n_heads=3, action_dim=33), False),
    # the top of the range: four full tiles
    "a64": ("mdtv", "mdtv_default", dict(action_dim=64), False),
    # MLP head (the head kernel reads the 112-wide hidden layer without a LayerNorm) and the proprioceptive token
    "a24_mlp_head_proprio": ("mdtv", "mdtv_default", dict(linear_output=False, action_dim=24), True),
    # the other architecture at its shipped width (d 512)
    "mdt_a20_d512": ("mdt", "mdt_default", dict(action_dim=20), False),
    # the plain decoder (sigma token)
    "a48_plain": ("mdtv", "mdtv_default", dict(use_ada_conditioning=False, action_dim=48), False),
    # NoiseBlock decoder
    "a40_noise": ("mdtv", "mdtv_default", dict(use_noise_encoder=True, action_dim=40), False),
    # wide and long together: RoPE, 24-step chunks (goal_dim 384: at obs_dim 256 the default 512 = 2 * obs_dim is the goal
    # truncation mdt_create refuses)
    "a64_ta24_rope_hd64": ("mdtv", "mdtv_default", dict(embed_dim=256, obs_dim=256, goal_dim=384, n_heads=4, use_rot_embed=True,
                                                        action_seq_len=24, action_dim=64), False),
}

WIDE_ENVELOPE = envelope_of(WIDE_SPEC)

# recorded from the reference by tests/golden/make_golden_wide.py at B = 2 (tests/golden/g20_wide_<name>.npz)
WIDE_GOLDEN = ["a17", "a64", "a24_mlp_head_proprio", "mdt_a20_d512", "a48_plain"]
WIDE_GOLDEN_B = 2

# mdt_config fields mdt_create refuses -> status (2 = MDT_ERR_UNSUPPORTED)
WIDE_REFUSED_AT_CREATE = [
    (dict(_BASE, action_dim=65), 2),   # past the top of the range
    (dict(_BASE, action_dim=0), 2),    # below it
]
