"""Model configurations and batches at which one training step reaches the row counts where the training path changes its
kernels (mdt_policy_amd/csrc/mdt_route.h, mdt_route_train.h), in the style of tests/long_chunk_configs.py: 4096 rows (GEMM
geometries 5 and 9), 8192 rows (the tall and weight-stationary bodies, k_gemm_tn's 192-wide tiles, k_gemm_tn_split) and the narrow
weight gradients' 512 row slices at more than four rows each.  Shared by tests/test_gpu_deep_row_training.py and by
tests/test_route_table.py, which ties every batch here to the route it is there for (tests/c_client/route_table.cpp: deep/ lines)."""
from tests.envelope_configs import envelope_of

# name -> (architecture, configs factory, overrides, proprio): the form the golden fixtures' meta records (tests/helpers.py: cfg_of)
DEEP_SPEC = {
    # 64-step chunks of 64-element actions: chunk attention and the wide head in a step that takes the deep-row routes
    "ta64_a64": ("mdtv", "mdtv_default", dict(action_seq_len=64, action_dim=64), False),
    # ... at d = 192: the K = 192 weight-stationary form and the 192-wide k_gemm_tn tiles
    "ta64_a64_d192": ("mdtv", "mdtv_default", dict(action_seq_len=64, action_dim=64, embed_dim=192, obs_dim=192, n_heads=4), False),
    # ... at d = 256 (heads of 32; goal_dim 384: at obs_dim 256 the default 512 = 2 * obs_dim is the goal truncation mdt_create refuses):
    # the width at which a 4096-row step takes GEMM geometry 5 beside geometry 9 (at d = 384 geometry 5 starts above 4096 rows)
    "ta64_a64_d256": ("mdtv", "mdtv_default", dict(action_seq_len=64, action_dim=64, embed_dim=256, obs_dim=256, goal_dim=384), False),
    # a 64-token context: 64 x 64 encoder chunk attention, a decoder cross-attention prefix of 10 keys
    "ctx64": ("mdtv", "mdtv_default", dict(n_obs_token=63), False),
    # the narrow gradients' wide instantiation on slices of 5 and 6 rows
    "a64_rows2600": ("mdtv", "mdtv_default", dict(action_dim=64), False),
    # the MLP head's (A, HP) gradient and the proprioceptive layer's, one column into the second tile
    "a17_mlp_proprio_rows2600": ("mdtv", "mdtv_default", dict(action_dim=17, linear_output=False), True),
    # the other architecture (d 512, six decoder blocks) at 40-step chunks
    "mdt_ta40": ("mdt", "mdt_default", dict(action_seq_len=40), False),
}

DEEP_ENVELOPE = envelope_of(DEEP_SPEC)

# name -> batches of the eval-mode step; rows: what the batch is there for (decoder rows B * action_seq_len unless it says encoder)
DEEP_BATCHES = {
    "ta64_a64": [64, 80, 127, 128],        # 4096, 5120, 8128 and 8192 rows
    "ta64_a64_d192": [128],                # 8192 rows
    "ta64_a64_d256": [64],                 # 4096 rows
    "ctx64": [128],                        # 8192 encoder rows
    "a64_rows2600": [260],                 # 2600 rows
    "a17_mlp_proprio_rows2600": [260],     # 2600 rows
    "mdt_ta40": [205],                     # 8200 rows
}
DEEP_STEPS = [(name, B) for name, batches in DEEP_BATCHES.items() for B in batches]

# the train-mode step and the step with the split forms off
DEEP_DROPOUT = ("ta64_a64_d192", 128)
DEEP_SPLIT_OFF = ("ta64_a64", 128)
# scratch reuse: the capacity batch and a smaller one whose 384 x 384 weight gradients are cut into more slices (42 of 160 rows at
# 6720 rows against 26 of 320 at 8192: tests/test_route_table.py)
DEEP_REUSE = ("ta64_a64", 128, 105)


def rows_of(name, B):
    """(encoder rows, decoder rows) of a step of `name` at batch B."""
    e = DEEP_ENVELOPE[name]
    cfg = e["cfg"]
    te = cfg["goal_seq_len"] + (cfg["n_obs_token"] if e["arch"] == "mdtv" else 2) + (1 if e["proprio"] else 0)
    return B * te, B * cfg["action_seq_len"]
