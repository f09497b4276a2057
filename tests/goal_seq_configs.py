"""Model configurations whose goal is a sequence of G = goal_seq_len > 1 tokens, in the style of tests/long_context_configs.py.  The
goal is (B, G, goal_dim); its G embedded rows enter the encoder context: [sigma token] + G goal rows + state tokens + [proprio
token] (goal_conditioned=False: MDT-V keeps the G rows behind the state tokens).  Shared by the GPU tests
(tests/test_gpu_goal_seq*.py), the CPU checks (tests/test_cpu_goal_seq.py, tests/test_goal_seq_golden.py) and the recorder
tests/golden/make_golden_goal_seq.py."""
import functools

from tests import long_context_configs
from tests.envelope_configs import SHIPPED_MDT_CONFIG as _BASE, envelope_of

# name -> (architecture, configs factory, overrides, proprio): the form the golden fixtures' meta records (tests/helpers.py: cfg_of)
GOAL_SPEC = {
    # Te = 5: the first length past the collapsed cross-attention (Te <= 4)
    "g2_shipped": ("mdtv", "mdtv_default", dict(goal_seq_len=2), False),
    # Te = 17: the goal rows cross the 16-row tile
    "g14_tile": ("mdtv", "mdtv_default", dict(goal_seq_len=14), False),
    # Te = 32 + 32 = 64, the top of the rule; the decoder (Ta = 10, top-left causal) sees 10 of the 32 goal rows, the state tokens
    # only through the encoder
    "g32_top": ("mdtv", "mdtv_default", dict(goal_seq_len=32, n_obs_token=32), False),
    # the plain Linear goal embedder, one module for both modalities
    "g4_linear_goal": ("mdtv", "mdtv_default", dict(goal_seq_len=4, use_mlp_goal=False, use_modality_encoder=False), False),
    # goal rows behind the state tokens
    "g3_no_goal_cond": ("mdtv", "mdtv_default", dict(goal_seq_len=3, goal_conditioned=False), False),
    # the sigma token is row 0, the goal rows 1..3; the encoder runs inside the step loop
    "g3_plain": ("mdtv", "mdtv_default", dict(goal_seq_len=3, use_ada_conditioning=False), False),
    # NoiseBlock decoder
    "g2_noise": ("mdtv", "mdtv_default", dict(goal_seq_len=2, use_noise_encoder=True), False),
    # the proprio token behind the goal and state rows
    "g2_proprio": ("mdtv", "mdtv_default", dict(goal_seq_len=2), True),
    # Te = 16, the top of head dim 16
    "g13_hd16": ("mdtv", "mdtv_tiny", dict(goal_seq_len=13, n_obs_token=3), False),
    # MDT: goal token j adds pos_emb[:, j], the two state rows pos_emb[:, G]
    "mdt_g3_pos": ("mdt", "mdt_tiny", dict(goal_seq_len=3, use_abs_pos_emb=True), False),
    "mdt_g3_nopos": ("mdt", "mdt_tiny", dict(goal_seq_len=3, use_abs_pos_emb=False), False),
    # MDT with the sigma token in the context
    "mdt_g5_plain": ("mdt", "mdt_tiny", dict(goal_seq_len=5, use_ada_conditioning=False), False),
}

GOAL_ENVELOPE = envelope_of(GOAL_SPEC)


def goal_rows(name):
    return GOAL_ENVELOPE[name]["cfg"]["goal_seq_len"]


context_len = functools.partial(long_context_configs.context_len, envelope=GOAL_ENVELOPE)   # Te of a case of this table


def goal_row0(name):
    """Context row of goal token 0."""
    e = GOAL_ENVELOPE[name]
    cfg = e["cfg"]
    return int(not cfg["use_ada_conditioning"]) + (0 if cfg["goal_conditioned"] else cfg["n_obs_token"])


GOAL_TE = {"g2_shipped": 5, "g14_tile": 17, "g32_top": 64, "g4_linear_goal": 7, "g3_no_goal_cond": 6, "g3_plain": 7, "g2_noise": 5,
           "g2_proprio": 6, "g13_hd16": 16, "mdt_g3_pos": 5, "mdt_g3_nopos": 5, "mdt_g5_plain": 8}

# recorded from the reference by tests/golden/make_golden_goal_seq.py at B = 2 (tests/golden/g23_goalseq_<name>.npz).
# mdt_g3_pos cannot be recorded: the reference's MDTTransformer.apply_position_embeddings also adds pos_emb[:, 1:] (goal_seq_len +
# action_seq_len - 1 rows) to the action_seq_len action rows, a sum it never uses and that raises for every goal_seq_len > 1
# (mdt_transformer.py:322).  Its goal and state lines (:320-321) are what the oracle and the library compute; the MDT recording is
# mdt_g3_nopos, and mdt_g3_pos is held to the float64 oracle alone.
GOAL_GOLDEN = ["g2_shipped", "g14_tile", "g3_no_goal_cond", "g3_plain", "mdt_g3_nopos"]
GOAL_UNRECORDABLE = ["mdt_g3_pos"]
GOAL_GOLDEN_B = 2

# mdt_config fields mdt_create refuses -> (status, what the message names); 1 = MDT_ERR_INVALID_ARG, 2 = MDT_ERR_UNSUPPORTED
GOAL_REFUSED_AT_CREATE = [
    (dict(_BASE, goal_seq_len=0), 1, [b"goal_seq_len 0", b">= 1"]),
    # g13_hd16 with G = 14: 17 tokens at head dim 16
    (dict(_BASE, embed_dim=128, obs_dim=128, goal_seq_len=14), 2, [b"context length 17 tokens at head dim 16", b"14 goal", b"head dim 16 takes 1..16"]),
    # g32_top with G = 33: 65 tokens
    (dict(_BASE, goal_seq_len=33, n_obs_token=32), 2, [b"context length 65 tokens", b"33 goal + 32 state", b"<= 64"]),
]
