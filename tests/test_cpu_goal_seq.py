"""Goals of several tokens (goal_seq_len > 1) as far as they can be seen without a device: mdt_create's validation accepts every
configuration of tests/goal_seq_configs.py and refuses, with its status and a message that names the rule, goal_seq_len = 0 and the
two lengths just past the context rule; the facade's state_dict is the reference's at the recorded cases; a goal of another length
than the model was built for raises a ValueError that names both numbers; synthetic.sampler_inputs draws (B, goal_seq_len,
goal_dim) and, at goal_seq_len = 1, the values it has always drawn."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs, synthetic
from tests.goal_seq_configs import GOAL_ENVELOPE, GOAL_GOLDEN, GOAL_REFUSED_AT_CREATE, GOAL_TE, goal_rows
from tests.helpers import cfg_of, load_fixture


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(GOAL_ENVELOPE))
def test_create_accepts_every_goal_sequence_configuration(name):
    """Without a GPU every configuration gets as far as hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or
    MDT_ERR_UNSUPPORTED (2)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = GOAL_ENVELOPE[name]
    lib = _lib.load()
    cfg = GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])
    assert cfg.goal_seq_len == goal_rows(name) > 1
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_create_refuses_what_lies_outside_the_rule_and_names_it():
    """goal_seq_len = 0 is an invalid argument; g13_hd16 with one more goal token (17 tokens at head dim 16) and g32_top with one
    more (65 tokens) are unsupported, and the message states the goal's share of the context.  Each refusal comes back before any
    allocation, with or without a GPU."""
    lib = _lib.load()
    for bad, status, words in GOAL_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.MDTConfig(**bad)
        assert lib.mdt_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        msg = lib.mdt_last_error()
        for w in words:
            assert w in msg, (bad, w, msg)
    # one token fewer passes the validation (status 4 without a GPU, 0 with one)
    for bad, _, _ in GOAL_REFUSED_AT_CREATE[1:]:
        h = C.c_void_p()
        cfg = _lib.MDTConfig(**dict(bad, goal_seq_len=bad["goal_seq_len"] - 1))
        st = lib.mdt_create(C.byref(cfg), C.byref(h))
        assert st in (0, 4), (st, lib.mdt_last_error())
        if st == 0:
            lib.mdt_destroy(h)


@pytest.mark.parametrize("name", GOAL_GOLDEN)
def test_facade_state_dict_matches_the_reference(name):
    """Names, shapes and order of the facade's state_dict against the list the reference recorded (pos_emb grows with goal_seq_len)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    meta, fx = load_fixture(f"g23_goalseq_{name}.npz")
    cfg = cfg_of(meta)
    assert cfg == GOAL_ENVELOPE[name]["cfg"] and fx["ctx"].shape[1] == GOAL_TE[name]
    m = GCDenoiser(cfg, sigma_data=0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    pos = dict((k, s) for k, s in meta["state_dict"])["inner_model.pos_emb"]
    assert pos[1] >= cfg["goal_seq_len"] + cfg["action_seq_len"]


@pytest.mark.parametrize("name", ["g2_shipped", "g3_plain", "mdt_g3_pos"])
def test_a_goal_of_the_wrong_length_raises_and_names_both_numbers(name):
    """A handle is built for one layout: G - 1 and G + 1 rows, and a 2-D goal (one row), raise before anything reaches the library
    (the check needs no device).  G rows pass, zeroed as a whole by uncond."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    cfg = GOAL_ENVELOPE[name]["cfg"]
    G, gd = cfg["goal_seq_len"], cfg["goal_dim"]
    im = GCDenoiser(cfg, 0.5).eval().inner_model
    for bad in (torch.zeros(2, G - 1, gd), torch.zeros(2, G + 1, gd), torch.zeros(2, gd)):
        rows = bad.shape[1] if bad.dim() == 3 else 1
        with pytest.raises(ValueError) as ei:
            im._goals(bad, False)
        assert f"goal_seq_len={G}" in str(ei.value) and f"{rows} token" in str(ei.value), str(ei.value)
    good = torch.ones(2, G, gd)
    assert im._goals(good, False) is good
    z = im._goals(good, True)
    assert tuple(z.shape) == (2, G, gd) and not z.any()


def test_the_references_slicing_rule_stays_with_goal_seq_len_1():
    """A goal as long as the state sequence is cut to its first row only when goal_seq_len == 1 (mdtv_transformer.py:249)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    goal = torch.arange(2 * 3 * 512, dtype=torch.float32).reshape(2, 3, 512)
    one = GCDenoiser(configs.mdtv_default(), 0.5).eval().inner_model
    assert torch.equal(one._goals(goal, False), goal[:, :1])
    three = GCDenoiser(configs.mdtv_default(goal_seq_len=3), 0.5).eval().inner_model
    assert three._goals(goal, False) is goal


def test_train_mode_goal_mask_draws_on_the_goals_shape():
    """goal_drop in train() mode: torch.bernoulli on (B, G, goal_dim), so rows of one sample are masked independently."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    im = GCDenoiser(configs.mdtv_default(goal_seq_len=3, goal_drop=0.5), 0.5).train().inner_model
    torch.manual_seed(3)
    out = im._goals(torch.ones(4, 3, 512), False)
    torch.manual_seed(3)
    mask = torch.bernoulli(torch.ones(4, 3, 512) * 0.5)
    assert torch.equal(out, 1.0 - mask) and not torch.equal(out[:, 0], out[:, 1])


def test_synthetic_inputs_draw_the_goal_sequence_and_keep_todays_values_at_one_row():
    def digest(v):
        return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()[:16]
    # B = 3, seed 6: the digests of the arrays before goal_seq_len was read
    inp = synthetic.sampler_inputs(3, configs.mdtv_default(), 6, "mdtv")
    assert {k: (v.shape, digest(v)) for k, v in inp.items()} == {
        "goal": ((3, 1, 512), "72c8fa5d065ccce4"), "noise": ((3, 10, 7), "d849addc8d35a0fb"), "state_images": ((3, 3, 384), "867cfd9e9b6781f1")}
    inp = synthetic.sampler_inputs(3, configs.mdt_tiny(), 6, "mdt")
    assert {k: (v.shape, digest(v)) for k, v in inp.items()} == {
        "goal": ((3, 1, 512), "72c8fa5d065ccce4"), "noise": ((3, 10, 7), "d849addc8d35a0fb"), "gripper": ((3, 1, 128), "9cec0baaa069fc30"),
        "static": ((3, 1, 128), "88d25c3f4fc6817f")}
    cfg = configs.mdtv_default()
    del cfg["goal_seq_len"]   # a plain dict without the key: one row
    assert digest(synthetic.sampler_inputs(3, cfg, 6)["goal"]) == "72c8fa5d065ccce4"
    g3 = synthetic.sampler_inputs(3, configs.mdtv_default(goal_seq_len=3), 6)
    assert g3["goal"].shape == (3, 3, 512) and g3["goal"].dtype == np.float32
    assert digest(g3["noise"]) == "d849addc8d35a0fb" and digest(g3["state_images"]) == "867cfd9e9b6781f1"
    assert np.array_equal(g3["goal"], synthetic.normal("goal", (3, 3, 512), 6))
