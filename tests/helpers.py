"""Shared test helpers: fixture loading and regeneration of the synthetic weights/inputs behind them."""
import json
import os

import numpy as np
import torch

from mdt_policy_amd import configs, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

with open(os.path.join(GOLDEN, "state_dict_manifest.json")) as _f:
    MANIFEST = json.load(_f)


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name))
    meta = json.loads(str(z["meta"]))
    arrays = {k: z[k] for k in z.files if k != "meta"}
    return meta, arrays


def manifest_key(meta):
    if meta.get("overrides", {}).get("use_rot_embed"):
        return "mdtv_rope"
    return meta["config"]


def cfg_of(meta):
    return configs.NAMED[meta["config"]](**meta.get("overrides", {}))


def rotary_freqs(rot_dim=32, theta=10000.0):
    return 1.0 / (theta ** (torch.arange(0, rot_dim, 2)[: rot_dim // 2].float() / rot_dim))


def params_of(meta, dtype=torch.float32):
    """{state_dict name: tensor} regenerated from the deterministic generator (rotary buffers recomputed)."""
    if "state_dict" in meta:  # variant fixtures carry their own name/shape list
        shapes = [(k, tuple(s)) for k, s in meta["state_dict"]]
    else:
        shapes = [(k, tuple(s)) for k, s in MANIFEST[manifest_key(meta)]["state_dict"]]
    P = {k: torch.from_numpy(v) for k, v in
         synthetic.fill_state_dict(shapes, meta["weight_seed"], meta["profile"]).items()}
    for k, s in shapes:
        if k.endswith("rotary_pos_emb.freqs"):
            P[k] = rotary_freqs(2 * s[0])
    if not cfg_of(meta).get("use_modality_encoder", False):  # lang_emb is goal_emb under a second name
        for k in list(P):
            if k.startswith("inner_model.lang_emb"):
                P[k] = P[k.replace("inner_model.lang_emb", "inner_model.goal_emb")]
    return {k: v.to(dtype) for k, v in P.items()}


def observation(cfg, arch, proprio, B, seed, dtype=torch.float32, obs_seed=None):
    """(state, goal, noise) on the host from synthetic.sampler_inputs; with ``proprio`` also state_obs (B, 1, proprio_dim), drawn
    at ``obs_seed`` (``seed`` when that is None)."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in synthetic.sampler_inputs(B, cfg, seed, arch).items()}
    if arch == "mdtv":
        state = {"state_images": t["state_images"], "modality": "lang"}
    else:
        state = {"static": t["static"], "gripper": t["gripper"], "modality": "lang"}
    if proprio:
        obs_seed = seed if obs_seed is None else obs_seed
        state["state_obs"] = torch.from_numpy(synthetic.normal("state_obs", (B, 1, cfg["proprio_dim"]), obs_seed)).to(dtype)
    return state, t["goal"], t["noise"]


def inputs_of(meta, dtype=torch.float32, batch=None):
    state, goal, noise = observation(cfg_of(meta), meta["arch"], False, batch or meta["B"], meta["input_seed"], dtype)
    return dict(state, modality=meta["modality"]), goal, noise


def to(state, fn):
    """The observation dict with ``fn`` applied to its tensors."""
    return {k: (fn(v) if torch.is_tensor(v) else v) for k, v in state.items()}


def cuda(t):
    return to(t, torch.Tensor.cuda) if isinstance(t, dict) else t.cuda()


def rich_weights(model, seed=5):
    """Loads the 'rich' synthetic weights of the model's own state_dict() shapes (strict=False: rotary buffers as drawn, lang_emb
    not aliased -- unlike params_of's recipe, which recorded fixtures rest on) and returns them, {name: float32 tensor}."""
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed, "rich").items()}
    model.load_state_dict(P, strict=False)
    return P


def rich_model(cfg):
    """(GCDenoiser(cfg, 0.5) on the host with rich_weights, those weights); the caller moves it: ``.cuda().eval()``."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    torch.manual_seed(0)
    m = GCDenoiser(cfg, 0.5)
    return m, rich_weights(m)


RTOL, ATOL = 1e-3, 1e-4  # BASELINE.json north_star parity gate


def assert_close(got, want, rtol=RTOL, atol=ATOL, what=""):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = np.abs(got - want)
    tol = atol + rtol * np.abs(want)
    bad = err > tol
    assert not bad.any(), (f"{what}: {bad.sum()}/{bad.size} outside rtol={rtol} atol={atol}; "
                           f"max abs err {err.max():.3e} (|want| max {np.abs(want).max():.3e})")


def perceiver_case(name):
    """(meta, fixture arrays, params, media tokens, mask) of a g9 Perceiver-resampler fixture."""
    meta, fx = load_fixture(f"g9_perceiver_{name}.npz")
    shapes = [(k, tuple(s)) for k, s in meta["state_dict"]]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, meta["weight_seed"], meta["profile"]).items()}
    x = torch.from_numpy(synthetic.normal("media", (meta["B"], meta["T"], meta["n"], meta["kwargs"]["dim"]),
                                          meta["input_seed"]))
    mask = None if meta["mask"] is None else torch.tensor(meta["mask"], dtype=torch.bool)
    return meta, fx, P, x, mask


def envelope_params(shapes, seed):
    return {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict([(k, tuple(s)) for k, s in shapes], seed, "rich").items()}


def resampler_envelope_fixture(name):
    """(meta, fixture arrays, params, media tokens, mask, cotangent) of a g18 resampler fixture (tests/envelope_configs.py)."""
    meta, fx = load_fixture(f"g18_resampler_{name}.npz")
    P = envelope_params(meta["state_dict"], meta["weight_seed"])
    x = torch.from_numpy(synthetic.normal("media", (meta["B"], meta["T"], meta["n"], meta["kwargs"]["dim"]), meta["input_seed"]))
    mask = None if meta["mask"] is None else torch.tensor(meta["mask"], dtype=torch.bool)
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(fx["out"].shape), meta["cot_seed"]))
    return meta, fx, P, x, mask, cot


def map_envelope_fixture(name):
    """(meta, fixture arrays, params, tokens, cotangent) of a g18 MAPBlock fixture."""
    meta, fx = load_fixture(f"g18_map_{name}.npz")
    P = envelope_params(meta["state_dict"], meta["weight_seed"])
    x = torch.from_numpy(synthetic.normal("ctx", (meta["B"], meta["N"], meta["kwargs"]["embed_dim"]), meta["input_seed"]))
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(fx["out"].shape), meta["cot_seed"]))
    return meta, fx, P, x, cot


def grad_summary(g):
    g = g.detach().double().cpu()
    return [float(g.norm()), float(g.sum())] + [float(v) for v in g.flatten()[:6]]


def check_grad_summaries(named_grads, want, what):
    """The oracle-vs-reference gate of test_perceiver.py / test_cla.py: each summary to 2e-3 of the gradient's norm."""
    assert set(named_grads) == set(want), what
    for k, w in want.items():
        g, w = np.array(grad_summary(named_grads[k])), np.array(w)
        tol = 2e-3 * abs(w[0]) + 1e-6
        assert np.all(np.abs(g - w) <= tol), f"{what} {k}: {g} vs {w}"


def mae_inputs(kw, B, n_ctx, seed):
    """(context, images, mask noise) of a masked-image head case from the deterministic generator."""
    n = (kw["resolution"] // kw["patch_size"]) ** 2
    ctx = torch.from_numpy(synthetic.normal("ctx", (B, n_ctx, kw["context_dim"]), seed))
    img = torch.from_numpy(synthetic.normal("img", (B, 2, kw["in_channels"], kw["resolution"], kw["resolution"]), seed + 1))
    noise = torch.from_numpy(synthetic.uniform("mask_noise", (B, n) if kw["symmetric_mask"] else (B, 2, n), seed + 2))
    return ctx, img, noise


def mae_params(state_dict_shapes, kw, seed=151, profile="rich"):
    """{state_dict name: tensor} of a head: the generator's values, decoder_pe from the oracle's position table."""
    from oracle import mae_oracle as O
    shapes = [(k, tuple(s)) for k, s in state_dict_shapes if k != "decoder_pe"]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed, profile).items()}
    table = O.position_table(kw["decoder_embed_dim"], kw["resolution"] // kw["patch_size"])
    P["decoder_pe"] = torch.from_numpy(table).float().unsqueeze(0)
    return P


def mae_envelope_fixture(name):
    """(meta, fixture arrays, params, context, images, shuffle) of a g15 envelope fixture (tests/envelope_configs.py MAE_GOLDEN)."""
    meta, fx = load_fixture(f"g15_mae_{name}.npz")
    kw = meta["kwargs"]
    P = mae_params(meta["state_dict"], kw, meta["weight_seed"], meta["profile"])
    ctx = torch.from_numpy(synthetic.normal("ctx", (meta["B"], meta["Tc"], kw["context_dim"]), meta["ctx_seed"]))
    img = torch.from_numpy(synthetic.normal("img", (meta["B"], 2, kw["in_channels"], kw["resolution"], kw["resolution"]), meta["img_seed"]))
    shuffle = torch.argsort(torch.from_numpy(fx["restore"]), dim=1)
    return meta, fx, P, ctx, img, shuffle
