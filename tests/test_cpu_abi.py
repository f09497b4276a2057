"""CPU-tier checks of the drop-in boundary: the C-ABI library builds/loads and exports every declared symbol, the
facade keeps the reference's state_dict contract, and the product path refuses to run without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib, configs
from tests import envelope_configs as EC
from tests.envelope_configs import ENVELOPE
from tests.helpers import MANIFEST, load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    names = set()
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        src = open(os.path.join(ROOT, "include", hdr)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        names |= set(re.findall(r"\b(mdt_[a-z_0-9]+)\s*\(", src))
    return names


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    assert os.path.exists(_lib.library_path())
    decl = declared_symbols()
    assert len(decl) >= 20
    for name in decl:
        assert hasattr(lib, name), f"libmdt_hip.so does not export {name}"
    assert {s[0] for s in _lib.SYMBOLS} == decl, "ctypes table and headers disagree"
    assert b"gfx950" in lib.mdt_version()


def test_code_object_targets_gfx950():
    blob = open(_lib.library_path(), "rb").read()
    assert b"gfx950" in blob and b"v_mfma" not in blob[:0]  # offload bundle names its target
    assert b"amdgcn-amd-amdhsa--gfx950" in blob


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
def test_create_without_gpu_reports_an_error_instead_of_crashing():
    lib = _lib.load()
    cfg = _lib.MDTConfig(arch=0, embed_dim=128, n_heads=8, n_enc_layers=1, n_dec_layers=2, action_dim=7, obs_dim=128,
                         goal_dim=512, n_obs_token=3, goal_seq_len=1, action_seq_len=10, use_mlp_goal=1,
                         use_modality_encoder=1, use_abs_pos_emb=1, use_rot_embed=0, use_ada_conditioning=1,
                         use_noise_encoder=0, linear_output=1, bias=0, sigma_data=0.5)
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value  # MDT_ERR_HIP
    assert b"hipMalloc" in lib.mdt_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(ENVELOPE))
def test_create_accepts_every_envelope_configuration(name):
    """Every configuration the GPU envelope test runs passes mdt_create's validation: without a GPU it gets as far as
    hipMalloc (MDT_ERR_HIP = 4), not MDT_ERR_INVALID_ARG (1) or MDT_ERR_UNSUPPORTED (2)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    e = ENVELOPE[name]
    lib = _lib.load()
    cfg = GCDenoiser(e["cfg"], 0.5).inner_model._hip_config(0.5, proprio=e["proprio"])
    h = C.c_void_p()
    st = lib.mdt_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()



def _resampler_config(kw):
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    return _lib.ResamplerConfig(**PerceiverResampler(**kw)._cfg)


def _map_config(kw):
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    return _lib.MapPoolConfig(**MAPBlock(**kw)._cfg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(EC.RESAMPLER_ENVELOPE))
def test_resampler_create_accepts_every_envelope_configuration(name):
    """As above for mdt_resampler_create, with the config the facade builds from the case's constructor kwargs."""
    lib = _lib.load()
    cfg = _resampler_config(EC.RESAMPLER_ENVELOPE[name]["kwargs"])
    h = C.c_void_p()
    st = lib.mdt_resampler_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks behaviour WITHOUT a GPU")
@pytest.mark.parametrize("name", sorted(EC.MAP_ENVELOPE))
def test_map_pool_create_accepts_every_envelope_configuration(name):
    """As above for mdt_map_pool_create (the over-budget cases too: the LDS budget is a property of a call, not of the
    constructor)."""
    lib = _lib.load()
    cfg = _map_config(EC.MAP_ENVELOPE[name]["kwargs"])
    h = C.c_void_p()
    st = lib.mdt_map_pool_create(C.byref(cfg), C.byref(h))
    assert st == 4 and not h.value, (name, st, lib.mdt_last_error())
    assert b"hipMalloc" in lib.mdt_last_error()


def test_resampler_and_map_pool_create_refuse_what_their_headers_exclude_before_touching_the_device():
    """Each documented constructor refusal comes back as MDT_ERR_INVALID_ARG / MDT_ERR_UNSUPPORTED (never 4 = MDT_ERR_HIP: the
    validation runs before any allocation, with or without a GPU).  ff_mult * dim is a multiple of 16 whenever dim is, so the
    only ff_mult the constructor can refuse is one below 1."""
    lib = _lib.load()
    for bad, status in EC.RESAMPLER_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.ResamplerConfig(**bad)
        assert lib.mdt_resampler_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        assert lib.mdt_last_error()
    for bad, status in EC.MAP_REFUSED_AT_CREATE:
        h = C.c_void_p()
        cfg = _lib.MapPoolConfig(**bad)
        assert lib.mdt_map_pool_create(C.byref(cfg), C.byref(h)) == status and not h.value, bad
        assert lib.mdt_last_error()
    assert lib.mdt_resampler_create(None, None) == 1 and lib.mdt_map_pool_create(None, None) == 1
    # the facade maps MAPBlock(16, 96, 1, 48, mlp_ratio=2.5) onto the refused mlp_hidden = 120
    assert _map_config(dict(n_latents=16, embed_dim=96, n_heads=1, output_dim=48, mlp_ratio=2.5)).mlp_hidden == 120
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    with pytest.raises(NotImplementedError):
        PerceiverResampler(dim=64, depth=1, activation="relu")


@pytest.mark.parametrize("name", sorted(EC.RESAMPLER_GOLDEN))
def test_resampler_facade_state_dict_matches_the_reference_at_the_envelope(name):
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    meta, _ = load_fixture(f"g18_resampler_{name}.npz")
    m = PerceiverResampler(**meta["kwargs"])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in meta["state_dict"]]


@pytest.mark.parametrize("name", sorted(EC.MAP_GOLDEN))
def test_map_block_facade_state_dict_matches_the_reference_at_the_envelope(name):
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    meta, _ = load_fixture(f"g18_map_{name}.npz")
    m = MAPBlock(**meta["kwargs"])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in meta["state_dict"]]


def test_create_rejects_unsupported_configurations_before_touching_the_device():
    lib = _lib.load()
    base = dict(arch=0, embed_dim=128, n_heads=8, n_enc_layers=1, n_dec_layers=2, action_dim=7, obs_dim=128,
                goal_dim=512, n_obs_token=3, goal_seq_len=1, action_seq_len=10, use_mlp_goal=1,
                use_modality_encoder=1, use_abs_pos_emb=1, use_rot_embed=0, use_ada_conditioning=1,
                use_noise_encoder=0, linear_output=1, bias=0, sigma_data=0.5)
    for bad, status in ((dict(use_ada_conditioning=0, n_obs_token=15), 2), (dict(embed_dim=100), 2),
                        (dict(use_rot_embed=1), 1), (dict(arch=5), 1), (dict(sigma_data=0.0), 1),
                        (dict(goal_dim=256), 2), (dict(action_seq_len=17), 2)):
        cfg = _lib.MDTConfig(**dict(base, **bad))
        h = C.c_void_p()
        assert lib.mdt_create(C.byref(cfg), C.byref(h)) == status, bad
        assert lib.mdt_last_error()
    assert lib.mdt_create(None, None) == 1


@pytest.mark.parametrize("key,cfg", [("mdtv_default", configs.mdtv_default()),
                                     ("mdtv_rope", configs.mdtv_default(use_rot_embed=True)),
                                     ("mdtv_tiny", configs.mdtv_tiny()), ("mdt_default", configs.mdt_default()),
                                     ("mdt_tiny", configs.mdt_tiny())])
def test_facade_state_dict_names_shapes_and_order_match_the_reference(key, cfg):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    m = GCDenoiser(cfg, sigma_data=0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == MANIFEST[key]["state_dict"]
    assert [k for k, _ in m.named_parameters()] == MANIFEST[key]["named_parameters"]
    assert m.get_params is not None and m.inner_model.latent_encoder_emb is None


@pytest.mark.parametrize("name", ["bias", "plain_goal", "two_tokens", "mdt_bias_nopos", "no_ada", "noise_block",
                                  "mdt_no_ada", "mlp_head", "mdt_mlp_head", "no_goal_cond", "mdt_no_goal_cond"])
def test_facade_state_dict_of_the_constructor_variants(name):
    """bias / goal embedder / token-count variants and the two other decoder conditionings (plain TransformerDecoder
    without adaLN_zero for use_ada_conditioning=False, NoiseBlock for use_noise_encoder=True)."""
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from tests.helpers import cfg_of
    meta, _ = load_fixture(f"g8_{name}.npz")
    m = GCDenoiser(cfg_of(meta), 0.5)
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta["state_dict"]


def test_facade_initialisation_follows_the_reference_distributions():
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    torch.manual_seed(0)
    im = GCDenoiser(configs.mdtv_default(), 0.5).inner_model
    assert abs(im.decoder.blocks[0].mlp.c_fc.weight.std().item() - 0.02) < 1e-3
    assert im.tok_emb.bias.abs().max().item() == 0
    assert (im.encoder.ln.weight == 1).all() and (im.decoder.blocks[1].ln3.bias == 0).all()
    assert abs(im.decoder.blocks[0].adaLN_zero.modulation[1].weight.std().item() - 0.02) < 1e-3  # NOT zero-init


def test_facade_refuses_cpu_execution():
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    m = GCDenoiser(configs.mdtv_tiny(), 0.5).eval()
    state = {"state_images": torch.zeros(1, 3, 128), "modality": "lang"}
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        m(state, torch.zeros(1, 10, 7), torch.zeros(1, 1, 512), torch.ones(1))
    with pytest.raises(NotImplementedError, match="autograd"):
        m(state, torch.zeros(1, 10, 7), torch.zeros(1, 1, 512), torch.ones(1))
    with pytest.raises(NotImplementedError):  # the reference builds this one but cannot run it
        GCDenoiser(configs.mdt_tiny(goal_conditioned=False, use_ada_conditioning=True), 0.5)
    with pytest.raises(TypeError):
        GCDenoiser(torch.nn.Linear(2, 2), 0.5)


def test_schedules_match_reference_golden():
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    _, fx = load_fixture("g5_schedules.npz")
    for smin in (0.001, 1.0):
        for n in (1, 3, 5, 10, 20):
            np.testing.assert_allclose(gs.get_sigmas_exponential(n, smin, 80.0).numpy(), fx[f"exp_{smin}_{n}"], rtol=1e-6)
    np.testing.assert_allclose(gs.get_sigmas_karras(10, 0.001, 80.0).numpy(), fx["karras_10"], rtol=1e-6)
    np.testing.assert_allclose(gs.get_sigmas_linear(10, 0.001, 80.0).numpy(), fx["linear_10"], rtol=1e-6)
    np.testing.assert_allclose(gs.get_sigmas_ve(10, 0.001, 80.0).numpy(), fx["ve_10"], rtol=1e-6)
    np.testing.assert_allclose(gs.get_sigmas_vp(10).numpy(), fx["vp_10"], rtol=1e-6)


@pytest.mark.parametrize("name", ["ddim", "euler", "heun", "dpmpp_2m"])
def test_host_sampler_loops_against_reference_golden_with_oracle_denoiser(name):
    """The host-side sampler loops (everything except the denoiser call) checked on CPU: plug the ORACLE denoiser
    in as ``model`` and compare with the reference's sampler outputs (G7)."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from oracle import mdt_oracle as O
    from tests.helpers import assert_close, cfg_of, inputs_of, params_of
    meta, fx = load_fixture("g7_samplers.npz")
    cfg, P = cfg_of(meta), params_of(meta)
    state, goal, noise = inputs_of(meta)
    ctx = O.encode(P, cfg, state, goal)
    model = lambda s, x, g, sigma: O.denoise(P, cfg, s, x, g, sigma, ctx=ctx)
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    out = getattr(gs, "sample_" + name)(model, state, noise * 80.0, goal, sig)
    assert_close(out.numpy(), fx[f"{name}_exp"], rtol=1e-4, atol=1e-4, what=name)


def test_flops_accounting_matches_survey():
    """1.812 GFLOP per chunk for MDT-V default, 10 steps; pure host arithmetic mirrored here."""
    D, Te, Ta, A, G, O_ = 384, 4, 10, 7, 512, 384
    attn = lambda tq, tk: 2 * (2 * tq * tk * D)
    enc = 2 * (G * 2 * D + 2 * D * D) + 2 * 3 * O_ * D + 4 * (Te * 2 * 12 * D * D + attn(Te, Te))
    kv = 4 * Te * 2 * 2 * D * D
    blk = 2 * D * 6 * D + Ta * 2 * 4 * D * D + Ta * 2 * 2 * D * D + Ta * 2 * 8 * D * D + attn(Ta, Ta) + attn(Ta, Te)
    step = 2 * (2 * D * D * 2) + 2 * Ta * A * D * 2 + 4 * blk
    total = enc + kv + 10 * step
    assert abs(total / 1e9 - 1.812) < 0.002


@pytest.mark.parametrize("name,kw,key", [
    ("lms", {}, "lms"), ("dpm_2", {}, "dpm_2"), ("dpmpp_2_with_lms", {}, "dpmpp_2_with_lms"), ("dpmpp_2s", {}, "dpmpp_2s"),
    ("euler_ancestral", dict(eta=0.), "euler_ancestral_eta0"), ("dpm_2_ancestral", dict(eta=0.), "dpm_2_ancestral_eta0"),
    ("dpmpp_2s_ancestral", dict(eta=0.), "dpmpp_2s_ancestral_eta0"),
    ("euler_ancestral", dict(seed=1234), "euler_ancestral_seed1234"),
    ("dpm_2_ancestral", dict(seed=1234), "dpm_2_ancestral_seed1234"),
    ("dpmpp_2s_ancestral", dict(seed=1234), "dpmpp_2s_ancestral_seed1234"),
    ("euler", dict(seed=1234, s_churn=4.), "euler_churn_seed1234")])
def test_remaining_sampler_loops_against_reference_golden(name, kw, key):
    """The rest of sample_loop's dispatch table (mdtv_agent.py:619-655) on CPU with the oracle denoiser as ``model``;
    the stochastic samplers consume the torch CPU generator in exactly the reference's order."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from oracle import mdt_oracle as O
    from tests.helpers import assert_close, cfg_of, inputs_of, params_of
    meta, fx = load_fixture("g7b_samplers.npz")
    cfg, P = cfg_of(meta), params_of(meta)
    state, goal, noise = inputs_of(meta)
    ctx = O.encode(P, cfg, state, goal)
    model = lambda s, x, g, sigma: O.denoise(P, cfg, s, x, g, sigma, ctx=ctx)
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    kw = dict(kw)
    if "seed" in kw:
        torch.manual_seed(kw.pop("seed"))
    out = getattr(gs, "sample_" + name)(model, state, noise * 80.0, goal, sig, **kw)
    assert_close(out.numpy(), fx[key], rtol=2e-4, atol=2e-4, what=key)


def _oracle_model(meta):
    from oracle import mdt_oracle as O
    from tests.helpers import cfg_of, inputs_of, params_of
    cfg, P = cfg_of(meta), params_of(meta)
    state, goal, noise = inputs_of(meta)
    ctx = O.encode(P, cfg, state, goal)
    return (lambda s, x, g, sigma: O.denoise(P, cfg, s, x, g, sigma, ctx=ctx)), state, goal, noise


def test_dpm_solver_fast_sde_and_iddpm_against_reference_golden():
    """DPM-Solver-fast (orders 3..3,2,1 / 3..3,r), DPM-Solver++ SDE (deterministic and with a fixed noise tensor) and
    the iDDPM schedule, with the oracle denoiser as ``model``, against outputs of the reference's own code."""
    from mdt_policy_amd import synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from tests.helpers import assert_close
    meta, fx = load_fixture("g7c_samplers.npz")
    model, state, goal, noise = _oracle_model(meta)
    x0 = noise * 80.0
    fixed = torch.from_numpy(synthetic.normal("sde_noise", tuple(x0.shape), meta["noise_seed"]))
    ns = lambda s0, s1: fixed
    for nfe in (9, 10, 11):
        out = gs.sample_dpm_fast(model, state, x0.clone(), goal, 0.001, 80.0, nfe, noise_sampler=ns)
        assert_close(out.numpy(), fx[f"dpm_fast_nfe{nfe}"], rtol=2e-4, atol=2e-4, what=f"dpm_fast nfe={nfe}")
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    out = gs.sample_dpmpp_sde(model, state, x0.clone(), goal, sig, eta=0., noise_sampler=ns)
    assert_close(out.numpy(), fx["dpmpp_sde_eta0"], rtol=2e-4, atol=2e-4, what="dpmpp_sde eta=0")
    out = gs.sample_dpmpp_sde(model, state, x0.clone(), goal, sig, eta=1., noise_sampler=ns)
    assert_close(out.numpy(), fx["dpmpp_sde_eta1_fixednoise"], rtol=2e-4, atol=2e-4, what="dpmpp_sde eta=1")
    np.testing.assert_allclose(gs.get_iddpm_sigmas(10, 0.001, 80.0).numpy(), fx["iddpm_10"], rtol=1e-6)
    np.testing.assert_allclose(gs.get_iddpm_sigmas(20).numpy(), fx["iddpm_20_default"], rtol=1e-6)


def test_dpm_solver_adaptive_converges_to_the_ode_solution():
    """The reference's adaptive solver cannot run (it reads ``noise_sampler`` before assigning it,
    gc_sampling.py:633), so there is no golden: parity unpinned.  Checked instead as a solver: both orders land on
    the probability-flow solution a 200-step DDIM integration reaches, tighter tolerances cost more evaluations, and
    the bookkeeping adds up."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    meta, _ = load_fixture("g7c_samplers.npz")
    model, state, goal, noise = _oracle_model(meta)
    x0 = noise[:2] * 80.0
    st = {"state_images": state["state_images"][:2], "modality": state["modality"]}
    from oracle import mdt_oracle as O
    from tests.helpers import cfg_of, params_of
    cfg, P = cfg_of(meta), params_of(meta)
    ctx = O.encode(P, cfg, st, goal[:2])
    m2 = lambda s, x, g, sigma: O.denoise(P, cfg, s, x, g, sigma, ctx=ctx)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    ref = gs.sample_ddim(m2, st, x0.clone(), goal[:2], gs.get_sigmas_exponential(120, 0.01, 80.0)[:-1])
    res = {}
    for order, rtol in ((3, 0.05), (2, 0.05), (3, 0.005)):
        out, info = gs.sample_dpm_adaptive(m2, st, x0.clone(), goal[:2], 0.01, 80.0, order=order, rtol=rtol,
                                           atol=0.0078 * rtol / 0.05, return_info=True)
        assert info["steps"] == info["n_accept"] + info["n_reject"] and info["nfe"] == order * info["steps"]
        res[(order, rtol)] = ((out - ref).abs().max().item(), info["nfe"])
    assert res[(3, 0.05)][0] < 0.15 and res[(2, 0.05)][0] < 0.15, res            # default tolerances: loose but near
    assert res[(3, 0.005)][0] < 0.05 and res[(3, 0.005)][0] < 0.6 * res[(3, 0.05)][0], res
    assert res[(3, 0.005)][1] > res[(3, 0.05)][1], res                           # accuracy is paid in evaluations
    with pytest.raises(ValueError):
        gs.sample_dpm_adaptive(m2, st, x0, goal[:2], 0.0, 80.0)


def test_headers_are_plain_c():
    """include/*.h is the boundary another host language binds: every header must compile as C11 on its own."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    inc = os.path.join(ROOT, "include")
    for hdr in sorted(os.listdir(inc)):
        r = subprocess.run([gcc, "-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", "-I", inc,
                            os.path.join(inc, hdr)], capture_output=True, text=True)
        assert r.returncode == 0, f"{hdr}: {r.stderr}"


def test_integration_doc_stub_matches_the_config_struct():
    """INTEGRATION.md shows the ctypes stub another host would write: its field list must follow include/mdt_hip.h
    (= _lib.MDTConfig), or the example corrupts the trailing fields."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index("class MDTConfig(C.Structure)"):doc.index("lib.mdt_last_error.restype")]
    names = re.findall(r'"([a-z_0-9]+)"', block)
    assert names == [n for n, _ in _lib.MDTConfig._fields_]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdt_hip.h")).read(), flags=re.S)
    struct = hdr[hdr.index("typedef struct {"):hdr.index("} mdt_config;")]
    assert re.findall(r"(?:int32_t|float)\s+([a-z_0-9]+);", struct) == names


_STRUCTS = {"mdt_config": "MDTConfig", "mdt_gemm_args": "GemmArgs", "mdt_attn_args": "AttnArgs", "mdt_head_args": "HeadArgs",
            "mdt_xfold_args": "XFoldArgs", "mdt_xapply_args": "XApplyArgs", "mdt_dropout": "Dropout",
            "mdt_ln_train_args": "LnTrainArgs", "mdt_ln_bwd_args": "LnBwdArgs", "mdt_attn_train_args": "AttnTrainArgs",
            "mdt_attn_bwd_args": "AttnBwdArgs", "mdt_merge_args": "MergeArgs", "mdt_linear_bwd_args": "LinearBwdArgs",
            "mdt_opt_tensor": "OptTensor", "mdt_map_pool_config": "MapPoolConfig", "mdt_infonce_args": "InfoNCEArgs",
            "mdt_resampler_config": "ResamplerConfig"}
_CTYPE = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float}


def _header_structs():
    """{struct name: [(field, ctypes type)]} parsed from include/*.h (POD structs: scalars and pointers only)."""
    out = {}
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(mdt_[a-z_]+);", src, flags=re.S):
            fields = []
            for decl in body.split(";"):
                decl = " ".join(decl.split())
                if not decl:
                    continue
                m = re.match(r"(?:const )?(\w+)\s*(.*)", decl)
                base, rest = m.group(1), m.group(2)
                for item in rest.split(","):
                    item = item.strip()
                    ptr = item.startswith("*")
                    fields.append((item.lstrip("* "), C.c_void_p if ptr else _CTYPE[base]))
            out[name] = fields
    return out


def test_ctypes_structs_mirror_the_headers_field_by_field():
    """Every POD struct of include/*.h against its ctypes mirror in _lib.py: names, order and types (a field appended to
    a header but not to its mirror silently shifts or truncates the arguments)."""
    hs = _header_structs()
    assert set(hs) == set(_STRUCTS), set(hs) ^ set(_STRUCTS)
    for cname, pyname in _STRUCTS.items():
        got = [(n, t) for n, t in getattr(_lib, pyname)._fields_]
        assert [n for n, _ in got] == [n for n, _ in hs[cname]], cname
        for (n, t), (_, want) in zip(got, hs[cname]):
            assert C.sizeof(t) == C.sizeof(want), f"{cname}.{n}"
            assert (t is C.c_float) == (want is C.c_float), f"{cname}.{n}"


def _kind(ctype):
    if ctype in (C.c_int32, C.c_uint32): return "i32"
    if ctype in (C.c_int64, C.c_uint64): return "i64"
    if ctype is C.c_float: return "f32"
    if ctype is C.c_double: return "f64"
    return "ptr"  # c_void_p, c_char_p, POINTER(...)


def test_ctypes_prototypes_mirror_the_headers():
    """Argument count and kind (pointer / 32-bit / 64-bit integer / float / double) of every function the headers
    declare against the ctypes table."""
    protos = {}
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", hdr)).read(), flags=re.S)
        src = re.sub(r"typedef struct \{.*?\}\s*mdt_[a-z_]+;", "", src, flags=re.S)
        for name, args in re.findall(r"\b(mdt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src):
            kinds = []
            for a in [x.strip() for x in args.split(",")]:
                if a in ("void", ""):
                    continue
                if "*" in a:
                    kinds.append("ptr")
                else:
                    t = a.replace("const ", "").split()[0]
                    kinds.append({"int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "float": "f32",
                                  "double": "f64", "mdt_tape_id": "i32",  # typedef int32_t mdt_tape_id
                                  "mdt_alloc_fn": "ptr", "mdt_free_fn": "ptr"}[t])  # function-pointer typedefs (mdt_set_allocator)
            protos[name] = kinds
    table = {n: [_kind(t) for t in argt] for n, _, argt in _lib.SYMBOLS}
    assert set(protos) == set(table)
    for n, kinds in protos.items():
        assert table[n] == kinds, (n, table[n], kinds)


def test_optimizer_hook_marks_only_the_modules_that_own_a_stepped_parameter():
    """utils/weight_cache.py: torch's fused optimizers do not bump parameter version counters, so an optimizer post-step hook marks
    the registered facade modules dirty -- those that own one of the stepped parameters, and only those."""
    import torch
    from mdt_policy_amd.utils import weight_cache

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn(3))
            self.dirty = 0
            weight_cache.track(self)

        def mark_dirty(self):
            self.dirty += 1

    a, b = Holder(), Holder()
    a.w.grad, b.w.grad = torch.ones(3), torch.ones(3)
    torch.optim.SGD(a.parameters(), lr=0.1).step()
    assert (a.dirty, b.dirty) == (1, 0)
    torch.optim.AdamW(list(a.parameters()) + list(b.parameters()), lr=0.1).step()
    assert (a.dirty, b.dirty) == (2, 1)
    other = torch.nn.Parameter(torch.zeros(2))
    other.grad = torch.ones(2)
    torch.optim.SGD([other], lr=0.1).step()
    assert (a.dirty, b.dirty) == (2, 1)
    del a  # tracked weakly: a dead module is simply gone
    import gc
    gc.collect()
    torch.optim.SGD(b.parameters(), lr=0.1).step()
    assert b.dirty == 2


def test_copies_of_the_facade_modules_are_tracked_by_the_optimizer_hook():
    """copy.deepcopy / pickle go through __getstate__ / __setstate__, not __init__: the copy has to register itself with
    utils/weight_cache.py as well, or a fused torch optimizer stepping the COPY (an EMA or target network that is trained)
    would leave its packed weight images stale (fused optimizers never bump the version counters the cache keys on)."""
    import copy
    import pickle
    import torch
    from mdt_policy_amd import configs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.models.img_generation.masked_transformer_decoder import MaskedTransformerImgDecoder
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    from mdt_policy_amd.utils import weight_cache

    mods = [GCDenoiser(configs.mdtv_tiny(), 0.5).inner_model,
            MaskedTransformerImgDecoder(resolution=32, patch_size=16, decoder_depth=1, decoder_embed_dim=48, decoder_n_heads=2,
                                        context_dim=32, mask_ratio=0.75),
            MAPBlock(n_latents=1, embed_dim=64, n_heads=4, output_dim=None), PerceiverResampler(dim=64, depth=1, dim_head=16, heads=2, num_latents=3)]
    for m in mods:
        for clone in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
            assert clone in weight_cache._tracked, type(m).__name__
            marks = []
            clone.mark_dirty = lambda marks=marks: marks.append(1)
            p = next(q for q in clone.parameters() if q.requires_grad)
            p.grad = torch.zeros_like(p)
            torch.optim.SGD([p], lr=0.1).step()
            assert marks, f"{type(m).__name__}: the optimizer hook did not reach the copy"


@pytest.mark.parametrize("N,K", [(1536, 384), (384, 1536), (1152, 384), (384, 384), (9216, 384), (256, 256), (1024, 256), (192, 192),
                                 (576, 192), (1536, 192), (192, 768), (768, 192), (512, 128), (112, 384), (1024, 384)])
def test_linear_backward_scratch_bound_serves_every_smaller_row_count(N, K):
    """The training handles size `lin_scratch` ONCE, for the largest batch seen, and reuse it for every smaller batch; the slice
    count of the weight-gradient product is not monotone in the row count (n-tile switch at 8192 rows, whole rounds of resident
    workgroups), so mdt_op_linear_bwd_scratch(M) must cover the exact need of every M' <= M (with D = 256, Ta = 11 a
    batch of 219 needed 789 504 floats more than the capacity batch of 256 had been given)."""
    lib = _lib.load()
    caps = [128 * 10, 256 * 11, 128 * 16, 1024 * 10, 8191, 8192, 1024 * 102, 50176]
    for cap in caps:
        bound = lib.mdt_op_linear_bwd_scratch(cap, N, K)
        rows = set(range(1, min(cap, 4096) + 1)) | set(range(4096, cap + 1, 7)) | {cap}
        rows |= {m for b in (8191, 8192, 8193) for m in (b,) if m <= cap}
        worst = max(lib.mdt_op_linear_bwd_scratch_exact(m, N, K) for m in rows)
        assert worst <= bound, f"cap {cap} rows: a smaller batch needs {worst} floats, the bound is {bound}"
    # ... and the bound itself never shrinks as the capacity grows
    prev = 0
    for cap in sorted(set(caps) | {1, 10, 127, 128, 129, 4095, 4096}):
        b = lib.mdt_op_linear_bwd_scratch(cap, N, K)
        assert b >= prev, (cap, b, prev)
        prev = b
