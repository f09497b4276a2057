"""The MAP pooling block at 17 .. 64 tokens on the MI355X (pytest -m gpu): every case of tests/map_long_configs.py
for inference across its batches and for a training step, against float64 through oracle/cla_oracle.map_block (which
tests/test_map_long_golden.py pins to the reference at these shapes) and against what the REFERENCE recorded
(tests/golden/g22_map_long_<name>.npz); three live tapes of both kernel families into one gradient buffer; bit-reproducibility;
the refusals that stay and the ones that went; compute_contrastive_loss end to end at contexts of 17, 18 and 34 tokens.

Gates: those of tests/test_gpu_module_envelope.py -- tests/helpers.assert_close's defaults for outputs, 2e-3 of a tensor's largest
entry for every parameter gradient and d(x).  The reference's own float32 arithmetic lies within 1.2e-6 of the float64 oracle by
that measure at every case (tests/golden/make_golden_map_long.py prints the figure)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import cla_oracle as CO
from tests import envelope_configs as E
from tests import map_long_configs as L
from tests.helpers import assert_close, check_grad_summaries, envelope_params
from tests.map_long_configs import map_long_fixture

pytestmark = pytest.mark.gpu

NAMES = sorted(L.MAP_LONG)
_MODELS = {}


def block_of(kwargs):
    """(MAPBlock on cuda:0, its float32 state dict) with the recorder's 'rich' weights; cases that share constructor kwargs share
    the module, so one handle runs both kernel families and sees its workspace grow and shrink."""
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    key = tuple(sorted(kwargs.items()))
    if key not in _MODELS:
        m = MAPBlock(**kwargs)
        P = envelope_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], L.WEIGHT_SEED)
        m.load_state_dict(P, strict=True)
        _MODELS[key] = (m.cuda().eval(), P)
    return _MODELS[key]


def map_of(name):
    return block_of(L.MAP_LONG[name]["kwargs"])


def tokens(kwargs, B, N, seed):
    return torch.from_numpy(synthetic.normal("ctx", (B, N, kwargs["embed_dim"]), seed))


def f64(P, grad=False):
    return {k: (v.double().requires_grad_() if grad else v.double()) for k, v in P.items()}


def oracle(kwargs, P, x):
    return CO.map_block(P, "", x, kwargs["n_heads"])


def check_grads(module, P64, what):
    n = 0
    for k, p in module.named_parameters():
        ref = P64[k].grad
        assert p.grad is not None and ref is not None, k
        assert_close(p.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what=f"{what} {k}")
        n += 1
    return n


def check_dx(got, ref, what):
    assert_close(got.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-9, what=what)


def train_step(kwargs, B, N, seed):
    """Taped forward + backward with a random cotangent on the HIP module and in float64 through the oracle."""
    model, P = block_of(kwargs)
    x = tokens(kwargs, B, N, seed)
    model.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_()
    out = model(xg)
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(out.shape), seed + 1))
    (out * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    P64 = f64(P, grad=True)
    x64 = x.double().requires_grad_()
    o64 = oracle(kwargs, P64, x64)
    (o64 * cot.double()).sum().backward()
    return model, out.detach(), xg.grad, P64, o64.detach(), x64.grad


@pytest.mark.parametrize("name", NAMES)
def test_inference_across_the_batches(name):
    """mdt_map_pool_forward against the float64 oracle at every batch of the case; a second call is bit-equal; the first and the
    last sample run alone reproduce their rows at the parity gate (one sample and many take different GEMM tilings)."""
    c = L.MAP_LONG[name]
    kw, N = c["kwargs"], c["N"]
    model, P = map_of(name)
    P64 = f64(P)
    for B in c["batches"]:
        x = tokens(kw, B, N, 20 + B)
        want = oracle(kw, P64, x.double())
        with torch.no_grad():
            got = model(x.cuda())
            assert_close(got.cpu(), want, what=f"{name} B = {B}")
            assert torch.equal(model(x.cuda()), got), f"{name} B = {B}: second call differs"
            for i in sorted({0, B - 1}) if B > 1 else ():
                assert_close(model(x[i:i + 1].cuda()).cpu(), got[i:i + 1].cpu(), what=f"{name} sample {i} of {B} alone")


@pytest.mark.parametrize("name", NAMES)
def test_training_step_gradients(name):
    """mdt_map_pool_forward_train + mdt_map_pool_backward: the taped output, every parameter gradient and d(x) against float64
    autograd through the oracle."""
    c = L.MAP_LONG[name]
    model, out, dx, P64, o64, dx64 = train_step(c["kwargs"], c["train_b"], c["N"], 33)
    assert_close(out.cpu(), o64, what=f"{name} taped forward")
    assert check_grads(model, P64, name) == len(P64)
    check_dx(dx, dx64, f"{name} d_x")


@pytest.mark.parametrize("name", sorted(L.MAP_LONG_GOLDEN))
def test_matches_the_reference_golden(name):
    """Output and gradients against what the REFERENCE module gave for the same weights and inputs."""
    meta, fx, P, x, cot = map_long_fixture(name)
    model, PM = map_of(name)
    assert all(torch.equal(P[k], PM[k]) for k in P)
    with torch.no_grad():
        assert_close(model(x.cuda()).cpu(), fx["out"], what=f"{name} vs reference golden")
    model.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_()
    out = model(xg)
    (out * cot.cuda()).sum().backward()
    assert_close(out.detach().cpu(), fx["out"], what=f"{name} taped vs reference golden")
    check_grad_summaries({k: p.grad for k, p in model.named_parameters()}, meta["grads"], name + " (HIP)")
    assert_close(xg.grad.cpu(), fx["d_x"], rtol=2e-3, atol=2e-3 * float(abs(fx["d_x"]).max()), what=name + " d_x")


def test_three_live_tapes_of_both_families_accumulate_into_one_gradient_buffer():
    """The C entry points on one handle: taped forwards at N = 9 (the one-workgroup-per-sample kernels), 17 and 64 (the head-group
    kernels) with different batches, all three tapes alive; then three backwards into ONE flat gradient buffer, which must hold the
    sum over the tapes; then the tapes are released, and a released tape is refused."""
    from mdt_policy_amd import _lib
    kw = L.MAP_LONG["hd3_n17"]["kwargs"]
    model, P = block_of(kw)
    lib, stream = model._engine(torch.device("cuda", 0), train=True)
    h, Q, D = model._handle, kw["n_latents"], kw["output_dim"]
    runs = [(4, 9, 41), (2, 17, 42), (3, 64, 43)]
    xs = [tokens(kw, B, N, seed) for B, N, seed in runs]
    cots = [torch.from_numpy(synthetic.normal("cotangent", (B, Q, D), seed + 10)) for B, _, seed in runs]
    dev_x = [x.cuda() for x in xs]
    outs, tapes = [], []
    for (B, N, _), x in zip(runs, dev_x):
        out = torch.empty((B, Q, D), device="cuda")
        tape = C.c_int32(-1)
        _lib.check(lib.mdt_map_pool_forward_train(h, x.data_ptr(), B, N, out.data_ptr(), C.byref(tape), stream))
        outs.append(out)
        tapes.append(int(tape.value))
    assert len(set(tapes)) == 3
    grads = torch.zeros(model._grad_numel, device="cuda")
    dxs = [torch.empty_like(x) for x in dev_x]
    for tape, cot, dx in zip(tapes, cots, dxs):
        g = cot.cuda()
        _lib.check(lib.mdt_map_pool_backward(h, tape, g.data_ptr(), grads.data_ptr(), dx.data_ptr(), stream))
    for tape in tapes:
        _lib.check(lib.mdt_map_pool_tape_release(h, tape))
    torch.cuda.synchronize()
    assert lib.mdt_map_pool_backward(h, tapes[1], cots[1].cuda().data_ptr(), grads.data_ptr(), None, stream) != 0
    assert b"tape" in lib.mdt_last_error()
    P64 = f64(P, grad=True)
    x64 = [x.double().requires_grad_() for x in xs]
    total = 0
    for x, cot, out in zip(x64, cots, outs):
        o = oracle(kw, P64, x)
        assert_close(out.cpu(), o.detach(), what=f"taped forward at N = {x.shape[1]}")
        total = total + (o * cot.double()).sum()
    total.backward()
    for k, (off, n) in model._grad_layout.items():
        ref = P64[k].grad
        assert_close(grads[off:off + n].view(ref.shape).cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7,
                     what=f"three tapes {k}")
    for x, dx in zip(x64, dxs):
        check_dx(dx, x.grad, f"d_x at N = {x.shape[1]}")


@pytest.mark.parametrize("name", ["clip_n34", "q16_hd256_n64"])
def test_the_same_backward_twice_gives_identical_bits(name):
    c = L.MAP_LONG[name]
    runs = []
    for _ in range(2):
        model, out, dx, *_ = train_step(c["kwargs"], c["train_b"], c["N"], 51)
        runs.append([out.clone(), dx.clone()] + [p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))


def test_sixteen_tokens_keep_their_lds_refusal_and_seventeen_run():
    """The <= 16-token kernels keep their 64 KiB rule: 16 latents x 512 channels is refused at 16 tokens -- m_refused's block
    (tests/envelope_configs.py) and the worst-case block of this table alike, for inference and for training -- and both run at
    17, where the head-group kernels take over."""
    from mdt_policy_amd._lib import MDTHipError
    for kw in (L.MAP_LONG["q16_hd256_n64"]["kwargs"], E.MAP_ENVELOPE["m_refused"]["kwargs"]):
        model, P = block_of(kw)
        x16 = tokens(kw, 2, 16, 61)
        with torch.no_grad(), pytest.raises(MDTHipError, match="LDS budget"):
            model(x16.cuda())
        with pytest.raises(MDTHipError, match="LDS budget"):
            model(x16.cuda().requires_grad_())
        x17 = tokens(kw, 2, 17, 62)
        with torch.no_grad():
            assert_close(model(x17.cuda()).cpu(), oracle(kw, f64(P), x17.double()), what="17 tokens")
        model, out, dx, P64, o64, dx64 = train_step(kw, 2, 17, 63)
        assert_close(out.cpu(), o64, what="17 tokens, taped")
        check_grads(model, P64, "17 tokens")
        check_dx(dx, dx64, "17 tokens d_x")


def test_zero_and_65_tokens_are_refused_by_the_handle():
    """MDT_ERR_UNSUPPORTED (2) with a text that names 1..64, from both entry points, and the block is still right afterwards."""
    from mdt_policy_amd._lib import MDTHipError
    kw = L.MAP_LONG["hd1_n63"]["kwargs"]
    model, P = block_of(kw)
    x = tokens(kw, 2, 65, 71)
    with torch.no_grad(), pytest.raises(MDTHipError, match="1..64 tokens"):
        model(x.cuda())
    with pytest.raises(MDTHipError, match="1..64 tokens"):
        model(x.cuda().requires_grad_())
    lib, stream = model._engine(torch.device("cuda", 0), train=True)
    xd, out, tape = x.cuda(), torch.empty((2, kw["n_latents"], kw["output_dim"]), device="cuda"), C.c_int32(-1)
    assert lib.mdt_map_pool_forward(model._handle, xd.data_ptr(), 2, 0, out.data_ptr(), stream) == 2
    assert b"1..64 tokens" in lib.mdt_last_error()
    assert lib.mdt_map_pool_forward_train(model._handle, xd.data_ptr(), 2, 0, out.data_ptr(), C.byref(tape), stream) == 2
    assert b"1..64 tokens" in lib.mdt_last_error() and tape.value == -1
    with torch.no_grad():
        assert_close(model(x[:, :64].contiguous().cuda()).cpu(), oracle(kw, f64(P), x[:, :64].double()), what="64 tokens")


# ------------------------------------------------------------------------------------------------------- contrastive loss
@pytest.mark.parametrize("style,n_obs_token,pooled", [("map_state_only", 16, 16), ("map", 17, 18), ("map", 33, 34)])
def test_contrastive_loss_end_to_end_at_long_contexts(style, n_obs_token, pooled):
    """compute_contrastive_loss on a narrow MDT-V denoiser (d 128, 4 heads of 32, one encoder and two decoder blocks) whose
    context is goal + n_obs_token tokens, B = 6, with the HIP MAPBlock of ClipStyleProjection(style): value and gradients (goal
    embedders, encoder, pooling head, temperature) against float64 autograd through the two oracles.  'map_state_only' at 17
    tokens pools 16 (the one-workgroup-per-sample kernels), 'map' at 18 and 34 tokens runs the head-group kernels."""
    from mdt_policy_amd import configs
    from mdt_policy_amd.models.contrastive import compute_contrastive_loss
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.models.networks.transformers.transformer_blocks import ClipStyleProjection
    from oracle import mdt_oracle as MO
    from tests.helpers import params_of
    # clip_extra_forward puts the model into train() mode as the reference does: no dropout here, so that the float64 oracles
    # (eval arithmetic) are the exact expectation
    ov = dict(embed_dim=128, obs_dim=128, n_heads=4, n_enc_layers=1, n_dec_layers=2, n_obs_token=n_obs_token, attn_pdrop=0.0,
              resid_pdrop=0.0, mlp_pdrop=0.0)
    cfg = configs.mdtv_default(**ov)
    B = 6
    model = GCDenoiser(cfg, 0.5)
    meta = dict(config="mdtv_default", overrides=ov, arch="mdtv", weight_seed=231, profile="rich",
                state_dict=[[k, list(v.shape)] for k, v in model.state_dict().items()])
    PM = params_of(meta)
    model.load_state_dict(PM)
    model = model.cuda().eval()
    clip = ClipStyleProjection(style, token_dim=128, clip_token_index=1, num_token=1 + n_obs_token)
    PC = envelope_params([(k, tuple(v.shape)) for k, v in clip.state_dict().items()], 232)
    clip.load_state_dict(PC)
    clip = clip.cuda()
    ls = torch.nn.Parameter(torch.tensor(float(np.log(1 / 0.07)), device="cuda"))
    inp = synthetic.sampler_inputs(B, cfg, 31, "mdtv")
    li = synthetic.loss_inputs(B, cfg, 32)
    img_goal = torch.from_numpy(synthetic.normal("img_goal", (B, 1, 512), 33))
    state = {"state_images": torch.from_numpy(inp["state_images"]).cuda(), "modality": "lang"}
    a, nz, sg = (torch.from_numpy(li[k]).cuda() for k in ("actions", "noise_train", "sigma"))
    loss, _ = model.loss(state, a, torch.from_numpy(inp["goal"]).cuda(), nz, sg)
    assert model.inner_model.latent_encoder_emb.shape[1] == 1 + n_obs_token
    cont = compute_contrastive_loss(model, clip, ls, dict(state, modality="vis"), img_goal.cuda(), a, sg, nz)
    (loss + cont).backward()
    # float64 oracles
    P = {k: v.double().requires_grad_(v.dtype.is_floating_point) for k, v in PM.items()}
    Q = {k: v.double().requires_grad_() for k, v in PC.items()}
    st = {"state_images": torch.from_numpy(inp["state_images"]).double(), "modality": "lang"}
    l64, _ = MO.loss(P, cfg, st, torch.from_numpy(li["actions"]).double(), torch.from_numpy(inp["goal"]).double(),
                     torch.from_numpy(li["noise_train"]).double(), torch.from_numpy(li["sigma"]).double())
    ctx_l = MO.encode(P, cfg, st, torch.from_numpy(inp["goal"]).double(), "mdtv", "forward")
    ctx_v = MO.forward_context_only(P, cfg, dict(st, modality="vis"), img_goal.double())
    assert ctx_l.shape[1] == 1 + n_obs_token and pooled == ctx_l.shape[1] - (style == "map_state_only")
    ls64 = torch.tensor(float(np.log(1 / 0.07)), dtype=torch.float64, requires_grad=True)
    c64 = CO.clip_auxiliary_loss(CO.clip_style_projection(Q, ctx_v, style), CO.clip_style_projection(Q, ctx_l, style), ls64)
    (l64 + c64).backward()
    assert abs(cont.item() - c64.item()) <= 1e-3 * abs(c64.item())
    assert abs(ls.grad.item() - ls64.grad.item()) <= 2e-3 * abs(ls64.grad.item()) + 1e-6
    for k, p in clip.named_parameters():
        ref = Q[k].grad
        assert_close(p.grad.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what="clip " + k)
    for k in ("goal_emb.0.weight", "lang_emb.2.weight", "tok_emb.weight", "encoder.blocks.0.attn.key.weight", "encoder.ln.weight",
              "decoder.blocks.1.mlp.c_fc.weight"):
        ref = P["inner_model." + k].grad
        got = dict(model.inner_model.named_parameters())[k].grad
        assert_close(got.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what=k)
