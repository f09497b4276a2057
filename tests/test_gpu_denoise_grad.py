"""GCDenoiser.denoise_grad: D(x; sigma) recorded by torch.autograd on the HIP path (mdt_train_denoise_fwd / _bwd behind
_autograd.HipDenoise) against float64 torch.autograd through the oracle (oracle/mdt_oracle.py: encode, decode / denoise).

Bounds: the forward value rtol 1e-3 / atol 1e-4 (the project's forward tolerance); every gradient rtol 2e-3 and
atol 2e-3 * max |ref| + 1e-7 per tensor (test_train_grads.py).  The unrolled-steps test measures its bound in the test itself
(see there).  Every check prints its largest error as a fraction of its tolerance."""
import math

import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import mdt_oracle as O
from tests.helpers import assert_close, params_of
from tests.test_gpu_train_dropout import (CachedMasks, check_gradients, grads_of, hip_grads, load_case, on_device, oracle_leaves,
                                          spy_seeds, worst)

pytestmark = pytest.mark.gpu

SD = 0.5  # sigma_data of every model here


def facade(meta, cfg, train=False):
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model = GCDenoiser(cfg, SD)
    model.load_state_dict(params_of(meta))
    model = model.cuda()
    return model.train() if train else model.eval()


def leaves(state, goal, li):
    """The HIP side's differentiable inputs: state tensors, goal, the noisy actions and sigma."""
    gstate = {k: (v.cuda().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    x = (li["actions"] + li["noise_train"] * li["sigma"][:, None, None]).cuda().requires_grad_()
    return gstate, goal.cuda().requires_grad_(), x, li["sigma"].cuda().requires_grad_()


def upstream(shape, seed=3):
    """The random upstream weight w of L = (D . w).sum(): standard normal draws."""
    return torch.from_numpy(synthetic.normal("denoised_weight", tuple(shape), seed))


def sibling_scale(ref, k):
    """max |ref| of the query bias beside key bias ``k``, where ``k``'s own reference gradient is zero in exact arithmetic; else None.

    A key bias without RoPE shifts every score of a softmax row by the same amount, so its gradient is exactly zero and the
    float64 reference holds ~1e-16 of rounding.  Its tensor bound 2e-3 * max |ref| + 1e-7 then is the absolute floor alone, which
    was set for the mean-reduced diffusion loss (seed dF = 2 (F - target) / n) and says nothing about L = (D . w).sum() with
    unit-variance w, whose upstream gradient is ~n times larger: what a float32 backward leaves in such a tensor is rounding noise
    proportional to the upstream gradient.  The gradient is the column sum of dK, formed by the same launches, over the same rows
    and from scores of the same size as the query bias's column sum of dQ in the same attention; so it is held to what that sibling
    is held to in absolute terms, 2e-3 * max |ref(query.bias)| + 1e-7.  Every other tensor keeps its own bound."""
    if not k.endswith(".key.bias") or ref.get(k) is None:
        return None
    q = ref.get(k[:-len("key.bias")] + "query.bias")
    if q is None:
        return None
    qs = float(q.abs().max())
    return qs if float(ref[k].abs().max()) <= 1e-9 * qs else None


def check_grads(got, ref, what, at_least):
    """tests/test_gpu_train_dropout.check_gradients with the exactly-zero key biases on their sibling's scale (sibling_scale)."""
    zero = {k: sibling_scale(ref, k) for k in ref}
    zero = {k: v for k, v in zero.items() if v is not None}
    for k, qs in zero.items():
        assert got.get(k) is not None, f"{what} {k}: no gradient"
        err, atol = float((got[k].double() - ref[k]).abs().max()), 2e-3 * qs + 1e-7
        assert err <= atol, f"{what} {k}: zero in exact arithmetic, max abs err {err:.3e} > {atol:.3e} (query bias scale {qs:.3e})"
    if zero:
        worst_k = max(zero, key=lambda k: float((got[k].double() - ref[k]).abs().max()) / (2e-3 * zero[k] + 1e-7))
        print(f"{what}: {len(zero)} key biases zero in exact arithmetic, largest |got| "
              f"{max(float(got[k].abs().max()) for k in zero):.3e} (bound of {worst_k}: {2e-3 * zero[worst_k] + 1e-7:.3e})")
    check_gradients({k: v for k, v in got.items() if k not in zero}, {k: v for k, v in ref.items() if k not in zero}, what,
                    at_least=at_least - len(zero))


def all_grads(model, gstate, ggoal, x, sigma):
    got = hip_grads(model, gstate, ggoal)
    got["d_x"] = x.grad.cpu() if x.grad is not None else None
    got["d_sigma"] = sigma.grad.cpu() if sigma.grad is not None else None
    return got


def oracle_run(meta, cfg, state, goal, li, fn, sigma_grad=True):
    """fn(denoise, x64, sigma64, dev) -> scalar, with denoise(x, sigma, uncond=False) the float64 oracle's D; returns
    (value, {name: gradient}) with the parameters, d_<state key>, d_goal, d_x, d_sigma."""
    def run(dev):
        P, st, g64 = oracle_leaves(meta, state, goal, dev)
        x = (li["actions"] + li["noise_train"] * li["sigma"][:, None, None]).double().to(dev).requires_grad_()
        sg = li["sigma"].double().to(dev).requires_grad_(sigma_grad)

        def denoise(x_, s_, uncond=False):
            g = torch.zeros_like(g64) if uncond else g64
            return O.denoise(P, cfg, st, x_, g, s_, SD, meta["arch"])

        val = fn(denoise, x, sg, dev)
        val.backward()
        out = grads_of(P, st, g64)
        out["d_x"] = x.grad.cpu()
        out["d_sigma"] = sg.grad.cpu() if sg.grad is not None else None
        return val.item(), out
    return on_device(run)


CASES = [("mdtv_tiny", None), ("mdtv_default", None), ("mdt_tiny", None), ("mdtv_rope", None), ("mdtv_noise_block", None),
         ("mdtv_no_ada", None), ("proprio_default", None), ("mdtv_no_goal_cond", None), ("mdtv_mlp_head", None),
         ("mdtv_default", 96)]  # 96 x 10 action rows: a batch at which the inference path's bf16-split launches are the default


@pytest.mark.parametrize("name,B", CASES, ids=[n + (f"-B{b}" if b else "") for n, b in CASES])
def test_value_and_every_gradient_for_a_random_upstream_weight(name, B):
    """L = (D . w).sum(): the forward value, then the gradient of every parameter, the state tensors, the goal, the noisy actions
    and sigma.  Sigma-token models (use_ada_conditioning=False): everything but d_sigma, and sigma.requires_grad raises."""
    meta, cfg, state, goal, li = load_case(name, B=B)
    model = facade(meta, cfg)
    token = not cfg.get("use_ada_conditioning", False)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    if token:
        with pytest.raises(NotImplementedError, match="context token"):
            model.denoise_grad(gstate, x, ggoal, sigma)
        sigma = sigma.detach()
    w = upstream(x.shape)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    assert den.requires_grad and model.inner_model.latent_encoder_emb is not None
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    vals = {}

    def objective(denoise, x64, s64, dev):
        vals["den"] = denoise(x64, s64)
        return (vals["den"] * w.double().to(dev)).sum()

    _, ref = oracle_run(meta, cfg, state, goal, li, objective, sigma_grad=not token)
    print(f"{name}: denoised {worst(den.detach().cpu(), vals['den'].detach().cpu(), 1e-3, 1e-4):.3f} of its tolerance")
    assert_close(den.detach().cpu(), vals["den"].detach().cpu(), rtol=1e-3, atol=1e-4, what=name + " denoised")
    got = all_grads(model, gstate, ggoal, x, sigma)
    if token:
        assert got.pop("d_sigma") is None and ref.pop("d_sigma") is None
    else:
        assert got["d_sigma"] is not None and got["d_sigma"].shape == li["sigma"].shape
    check_grads(got, ref, name, at_least=30)
    with torch.no_grad():  # without a graph it IS forward
        a, b = model.denoise_grad(gstate, x, ggoal, sigma), model(gstate, x, ggoal, sigma)
    assert torch.equal(a, b)
    assert_close(a.cpu(), den.detach().cpu(), rtol=1e-3, atol=1e-4, what=name + " no_grad vs taped forward")


def test_gradients_at_the_c3_batch_b1024():
    """BASELINE configs[2] at its own size (10 240 action rows): the batched split-K weight-gradient products and the d_sigma
    reduction over 1024 samples."""
    name, B = "mdtv_default", 1024
    meta, cfg, state, goal, li = load_case(name, B=B)
    model = facade(meta, cfg)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    w = upstream(x.shape)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    _, ref = oracle_run(meta, cfg, state, goal, li, lambda denoise, x64, s64, dev: (denoise(x64, s64) * w.double().to(dev)).sum())
    check_grads(all_grads(model, gstate, ggoal, x, sigma), ref, "B=1024", at_least=100)


def huber(r, delta=0.3):
    a = r.abs()
    return torch.where(a <= delta, 0.5 * r * r, delta * (a - 0.5 * delta))


def test_custom_huber_objective_end_to_end_and_the_optimizer_step_reaches_the_next_forward():
    """Huber loss on D - a with a per-dimension weight: value and every gradient against the oracle; then FusedAdamW.step() must
    change what the next forward returns (the weight cache sees the update on this path too)."""
    from mdt_policy_amd.optim.fused_adamw import FusedAdamW
    name = "mdtv_tiny"
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    wd = torch.linspace(0.5, 2.0, cfg["action_dim"])
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    loss = (huber(den - li["actions"].cuda()) * wd.cuda()).mean()
    loss.backward()
    torch.cuda.synchronize()
    val, ref = oracle_run(meta, cfg, state, goal, li, lambda denoise, x64, s64, dev:
                          (huber(denoise(x64, s64) - li["actions"].double().to(dev)) * wd.double().to(dev)).mean())
    print(f"huber: loss {loss.item():.7g} / oracle {val:.7g}")
    assert abs(loss.item() - val) <= 1e-3 * abs(val)
    check_grads(all_grads(model, gstate, ggoal, x, sigma), ref, "huber", at_least=30)
    opt = FusedAdamW([p for p in model.parameters() if p.grad is not None], lr=1e-2)
    opt.step()
    with torch.no_grad():
        after = model.denoise_grad(gstate, x, ggoal, sigma)
    den2 = model.denoise_grad(gstate, x.detach(), ggoal.detach(), sigma.detach())  # the taped forward reads the new weights too
    assert float((after - den.detach()).abs().max()) > 1e-3
    assert_close(den2.detach().cpu(), after.cpu(), rtol=1e-3, atol=1e-4, what="taped vs plain forward after the step")


@pytest.mark.parametrize("name", ["mdtv_tiny", "mdtv_noise_block", "mdt_tiny"])
def test_reference_loss_written_on_denoise_grad_agrees_with_loss_backward(name):
    """score_wrappers.py:45-63 in torch on denoise_grad's output: ((D - c_skip x) / c_out - target)^2, the same kernels downstream
    of the seed as model.loss(...).backward()."""
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    gstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    a, nz, sg = li["actions"].cuda(), li["noise_train"].cuda(), li["sigma"].cuda()
    l0, _ = model.loss(gstate, a, goal.cuda(), nz, sg)
    l0.backward()
    want = {k: p.grad.clone() for k, p in model.inner_model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    c_skip, c_out, _ = [c[:, None, None] for c in model.get_scalings(sg)]
    noised = a + nz * sg[:, None, None]
    den = model.denoise_grad(gstate, noised, goal.cuda(), sg)
    l1 = (((den - c_skip * noised) / c_out - (a - c_skip * noised) / c_out) ** 2).flatten(1).mean()
    l1.backward()
    assert abs(l1.item() - l0.item()) <= 1e-3 * abs(l0.item())
    n, top = 0, 0.0
    for k, p in model.inner_model.named_parameters():
        if k not in want:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        r = want[k].cpu()
        atol = 2e-3 * float(r.abs().max()) + 1e-7
        top = max(top, worst(p.grad.cpu(), r, 2e-3, atol))
        assert_close(p.grad.cpu(), r, rtol=2e-3, atol=atol, what=k)
        n += 1
    print(f"{name}: {n} gradients against loss.backward(), largest error {top:.3f} of its tolerance")
    assert n >= 30


def test_guidance_gradients_against_the_two_evaluation_formula():
    name, lam = "mdtv_tiny", 2.5
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    w = upstream(x.shape)
    den = model.denoise_grad(gstate, x, ggoal, sigma, cond_lambda=lam)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert_close(den.detach().cpu(), model(gstate, x, ggoal, sigma, cond_lambda=lam).cpu(), rtol=1e-3, atol=1e-4, what="guided value")

    def objective(denoise, x64, s64, dev):
        d_u, d_g = denoise(x64, s64, uncond=True), denoise(x64, s64)
        return ((d_u + lam * (d_g - d_u)) * w.double().to(dev)).sum()

    _, ref = oracle_run(meta, cfg, state, goal, li, objective)
    check_grads(all_grads(model, gstate, ggoal, x, sigma), ref, "cond_lambda=2.5", at_least=30)


def ddim_unrolled(denoise, x, sigmas):
    """Four hand-unrolled DDIM steps (gc_sampling.py:946-950) on any denoise(x, sigma) -> D."""
    s_in = x.new_ones([x.shape[0]])
    for i in range(len(sigmas) - 1):
        den = denoise(x, sigmas[i] * s_in)
        t, t_next = -math.log(sigmas[i]), -math.log(sigmas[i + 1])
        x = (math.exp(-t_next) / math.exp(-t)) * x - math.expm1(-(t_next - t)) * den
    return x


def test_four_unrolled_ddim_steps_share_one_context():
    """One forward_context_only under autograd, four denoise_grad(..., context=ctx), a scalar of the final chunk: gradients of the
    parameters, the initial noise and the state tokens against float64 autograd through the oracle's same four steps.

    Errors compound over the steps, so the bound is measured here: the oracle in float32 on the CPU, its per-tensor deviation
    from the float64 result, and the HIP result is allowed 4x that (the different summation order and the split launches'
    <= 1.5x per-product allowance) -- never less than the single-evaluation bound 2e-3 * max |ref| + 1e-7.  Both deviations and
    their largest ratio are printed; DESIGN.md section 8a is where the observed ratio belongs."""
    name = "mdtv_tiny"
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    sigmas = [float(v) for v in O.get_sigmas_exponential(4, 0.05, 2.0)[:5]]
    sigmas[-1] = 0.02  # the schedule's appended zero has no DDIM step through ln(sigma)
    x0 = li["noise_train"] * sigmas[0]
    w = upstream(x0.shape, seed=9)
    gstate = {k: (v.cuda().requires_grad_() if torch.is_tensor(v) else v) for k, v in state.items()}
    ggoal, gx = goal.cuda().requires_grad_(), x0.cuda().requires_grad_()
    ctx = model.forward_context_only(gstate, None, ggoal, torch.full((x0.shape[0],), sigmas[0], device="cuda"))
    out = ddim_unrolled(lambda x, s: model.denoise_grad(None, x, None, s, context=ctx), gx, sigmas)
    (out * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    got = hip_grads(model, gstate, ggoal)
    got["d_x"] = gx.grad.cpu()

    def oracle(dtype, dev):
        P, st, g = oracle_leaves(meta, state, goal, dev)
        P = {k: v.detach().to(dtype).requires_grad_(v.requires_grad) for k, v in P.items()}
        st = {k: (v.detach().to(dtype).requires_grad_() if torch.is_tensor(v) else v) for k, v in st.items()}
        g = g.detach().to(dtype).requires_grad_()
        x = x0.to(dtype).to(dev).requires_grad_()
        c = O.forward_context_only(P, cfg, st, g, meta["arch"])
        o = ddim_unrolled(lambda x_, s_: O.denoise(P, cfg, st, x_, g, s_, SD, meta["arch"], ctx=c), x, sigmas)
        (o * w.to(dtype).to(dev)).sum().backward()
        r = grads_of(P, st, g)
        r["d_x"] = x.grad.cpu()
        return o.detach().cpu(), r

    o64, ref = on_device(lambda dev: oracle(torch.float64, dev))
    _, r32 = oracle(torch.float32, "cpu")
    assert_close(out.detach().cpu(), o64, rtol=4e-3, atol=4e-4, what="final chunk")  # four evaluations of the 1e-3 / 1e-4 forward
    n, top_ratio = 0, (0.0, "")
    for k, r in ref.items():
        if r is None:
            assert got.get(k) is None or float(got[k].abs().max()) == 0.0, k
            continue
        qs = sibling_scale(ref, k)  # a key bias that is zero in exact arithmetic: its query bias's scale
        single = 2e-3 * (float(r.abs().max()) if qs is None else qs) + 1e-7
        dev32 = float((r32[k].double() - r).abs().max())
        devhip = float((got[k].double() - r).abs().max())
        bound = max(4.0 * dev32, single)
        top_ratio = max(top_ratio, (devhip / max(dev32, 1e-30), k)) if dev32 > 0 else top_ratio
        print(f"unrolled {k}: HIP deviation {devhip:.3e}, float32 oracle {dev32:.3e}, bound {bound:.3e}")
        assert devhip <= bound, (k, devhip, dev32, bound)
        n += 1
    print(f"unrolled: {n} gradients, largest HIP / float32-oracle deviation ratio {top_ratio[0]:.2f} ({top_ratio[1]})")
    assert n >= 30 and got["d_state_images"] is not None


def test_train_mode_replays_the_shipped_dropout_masks():
    """train() mode, the shipped dropouts (0.3 / 0.1 / 0.05): one seed per evaluation covers the encoder's and the decoder's
    sites; the float64 oracle multiplies with the replayed Philox masks (tests/dropout_masks.py)."""
    name = "mdtv_tiny"
    meta, cfg, state, goal, li = load_case(name)
    assert (cfg["attn_pdrop"], cfg["resid_pdrop"], cfg["mlp_pdrop"]) == (0.3, 0.1, 0.05)
    model = facade(meta, cfg, train=True)
    seeds = spy_seeds(model.inner_model)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    w = upstream(x.shape)
    torch.manual_seed(31)
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    (den * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert len(seeds) == 1 and seeds[0] > 0

    def run(dev):
        P, st, g64 = oracle_leaves(meta, state, goal, dev)
        x64 = x.detach().double().to(dev).requires_grad_()
        s64 = li["sigma"].double().to(dev).requires_grad_()
        masks = CachedMasks.of(seeds[0], cfg)
        c_skip, c_out, c_in = [s[:, None, None] for s in O.get_scalings(s64, SD)]
        c = O.encode(P, cfg, st, g64, meta["arch"], "forward", sigma=s64, masks=masks)
        d = O.decode(P, cfg, c, x64 * c_in, s64, masks=masks) * c_out + x64 * c_skip
        (d * w.double().to(dev)).sum().backward()
        r = grads_of(P, st, g64)
        r["d_x"], r["d_sigma"] = x64.grad.cpu(), s64.grad.cpu()
        return d.detach().cpu(), r

    d64, ref = on_device(run)
    print(f"train mode: denoised {worst(den.detach().cpu(), d64, 1e-3, 1e-4):.3f} of its tolerance")
    assert_close(den.detach().cpu(), d64, rtol=1e-3, atol=1e-4, what="train-mode denoised")
    check_grads(all_grads(model, gstate, ggoal, x, sigma), ref, "train mode", at_least=30)
    model.eval()
    with torch.no_grad():
        assert float((model(gstate, x, ggoal, sigma) - den.detach()).abs().max()) > 1e-3  # the masks matter


@pytest.mark.parametrize("name", ["mdtv_tiny", "mdtv_noise_block"])
def test_two_backwards_of_identical_forwards_give_identical_bits(name):
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        gstate, ggoal, x, sigma = leaves(state, goal, li)
        den = model.denoise_grad(gstate, x, ggoal, sigma)
        (den * upstream(x.shape).cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((den.detach().clone(), all_grads(model, gstate, ggoal, x, sigma)))
    (d0, g0), (d1, g1) = runs
    assert torch.equal(d0, d1) and set(g0) == set(g1) and g0["d_sigma"] is not None
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None) and (g0[k] is None or torch.equal(g0[k], g1[k])), f"{k} differs between two runs"


def test_tape_lifecycle_and_the_c_abi_refusals():
    import ctypes as C
    from mdt_policy_amd import _lib
    name = "mdtv_tiny"
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    gstate, ggoal, x, sigma = leaves(state, goal, li)
    # a second backward: the tape is gone
    den = model.denoise_grad(gstate, x, ggoal, sigma)
    den.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed"):
        den.sum().backward()
    # 40 forwards whose graphs are dropped without a backward hand their tapes back (two tapes each: encoder and decoder)
    for _ in range(40):
        model.denoise_grad(gstate, x, ggoal, sigma)
    ctx = model.forward_context_only(gstate, None, ggoal, sigma.detach())
    live = []
    with pytest.raises(RuntimeError, match="more than 16 tapes alive"):  # a host-side status: nothing is enqueued for the 17th
        for _ in range(17):
            live.append(model.denoise_grad(None, x, None, sigma, context=ctx))
    assert len(live) == 15  # the context's own tape is the sixteenth
    del live
    den = model.denoise_grad(None, x, None, sigma, context=ctx)  # the pool is free again
    den.sum().backward()
    assert x.grad is not None and gstate["state_images"].grad is not None
    # a detached context: the encoder's parameters take no gradient
    model.zero_grad(set_to_none=True)
    model.denoise_grad(None, x, None, sigma, context=ctx.detach()).sum().backward()
    grads = {k: p.grad for k, p in model.inner_model.named_parameters()}
    assert grads["encoder.blocks.0.mlp.c_fc.weight"] is None and grads["tok_emb.weight"] is None
    assert grads["decoder.blocks.0.mlp.c_fc.weight"] is not None and grads["sigma_emb.1.weight"] is not None
    # the implicit call stays inference-only and points at the explicit one
    with pytest.raises(NotImplementedError, match="autograd.*denoise_grad"):
        model(gstate, x, ggoal, sigma)
    # C ABI: argument, state and tape refusals (host-side statuses)
    eng = model._engine(allow_grad=True, state=gstate)
    lib, h = eng.lib, eng.handle
    B = x.shape[0]
    out, tape = torch.empty_like(x), C.c_int32(-1)
    c_, x_, s_ = ctx.detach().contiguous(), x.detach().contiguous(), sigma.detach().contiguous()
    assert lib.mdt_train_denoise_fwd(h, None, x_.data_ptr(), s_.data_ptr(), B, None, out.data_ptr(), C.byref(tape), None) == 1
    assert lib.mdt_train_denoise_fwd(h, c_.data_ptr(), x_.data_ptr(), s_.data_ptr(), 0, None, out.data_ptr(), C.byref(tape), None) == 1
    assert lib.mdt_train_denoise_fwd(h, c_.data_ptr(), x_.data_ptr(), s_.data_ptr(), B, None, out.data_ptr(), None, None) == 1
    assert lib.mdt_train_denoise_bwd(h, 999, out.data_ptr(), None, None, None, None, None) == 1      # unknown tape
    assert b"invalid or released tape" in lib.mdt_last_error()
    _, enc_tape = eng.train_encode_fwd(gstate, *model._train_inputs(eng, gstate, ggoal, True)[:3], True)
    assert lib.mdt_train_denoise_bwd(h, enc_tape, out.data_ptr(), None, None, None, None, None) == 5  # MDT_ERR_STATE: not its tape
    eng.tape_release(enc_tape)
    _, t2 = eng.train_denoise_fwd(c_, x_, s_)
    assert lib.mdt_train_denoise_bwd(h, t2, None, None, None, None, None, None) == 1                 # no upstream gradient
    g_ctx = torch.empty_like(c_)
    grads_buf = torch.zeros(eng._grad_numel, device="cuda")
    assert lib.mdt_train_encode_bwd(h, t2, g_ctx.data_ptr(), grads_buf.data_ptr(), None, None, None, None) == 5
    eng.tape_release(t2)
    # a handle without mdt_train_prepare
    cfg_c = model.inner_model._hip_config(SD, False)
    h2 = C.c_void_p()
    _lib.check(lib.mdt_create(C.byref(cfg_c), C.byref(h2)))
    try:
        assert lib.mdt_train_denoise_fwd(h2, c_.data_ptr(), x_.data_ptr(), s_.data_ptr(), B, None, out.data_ptr(), C.byref(tape), None) == 5
        assert lib.mdt_train_denoise_bwd(h2, 0, out.data_ptr(), None, None, None, None, None) == 5
    finally:
        lib.mdt_destroy(h2)


def test_sigma_token_models_refuse_d_sigma_in_the_library():
    import ctypes as C
    meta, cfg, state, goal, li = load_case("mdtv_no_ada")
    model = facade(meta, cfg)
    gstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    sg = li["sigma"].cuda()
    x = li["actions"].cuda()
    ctx = model.forward_context_only(gstate, None, goal.cuda(), sg).detach()
    eng = model._engine(allow_grad=True, state=gstate)
    out, tape = eng.train_denoise_fwd(ctx, x, sg)
    d_sigma = torch.empty_like(sg)
    st = eng.lib.mdt_train_denoise_bwd(eng.handle, tape, out.data_ptr(), None, None, None, d_sigma.data_ptr(), None)
    assert st == 2 and b"use_ada_conditioning" in eng.lib.mdt_last_error()  # MDT_ERR_UNSUPPORTED
    eng.tape_release(tape)


@pytest.mark.parametrize("name", ["mdtv_tiny", "proprio_default"])
def test_a_given_context_without_a_graph_and_without_a_state(name):
    """denoise_grad(None, x, None, sigma, context=ctx): the handle follows the context's layout (with / without the proprioceptive
    token), and under no_grad -- a taped decoder forward whose tape is handed back at once -- the value is forward's."""
    meta, cfg, state, goal, li = load_case(name)
    model = facade(meta, cfg)
    gstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    x = (li["actions"] + li["noise_train"] * li["sigma"][:, None, None]).cuda()
    g, sg = goal.cuda(), li["sigma"].cuda()
    with torch.no_grad():
        want = model(gstate, x, g, sg)
        ctx = model.inner_model.latent_encoder_emb.clone()
        got = model.denoise_grad(None, x, None, sg, context=ctx)
        assert not got.requires_grad
        assert_close(got.cpu(), want.cpu(), rtol=1e-3, atol=1e-4, what=name + " no_grad, given context")
        for _ in range(20):  # no tape stays behind
            model.denoise_grad(None, x, None, sg, context=ctx)
    taped = model.denoise_grad(None, x, None, sg, context=ctx)  # the parameters require grad: a node, on the same handle
    assert taped.requires_grad
    assert_close(taped.detach().cpu(), want.cpu(), rtol=1e-3, atol=1e-4, what=name + " taped, given context")
    assert torch.equal(taped.detach(), got)  # the same launches with and without a graph
    with pytest.raises(ValueError, match="context must be"):
        model.denoise_grad(None, x, None, sg, context=ctx[:, :-1].contiguous() if name == "mdtv_tiny" else ctx[:, :2].contiguous())


def test_denoise_backward_is_refused_between_the_stages_of_a_staged_loss_backward():
    """The chain's scratch carries a staged loss backward from stage to stage: a denoise backward in between is MDT_ERR_STATE (a
    host-side status, nothing enqueued), and runs once the staged backward has finished."""
    meta, cfg, state, goal, li = load_case("mdtv_tiny")
    model = facade(meta, cfg)
    st = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in state.items()}
    eng = model._engine(allow_grad=True, state=st)
    tok, tok2, gg, B, _, _ = model._train_inputs(eng, st, goal.cuda(), True)
    a, nz = eng._in(li["actions"].cuda(), (B, eng.Ta, eng.A)), eng._in(li["noise_train"].cuda(), (B, eng.Ta, eng.A))
    sg = eng._in(li["sigma"].cuda(), (B,))
    _, _, ctx, loss_tape = eng.train_loss_fwd(st, tok, tok2, gg, a, nz, sg, None)
    den, tape = eng.train_denoise_fwd(ctx, a, sg)
    buf = eng.train_loss_bwd_begin(torch.ones((), device="cuda"), None, tok, tok2, gg, (False, False, False))
    eng.train_loss_bwd_stage(loss_tape, 0, *buf)
    d_x = torch.empty_like(den)
    status = eng.lib.mdt_train_denoise_bwd(eng.handle, tape, den.data_ptr(), None, None, d_x.data_ptr(), None, None)
    assert status == 5 and b"staged loss backward" in eng.lib.mdt_last_error()
    for k in range(1, eng._n_stages):
        eng.train_loss_bwd_stage(loss_tape, k, *buf)
    _, _, d_x2, _ = eng.train_denoise_bwd(tape, den, B, (False, True, False), False)
    torch.cuda.synchronize()
    assert torch.isfinite(d_x2).all() and float(d_x2.abs().max()) > 0
    eng.tape_release(tape)
    eng.tape_release(loss_tape)
