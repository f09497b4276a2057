"""Every case of RESAMPLER_ENVELOPE and MAP_ENVELOPE (tests/envelope_configs.py: the edges of what mdt_resampler_* and
mdt_map_pool_* accept) on the MI355X (pytest -m gpu): inference across the batch thresholds, a training step's gradients, two
live tapes, bit-reproducibility, the LDS-budget refusals and graph capture above 64 KiB of LDS -- each against float64
through the oracles (oracle/perceiver_oracle.py, oracle/cla_oracle.py), which tests/test_module_envelope.py pins to the
reference at the same shapes.  Gates: tests/helpers.assert_close's defaults for outputs, 2e-3 of a gradient's largest value for
gradients (test_perceiver.py, test_cla.py, test_gpu_config_envelope.py)."""
import pytest
import torch

from mdt_policy_amd import synthetic
from oracle import cla_oracle as CO
from oracle import perceiver_oracle as PO
from tests import envelope_configs as E
from tests.helpers import (assert_close, check_grad_summaries, envelope_params, map_envelope_fixture,
                           resampler_envelope_fixture)

pytestmark = pytest.mark.gpu

R_NAMES, M_NAMES = sorted(E.RESAMPLER_ENVELOPE), sorted(E.MAP_ENVELOPE)
R_SEED, M_SEED = 181, 184  # the weight seeds of the g18 fixtures: one cached module serves the oracle and the golden checks
_MODELS = {}


def _module(cls, kwargs, seed):
    """(module on cuda:0 in eval mode, its float32 state dict) with 'rich' synthetic weights; cases that share constructor
    kwargs share the module, so one handle sees its workspace grow and shrink across their shapes."""
    key = (cls.__name__, tuple(sorted(kwargs.items())))
    if key not in _MODELS:
        m = cls(**kwargs)
        P = envelope_params([(k, tuple(v.shape)) for k, v in m.state_dict().items()], seed)
        m.load_state_dict(P, strict=True)
        _MODELS[key] = (m.cuda().eval(), P)
    return _MODELS[key]


def resampler_of(name):
    from mdt_policy_amd.models.networks.transformers.perceiver_resampler import PerceiverResampler
    return _module(PerceiverResampler, E.RESAMPLER_ENVELOPE[name]["kwargs"], R_SEED)


def map_of(name):
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    return _module(MAPBlock, E.MAP_ENVELOPE[name]["kwargs"], M_SEED)


def media(name, B, seed, mask_kind="case"):
    """(media tokens (B, T, n, dim), mask (B, T) bool or None) on the host: distinct per sample and frame."""
    c = E.RESAMPLER_ENVELOPE[name]
    x = torch.from_numpy(synthetic.normal("media", (B, c["T"], c["n"], c["kwargs"]["dim"]), seed))
    m = E.resampler_mask(c["mask"] if mask_kind == "case" else mask_kind, B, c["T"])
    return x, None if m is None else torch.tensor(m, dtype=torch.bool)


def tokens(name, B, seed):
    c = E.MAP_ENVELOPE[name]
    return torch.from_numpy(synthetic.normal("ctx", (B, c["N"], c["kwargs"]["embed_dim"]), seed))


def dev(t):
    return None if t is None else t.cuda()


def f64(P, grad=False):
    return {k: (v.double().requires_grad_() if grad else v.double()) for k, v in P.items()}


def r_oracle(name, P, x, mask):
    return PO.perceiver_resampler(P, x, E.RESAMPLER_ENVELOPE[name]["kwargs"]["heads"], mask)


def m_oracle(name, P, x):
    return CO.map_block(P, "", x, E.MAP_ENVELOPE[name]["kwargs"]["n_heads"])


def check_grads(module, P64, what, exact_zero_rows=()):
    """Every parameter gradient against float64 autograd, each to 2e-3 of its own largest value; rows of the parameters named
    in exact_zero_rows whose reference gradient is identically zero must be exactly zero."""
    n = 0
    for k, p in module.named_parameters():
        ref = P64[k].grad
        assert p.grad is not None and ref is not None, k
        got = p.grad.cpu()
        assert_close(got, ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-7, what=f"{what} {k}")
        if k in exact_zero_rows:
            dead = (ref.reshape(ref.shape[0], -1) == 0).all(dim=1)
            assert bool((got.reshape(got.shape[0], -1)[dead] == 0).all()), f"{what} {k}: rows {dead.nonzero().flatten().tolist()}"
            exact_zero_rows[k].append(int(dead.sum()))
        n += 1
    return n


def check_dx(got, ref, what):
    assert_close(got.cpu(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-9, what=what)


def lds_refusal():
    from mdt_policy_amd._lib import MDTHipError
    return pytest.raises(MDTHipError, match="LDS budget")


# ---------------------------------------------------------------------------------------------------------------- resampler
def r_forward_checked(name, B, seed, P64):
    """One inference call against the float64 oracle (full tensors); returns (inputs, output)."""
    model, _ = resampler_of(name)
    x, mask = media(name, B, seed)
    want = r_oracle(name, P64, x.double(), mask)
    with torch.no_grad():
        got = model(dev(x), dev(mask))
    assert_close(got.cpu(), want, what=f"{name} B = {B}")
    return x, mask, got


@pytest.mark.parametrize("name", R_NAMES)
def test_resampler_inference_across_the_batch_thresholds(name):
    """mdt_resampler_forward against the float64 oracle at every batch of the case (B = 1, a mid batch, and for the small
    widths a batch with >= 8192 media rows and >= 192 latent rows); a second identical call is bit-equal; the first and the last
    sample run alone reproduce their rows -- at the parity gate, not bit for bit: one row and thousands take different GEMM
    tilings, two float32 summation orders that are each held to that gate against float64.  A case over the inference budget
    must be refused, and the module must still be right afterwards."""
    c = E.RESAMPLER_ENVELOPE[name]
    model, P = resampler_of(name)
    P64 = f64(P)
    if not c["infer"]:
        x, mask = media(name, 1, 11)
        with torch.no_grad(), lds_refusal():
            model(dev(x), dev(mask))
        r_forward_checked("r_wide_k257", 2, 12, P64)  # same constructor kwargs, same handle
        return
    for B in c["batches"]:
        x, mask, got = r_forward_checked(name, B, 20 + B, P64)
        with torch.no_grad():
            assert torch.equal(model(dev(x), dev(mask)), got), f"{name} B = {B}: second call differs"
            for i in sorted({0, B - 1}) if B > 1 else ():
                one = model(dev(x[i:i + 1]), None if mask is None else dev(mask[i:i + 1]))
                assert_close(one.cpu(), got[i:i + 1].cpu(), what=f"{name} sample {i} of {B} alone")


def r_train_step(name, B, seed, mask_kind="case"):
    """Taped forward + backward with a random cotangent on the HIP module and in float64 through the oracle."""
    model, P = resampler_of(name)
    x, mask = media(name, B, seed, mask_kind)
    model.zero_grad(set_to_none=True)
    xg = dev(x).requires_grad_()
    out = model(xg, dev(mask))
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(out.shape), seed + 1))
    (out * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    P64 = f64(P, grad=True)
    x64 = x.double().requires_grad_()
    o64 = r_oracle(name, P64, x64, mask)
    (o64 * cot.double()).sum().backward()
    return model, out.detach(), xg.grad, P64, o64.detach(), x64.grad, mask


@pytest.mark.parametrize("name", R_NAMES)
def test_resampler_training_step_gradients(name):
    """mdt_resampler_forward_train + mdt_resampler_backward: the taped output, every parameter gradient and d(x_f) against
    float64 autograd through the oracle; time_pos_emb rows of frames that are masked in every sample (or not passed at all)
    get an exactly zero gradient.  A case over the training budget must be refused by the TAPED FORWARD, and inference on the
    same module must still work where the case allows it."""
    c = E.RESAMPLER_ENVELOPE[name]
    if not c["train"]:
        model, P = resampler_of(name)
        x, mask = media(name, c["train_b"], 31)
        with lds_refusal():
            model(dev(x).requires_grad_(), dev(mask))
        if c["infer"]:
            r_forward_checked(name, c["train_b"], 31, f64(P))
        else:
            r_forward_checked("r_wide_k257", 1, 32, f64(P))
        return
    B = c["train_b"]
    model, out, dx, P64, o64, dx64, mask = r_train_step(name, B, 33)
    assert_close(out.cpu(), o64, what=f"{name} taped forward")
    zero = {"time_pos_emb": []}
    assert check_grads(model, P64, name, zero) == len(P64)
    check_dx(dx, dx64, f"{name} d_x_f")
    T, E_ = c["T"], c["kwargs"]["num_time_embeds"]
    dead = E_ - T + (0 if mask is None else int((~mask).all(dim=0).sum()))
    assert zero["time_pos_emb"] == [dead], (zero, dead)


@pytest.mark.parametrize("name", sorted(E.RESAMPLER_GOLDEN))
def test_resampler_matches_the_reference_golden(name):
    """Output and gradients against what the REFERENCE module gave for the same weights and inputs (g18 fixtures)."""
    meta, fx, P, x, mask, cot = resampler_envelope_fixture(name)
    model, PM = resampler_of(name)
    assert all(torch.equal(P[k], PM[k]) for k in P)
    with torch.no_grad():
        assert_close(model(dev(x), dev(mask)).cpu(), fx["out"], what=f"{name} vs reference golden")
    model.zero_grad(set_to_none=True)
    xg = dev(x).requires_grad_()
    out = model(xg, dev(mask))
    (out * cot.cuda()).sum().backward()
    assert_close(out.detach().cpu(), fx["out"], what=f"{name} taped vs reference golden")
    check_grad_summaries({k: p.grad for k, p in model.named_parameters()}, meta["grads"], name + " (HIP)")
    dx = xg.grad.cpu()
    assert_close(dx[:, :, :4, :], fx["d_x_head"], rtol=2e-3, atol=2e-3 * float(abs(fx["d_x_head"]).max()), what=name + " d_x_f")
    assert abs(float(dx.double().norm()) - meta["d_x_summary"][0]) <= 2e-3 * meta["d_x_summary"][0]


def test_resampler_two_live_tapes_accumulate_into_one_backward():
    """Two taped forwards of different batch sizes and different masks, then ONE backward: parameter gradients (time_pos_emb
    among them) are the sum over both tapes.  Frame 2 is masked in every sample of both tapes: its row stays exactly zero."""
    name = "r_inner_lt_dim"
    model, P = resampler_of(name)
    xa, ma = media(name, 4, 41)
    xb, _ = media(name, 2, 42)
    mb = torch.tensor([[1, 1, 0, 0, 1], [0, 1, 0, 1, 1]], dtype=torch.bool)
    model.zero_grad(set_to_none=True)
    ga, gb = dev(xa).requires_grad_(), dev(xb).requires_grad_()
    oa, ob = model(ga, dev(ma)), model(gb, dev(mb))
    ca = torch.from_numpy(synthetic.normal("cotangent", tuple(oa.shape), 43))
    ((oa * ca.cuda()).sum() + (ob ** 2).sum()).backward()
    P64 = f64(P, grad=True)
    a64, b64 = xa.double().requires_grad_(), xb.double().requires_grad_()
    ra, rb = r_oracle(name, P64, a64, ma), r_oracle(name, P64, b64, mb)
    ((ra * ca.double()).sum() + (rb ** 2).sum()).backward()
    zero = {"time_pos_emb": []}
    check_grads(model, P64, "two tapes", zero)
    assert zero["time_pos_emb"] == [2]  # frame 2 and the sixth, unused embedding
    check_dx(ga.grad, a64.grad, "d_x_f first tape")
    check_dx(gb.grad, b64.grad, "d_x_f second tape")


def test_resampler_backward_is_bit_reproducible_above_64_kib_of_lds():
    name = "r_lds_k1000"
    runs = []
    for _ in range(2):
        model, _, dx, *_ = r_train_step(name, 2, 51)
        runs.append([dx.clone()] + [p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_resampler_inference_above_64_kib_of_lds_replays_as_a_graph():
    """mdt_resampler_forward with a 83 KiB attention workgroup (the raised dynamic-LDS attribute) captured by torch.cuda.graph
    and replayed twice with new inputs, each replay against the float64 oracle."""
    name = "r_lds_k1000"
    model, P = resampler_of(name)
    P64 = f64(P)
    x0, m0 = media(name, 2, 61)
    xs, ms = dev(x0), dev(m0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(2):
            model(xs, ms)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = model(xs, ms)
    for seed in (62, 63):
        x, _ = media(name, 2, seed)
        m = torch.tensor([[1, 0, 1], [1, 1, 0]] if seed == 62 else [[0, 1, 1], [0, 0, 0]], dtype=torch.bool)
        xs.copy_(x)
        ms.copy_(m)
        graph.replay()
        torch.cuda.synchronize()
        assert_close(out.cpu(), r_oracle(name, P64, x.double(), m), what=f"replay with seed {seed}")


def test_time_embedding_gradient_beyond_65535_frames():
    """B * T = 66000 frames: the per-frame partial sums of the time_pos_emb gradient run one workgroup per frame, more than a
    grid's y dimension holds."""
    name = "r_min_2keys"
    model, out, dx, P64, o64, dx64, _ = r_train_step(name, 66000, 71)
    assert_close(out.cpu(), o64, what="taped forward")
    check_grads(model, P64, "66000 frames")
    check_dx(dx, dx64, "d_x_f")


# ---------------------------------------------------------------------------------------------------------------- MAP block
def m_forward_checked(name, B, seed, P64):
    model, _ = map_of(name)
    x = tokens(name, B, seed)
    want = m_oracle(name, P64, x.double())
    with torch.no_grad():
        got = model(x.cuda())
    assert_close(got.cpu(), want, what=f"{name} B = {B}")
    return x, got


@pytest.mark.parametrize("name", M_NAMES)
def test_map_block_inference_across_the_batch_thresholds(name):
    """mdt_map_pool_forward against the float64 oracle at every batch of the case (up to >= 8192 token rows for the narrow
    blocks, beyond 300 samples for all but the two LDS cases); second call bit-equal; first and last sample alone reproduce
    their rows.  The case over the 64 KiB budget must be refused."""
    c = E.MAP_ENVELOPE[name]
    model, P = map_of(name)
    P64 = f64(P)
    if not c["infer"]:
        with torch.no_grad(), lds_refusal():
            model(tokens(name, 1, 11).cuda())
        # fewer tokens fit: 4 * (16 * 512 + 2 * 2 * 512 + 16 * 16 * 2) = 43008 bytes
        x = tokens(name, 3, 12)[:, :2].contiguous()
        with torch.no_grad():
            assert_close(model(x.cuda()).cpu(), m_oracle(name, P64, x.double()), what=f"{name} with 2 tokens")
        return
    for B in c["batches"]:
        x, got = m_forward_checked(name, B, 20 + B, P64)
        assert tuple(got.shape) == (B, c["kwargs"]["n_latents"], c["kwargs"]["output_dim"])
        with torch.no_grad():
            assert torch.equal(model(x.cuda()), got), f"{name} B = {B}: second call differs"
            for i in sorted({0, B - 1}) if B > 1 else ():
                assert_close(model(x[i:i + 1].cuda()).cpu(), got[i:i + 1].cpu(), what=f"{name} sample {i} of {B} alone")


def m_train_step(name, B, seed):
    model, P = map_of(name)
    x = tokens(name, B, seed)
    model.zero_grad(set_to_none=True)
    xg = x.cuda().requires_grad_()
    out = model(xg)
    cot = torch.from_numpy(synthetic.normal("cotangent", tuple(out.shape), seed + 1))
    (out * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    P64 = f64(P, grad=True)
    x64 = x.double().requires_grad_()
    o64 = m_oracle(name, P64, x64)
    (o64 * cot.double()).sum().backward()
    return model, out.detach(), xg.grad, P64, o64.detach(), x64.grad


@pytest.mark.parametrize("name", M_NAMES)
def test_map_block_training_step_gradients(name):
    """mdt_map_pool_forward_train + mdt_map_pool_backward: taped output, every parameter gradient and d(x) against float64
    autograd through the oracle.  The two cases over the training budget must be refused by the taped forward; inference on
    the same module still works where the case allows it."""
    c = E.MAP_ENVELOPE[name]
    if not c["train"]:
        model, P = map_of(name)
        with lds_refusal():
            model(tokens(name, c["train_b"], 31).cuda().requires_grad_())
        if c["infer"]:
            m_forward_checked(name, c["train_b"], 31, f64(P))
        return
    model, out, dx, P64, o64, dx64 = m_train_step(name, c["train_b"], 33)
    assert_close(out.cpu(), o64, what=f"{name} taped forward")
    assert check_grads(model, P64, name) == len(P64)
    check_dx(dx, dx64, f"{name} d_x")


@pytest.mark.parametrize("name", sorted(E.MAP_GOLDEN))
def test_map_block_matches_the_reference_golden(name):
    meta, fx, P, x, cot = map_envelope_fixture(name)
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


def test_map_block_two_live_tapes_accumulate_into_one_backward():
    """16 latents: two taped forwards of different batch sizes, then ONE backward; every gradient is the sum over both."""
    name = "m_q16_e96_d48"
    model, P = map_of(name)
    xa, xb = tokens(name, 5, 41), tokens(name, 9, 42)
    model.zero_grad(set_to_none=True)
    ga, gb = xa.cuda().requires_grad_(), xb.cuda().requires_grad_()
    oa, ob = model(ga), model(gb)
    ca = torch.from_numpy(synthetic.normal("cotangent", tuple(oa.shape), 43))
    ((oa * ca.cuda()).sum() + (ob ** 2).sum()).backward()
    P64 = f64(P, grad=True)
    a64, b64 = xa.double().requires_grad_(), xb.double().requires_grad_()
    ra, rb = m_oracle(name, P64, a64), m_oracle(name, P64, b64)
    ((ra * ca.double()).sum() + (rb ** 2).sum()).backward()
    check_grads(model, P64, "two tapes")
    check_dx(ga.grad, a64.grad, "d_x first tape")
    check_dx(gb.grad, b64.grad, "d_x second tape")


def test_map_block_backward_is_bit_reproducible_at_its_largest_workgroup():
    """The block's budget is 64 KiB, so no case is above it: this is the trainable case closest to it (62976 bytes)."""
    name = "m_q3_e640_h32"
    kw, N = E.MAP_ENVELOPE[name]["kwargs"], E.MAP_ENVELOPE[name]["N"]
    assert E.map_lds_bytes(kw["n_latents"], kw["output_dim"], kw["n_heads"], N, True) == 62976
    runs = []
    for _ in range(2):
        model, _, dx, *_ = m_train_step(name, 6, 51)
        runs.append([dx.clone()] + [p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
