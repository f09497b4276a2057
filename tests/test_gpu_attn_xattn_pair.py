"""k_attn_xattn with its output projection on fp16 pair splits (include/mdt_hip_ops.h: mdt_op_attn_xattn_pair; DESIGN.md section
5a (j)): accuracy against float64 and the fp32 launch, fp16's range, guard bands, refusals, and the model-level calls that take it."""
import ctypes as C
import math
import types

import pytest
import torch
import torch.nn.functional as F

from tests.guarded import NAN, bits, canary, same_bits
from tests.helpers import assert_close
from tests.test_gpu_f16_pair import check_gate, dev, model_case, pack, pack_pair, stream
from tests.test_gpu_ops import pack_t, ref_attn
from tests.test_gpu_ops_bounds import Lay

pytestmark = pytest.mark.gpu

H, HD = 8, 48
D = H * HD
IMAGE_BYTES = 4 * D * D + D


@pytest.fixture(scope="module")
def lib():
    from mdt_policy_amd import _lib
    return _lib


def host_case(T, Te, gated, bias, B, seed=0):
    """Inputs built as test_one_sample_per_workgroup_through_attention_projection_and_cross_attention builds them."""
    g = torch.Generator().manual_seed(17 * T + Te + B + 1000 * seed)
    c = types.SimpleNamespace(T=T, Te=Te, gated=gated, bias=bias, B=B)
    c.qkv = torch.randn(B * T, 3 * D, generator=g)
    c.W, c.b = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.1
    c.gate, c.y0 = torch.randn(B, 6 * D, generator=g), torch.randn(B * T, D, generator=g) * 2
    c.kv = torch.randn(B * Te, 2 * D, generator=g)
    c.Wq, c.bq = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.3
    c.Wo, c.bo = torch.randn(D, D, generator=g) / math.sqrt(D), torch.randn(D, generator=g) * 0.3
    c.lw, c.lb = torch.randn(D, generator=g) * 0.2 + 1, torch.randn(D, generator=g) * 0.2
    return c


def reference(c):
    """float64: the two sublayers"""
    B, T, Te = c.B, c.T, c.Te
    q3 = c.qkv.view(B, T, 3 * D)
    att = ref_attn(q3[..., :D], q3[..., D:2 * D], q3[..., 2 * D:], H, True).double().reshape(B * T, D)
    upd = att @ c.W.double().T + c.b.double()
    if c.gated:
        upd = c.gate[:, 2 * D:3 * D].double().repeat_interleave(T, 0) * upd
    y1 = (c.y0.double() + upd).view(B, T, D)
    kd = c.kv.double()
    K, V = kd[:, :D].view(B, Te, D), kd[:, D:].view(B, Te, D)
    q = F.layer_norm(y1, (D,), c.lw.double(), c.lb.double(), 1e-5) @ c.Wq.double().T + c.bq.double()
    qh, kh, vh = (x.view(B, -1, H, HD).transpose(1, 2) for x in (q, K, V))
    sc = qh @ kh.transpose(-2, -1) / math.sqrt(HD)
    sc = sc.masked_fill(~torch.ones(T, Te, dtype=torch.bool).tril(), float("-inf"))
    o = (sc.softmax(-1) @ vh).transpose(1, 2).reshape(B, T, D) @ c.Wo.double().T + (c.bo.double() if c.bias else 0)
    return (y1 + o).reshape(B * T, D)


class Operands:
    """Device operands of one case: the folded cross-attention images are made once and shared by the launches of a test."""

    def __init__(self, lib, c):
        self.lib, self.c = lib, c
        t = self.t = {k: dev(getattr(c, k)) for k in ("kv", "bq", "bo", "lw", "lb", "b", "gate")}
        t["WqT_p"], t["Wo_p"] = pack_t(lib, c.Wq), pack(lib, c.Wo)
        self.Wp, self.image = pack(lib, c.W), pack_pair(lib, c.W)
        NP = 4 * H
        self.U, self.Wf, self.cc = (torch.empty(n, device="cuda") for n in (c.B * NP * D, c.B * NP * D, c.B * NP))
        f = lib.XFoldArgs()
        f.kv, f.ldkv, f.WqT_p, f.bq, f.Wo_p = t["kv"].data_ptr(), 2 * D, t["WqT_p"].data_ptr(), t["bq"].data_ptr(), t["Wo_p"].data_ptr()
        f.U, f.Wf, f.c, f.B, f.H, f.hd, f.D, f.Te = self.U.data_ptr(), self.Wf.data_ptr(), self.cc.data_ptr(), c.B, H, HD, D, c.Te
        lib.check(lib.load().mdt_op_xattn_fold(C.byref(f), stream()))

    def args(self, out_ptr, image_ptr=None, fp32_image=True):
        c, t, lib = self.c, self.t, self.lib
        a = lib.GemmArgs()
        a.A, a.lda, a.bias, a.out, a.ldo, a.M, a.N, a.K = None, D, t["b"].data_ptr(), out_ptr, D, c.B * c.T, D, D
        a.Wp = self.Wp.data_ptr() if fp32_image else None
        a.Wp_pair = image_ptr
        a.shift_off = a.scale_off = -1
        a.gate_off = 2 * D if c.gated else -1
        a.mod, a.mod_stride = (t["gate"].data_ptr(), 6 * D) if c.gated else (None, 0)
        a.residual, a.rows_per_sample, a.gin, a.gout = 1, c.T, 1, 1
        x = lib.XApplyArgs()
        x.y, x.ln_w, x.ln_b, x.U, x.Wf, x.c = out_ptr, t["lw"].data_ptr(), t["lb"].data_ptr(), self.U.data_ptr(), self.Wf.data_ptr(), self.cc.data_ptr()
        x.bo = t["bo"].data_ptr() if c.bias else None
        x.B, x.H, x.D, x.Te, x.Ta = c.B, H, D, c.Te, c.T
        return a, x

    def run(self, pair, qkv=None, image=None):
        """One launch on a fresh copy of y0 -> the rows on the host.  pair: mdt_op_attn_xattn_pair with Wp NULL (it must not be
        read); otherwise mdt_op_attn_xattn with the pair image set as well (it must not be taken)."""
        c, L = self.c, self.lib.load()
        out, qd = dev(c.y0).clone(), dev(c.qkv if qkv is None else qkv)
        image = self.image if image is None else image
        a, x = self.args(out.data_ptr(), image.data_ptr(), fp32_image=not pair)
        op = L.mdt_op_attn_xattn_pair if pair else L.mdt_op_attn_xattn
        self.lib.check(op(C.byref(a), qd.data_ptr(), 3 * D, C.byref(x), HD, c.T, stream()))
        torch.cuda.synchronize()
        return out.cpu()


def err(got, want):
    return (got.double() - want).abs().max().item()


# (T, Te, gated, bias, B): the default shape; TKC = 16 with no padding rows; padding rows; a single real row
CASES = [(10, 4, True, False, 3), (16, 3, True, True, 2), (7, 2, False, True, 5), (1, 4, True, True, 4)]


@pytest.mark.parametrize("T,Te,gated,bias,B", CASES)
def test_pair_projection_keeps_fp32_accuracy(lib, T, Te, gated, bias, B):
    """mdt_op_attn_xattn_pair against float64 within 1.5x the fp32 launch's error + 1e-6 on the same inputs; finite; not the fp32
    launch's bits; the same bits on a second launch.  mdt_op_attn_xattn keeps launching the fp32 form with Wp_pair set."""
    c = host_case(T, Te, gated, bias, B)
    want = reference(c)
    ops = Operands(lib, c)
    fp32, got, again = ops.run(False), ops.run(True), ops.run(True)
    assert torch.isfinite(got).all()
    check_gate(err(got, want), err(fp32, want), f"attn_xattn pair T {T} Te {Te} gated {gated} bias {bias} B {B}")
    assert not torch.equal(got, fp32), "the pair form did not run"
    assert same_bits(got, again), "two launches on the same inputs differ"
    assert_close(fp32, want.float(), rtol=2e-4, atol=2e-4, what="the fp32 launch")


def test_pair_projection_over_the_fp32_range(lib):
    """The value columns of sample 1 scaled by 1e4 and of sample 2 by 1e-4 (the per-row scale absorbs both), a c_proj weight with
    one 16-row tile scaled by 1e-9 and another by 1e5: finite and inside the gate.  One Inf in a value row of sample 3 makes
    that sample's outputs non-finite; every other sample keeps the bits of the clean run."""
    T, B = 10, 5
    c = host_case(T, 4, True, True, B, seed=1)
    c.qkv[1 * T:2 * T, 2 * D:] *= 1e4
    c.qkv[2 * T:3 * T, 2 * D:] *= 1e-4
    c.W[16:32] *= 1e-9
    c.W[48:64] *= 1e5
    want = reference(c)
    ops = Operands(lib, c)
    fp32, got = ops.run(False), ops.run(True)
    assert torch.isfinite(got).all(), "a finite input gave a non-finite output"
    check_gate(err(got, want), err(fp32, want), "attn_xattn pair over the range")
    for s in range(B):   # (printed only: the largest sample's error decides the gate above)
        rows = slice(s * T, (s + 1) * T)
        print(f"  sample {s}: pair {err(got[rows], want[rows]):.3e}  fp32 {err(fp32[rows], want[rows]):.3e}")
    s = 3
    qi = c.qkv.clone()
    qi[s * T, 2 * D + 5] = float("inf")
    bad = ops.run(True, qkv=qi)
    rows = torch.arange(B * T) // T == s
    assert not torch.isfinite(bad[rows]).any(), "an Inf in a value row of sample 3 must make its outputs non-finite"
    assert same_bits(bad[~rows], got[~rows]), "the other samples changed"


@pytest.mark.parametrize("T,B", [(10, 3), (16, 1), (7, 2)])
def test_pair_projection_stays_inside_its_buffers(lib, T, B):
    """Guard bands around every operand (tests/guarded.py): nothing is written outside out[B T, D], no input changes, and no guard
    value reaches the result; then the image as the last bytes of its allocation with the guard pattern in front of it -- the
    same bits, so the op reads the image only inside its 4 D D + D bytes."""
    c = host_case(T, 3, True, True, B, seed=2)
    want = reference(c)
    ops = Operands(lib, c)
    plain = ops.run(True)
    L = Lay(True)
    what = f"attn_xattn pair T {T}, B {B}"
    g = {k: L.inp(k, getattr(c, k)) for k in ("b", "lw", "lb", "bo")}
    gate, qd = L.inp("gate", c.gate), L.inp("qkv", c.qkv)
    U, Wf, cc = (L.inp(k, v.cpu().reshape(B, -1)) for k, v in (("U", ops.U), ("Wf", ops.Wf), ("c", ops.cc)))
    image = L.image("Wp_pair", ops.image.cpu())
    out = L.out("out", B * T, D, fill=c.y0)
    a = lib.GemmArgs()
    a.A, a.lda, a.Wp, a.Wp_pair, a.bias, a.out, a.ldo, a.M, a.N, a.K = None, D, None, image.ptr, g["b"].ptr, out.ptr, D, B * T, D, D
    a.shift_off = a.scale_off = -1
    a.gate_off, a.mod, a.mod_stride = 2 * D, gate.ptr, gate.ld
    a.residual, a.rows_per_sample, a.gin, a.gout = 1, T, 1, 1
    x = lib.XApplyArgs(y=out.ptr, ln_w=g["lw"].ptr, ln_b=g["lb"].ptr, U=U.ptr, Wf=Wf.ptr, c=cc.ptr, bo=g["bo"].ptr, B=B, H=H, D=D,
                       Te=c.Te, Ta=T)
    lib.check(lib.load().mdt_op_attn_xattn_pair(C.byref(a), qd.ptr, 3 * D, C.byref(x), HD, T, stream()))
    L.check(what)
    out.check(what + ": out", written=True)
    assert same_bits(out.host(), plain), f"{what}: differs from the dense call's bits"
    check_gate(err(plain, want), err(ops.run(False), want), what)

    front = 512 - IMAGE_BYTES % 512            # the allocation ends with the image's last byte; 16-byte aligned start
    assert front % 16 == 0
    buf = torch.empty(front + IMAGE_BYTES, dtype=torch.uint8, device="cuda")
    buf[:front] = torch.full((front // 4,), NAN).view(torch.uint8).cuda()
    buf[front:] = ops.image
    assert same_bits(ops.run(True, image=buf[front:]), plain), f"{what}: the image at the end of its allocation gives other bits"


def test_pair_projection_refusals(lib):
    """null Wp_pair and a misaligned image: MDT_ERR_INVALID_ARG; hd != 48 and x.y != proj.out: MDT_ERR_UNSUPPORTED; the output
    stays untouched."""
    T, B = 10, 2
    c = host_case(T, 4, True, True, B, seed=3)
    ops = Operands(lib, c)
    L = lib.load()
    out, other, qd = canary(B * T, D).cuda(), canary(B * T, D).cuda(), dev(c.qkv)
    start = bits(out)
    shifted = torch.zeros(IMAGE_BYTES + 16, dtype=torch.uint8, device="cuda")
    shifted[4:4 + IMAGE_BYTES] = ops.image

    def call(image_ptr, hd=HD, y=None):
        a, x = ops.args(out.data_ptr(), image_ptr)
        if y is not None:
            x.y = y
        status = L.mdt_op_attn_xattn_pair(C.byref(a), qd.data_ptr(), 3 * D, C.byref(x), hd, T, stream())
        torch.cuda.synchronize()
        assert torch.equal(bits(out), start) and torch.equal(bits(other), start), "a refused call wrote into an output"
        return status

    assert call(None) == 1, "null Wp_pair"
    assert call(shifted.data_ptr() + 4) == 1, "misaligned image"
    assert call(ops.image.data_ptr(), hd=64) == 2, "head dimension 64"
    assert call(ops.image.data_ptr(), y=other.data_ptr()) == 2, "x.y != proj.out"


# ------------------------------------------------------------------------------------------------
# model level: g3_b256_lang.npz at B = 80 (800 decoder rows, just above the 768-row gate), 3 DDIM steps
# ------------------------------------------------------------------------------------------------
FIXTURE = "g3_b256_lang.npz"
PROJ = "decoder.blocks.{}.attn.c_proj.weight"


def ddim(model, state, noise, goal, sig, B=None):
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    if B is not None:
        state = {k: (v[:B] if torch.is_tensor(v) else v) for k, v in state.items()}
        noise, goal = noise[:B], goal[:B]
    with torch.no_grad():
        return gs.sample_ddim(model, state, noise * 80.0, goal, sig).clone()


def test_model_level_calls_take_the_pair_projection(lib):
    """sample_ddim at B = 80: oracle parity (rtol 1e-3, atol 1e-4), within 1e-4 / 1e-4 of the mdt_op_set_mlp_split(0) call, the same
    bits call after call.  At B = 70 (700 rows, below the gate) the call equals the mdt_op_set_mlp_split(0) call bit for bit."""
    meta, model, state, goal, noise, sig, want = model_case(FIXTURE)
    L = lib.load()
    L.mdt_op_set_mlp_split(1)
    try:
        got, again = ddim(model, state, noise, goal, sig), ddim(model, state, noise, goal, sig)
        low = ddim(model, state, noise, goal, sig, B=70)
        L.mdt_op_set_mlp_split(0)
        fp32 = ddim(model, state, noise, goal, sig)
        low_fp32 = ddim(model, state, noise, goal, sig, B=70)
    finally:
        L.mdt_op_set_mlp_split(-1)
    assert_close(got.cpu(), want, what="pair form against the oracle")
    assert torch.equal(got, again), "two calls differ"
    print(f"largest |pair - fp32| = {(got - fp32).abs().max().item():.3e}")
    assert_close(got.cpu(), fp32.cpu(), rtol=1e-4, atol=1e-4, what="pair against fp32 launches")
    assert torch.equal(low, low_fp32), "700 rows: below the 768-row gate the fp32 launches must run"


def test_a_changed_c_proj_weight_leaves_no_stale_image(lib):
    """A model with a training state (two SGD steps) gets other decoder attention c_proj weights loaded; its next sample has the bits
    of a freshly loaded model's, and not those from before the load."""
    from mdt_policy_amd import synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from tests.helpers import cfg_of, inputs_of
    meta, model, state, goal, noise, sig, _ = model_case(FIXTURE)
    cfg = cfg_of(meta)
    L = lib.load()
    L.mdt_op_set_mlp_split(1)
    try:
        trained = GCDenoiser(cfg, sigma_data=0.5).cuda()
        trained.load_state_dict(model.state_dict())
        trained.train()
        opt = torch.optim.SGD(trained.parameters(), lr=0.05)
        tstate, tgoal, _ = inputs_of(dict(meta, B=16, input_seed=1))
        tstate = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in tstate.items()}
        li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(16, cfg, 2).items()}
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, _ = trained.loss(tstate, li["actions"], tgoal.cuda(), li["noise_train"], li["sigma"])
            loss.backward()
            opt.step()
        trained.eval()
        before = ddim(trained, state, noise, goal, sig)
        sd = {k: v.detach().clone() for k, v in trained.state_dict().items()}
        g = torch.Generator().manual_seed(11)
        changed = [k for k in sd if k.endswith(".attn.c_proj.weight") and ".decoder.blocks." in k]
        assert changed, "no decoder c_proj weight in the state dict"
        for k in changed:
            sd[k] = sd[k] * 1.25 + 0.02 * torch.randn(sd[k].shape, generator=g).to(sd[k].device)
        trained.load_state_dict(sd)
        after = ddim(trained, state, noise, goal, sig)
        fresh = GCDenoiser(cfg, sigma_data=0.5).cuda().eval()
        fresh.load_state_dict(sd)
        ref = ddim(fresh, state, noise, goal, sig)
    finally:
        L.mdt_op_set_mlp_split(-1)
    assert not torch.equal(after, before), "the changed c_proj weights did not change the sampler's output"
    assert torch.equal(after, ref), "sampling after the load read a stale pair image"


def test_candidates_call_takes_the_pair_projection():
    """16 observations x 5 candidates = 80 chunks (800 rows): the ctx_div instantiation of the pair form, against the replicated
    call as tests/test_gpu_candidates.py compares them, and not the bits of the fp32 launches."""
    from mdt_policy_amd import _lib
    from tests.test_gpu_candidates import case, cuda, gs, model_of, sched
    B, K = 16, 5
    model, _ = model_of("mdtv_default")
    state, goal, x, wide, wide_goal = case("mdtv_default", B, K)
    L = _lib.load()
    L.mdt_op_set_mlp_split(1)
    try:
        with torch.no_grad():
            got = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sched(), extra_args={"candidates": K}).clone()
            plain = gs.sample_ddim(model, cuda(wide), x.cuda(), wide_goal.cuda(), sched()).clone()
            L.mdt_op_set_mlp_split(0)
            fp32 = gs.sample_ddim(model, cuda(state), x.cuda(), goal.cuda(), sched(), extra_args={"candidates": K}).clone()
    finally:
        L.mdt_op_set_mlp_split(-1)
    assert tuple(got.shape)[0] == B * K
    assert_close(got.cpu(), plain.cpu(), what="(16, 5) against the replicated native call")
    assert not torch.equal(got, fp32), "the pair launches did not run"
    assert_close(got.cpu(), fp32.cpu(), rtol=1e-4, atol=1e-4, what="(16, 5) pair against fp32 launches")
