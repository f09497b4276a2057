"""The two attention launches of the MAP pooling block through the hooks of include/mdt_hip_debug.h (mdt_op_map_attn_fwd / _bwd),
on the MI355X (pytest -m gpu): the (sample, head group) kernels of 17 .. 64 tokens held to their buffers
(tests/guarded.py: guard bands around every operand, canary-filled outputs, everything outside the call compared bit for bit), a NaN
twin that shows which sample reads what, and the same kernels at 1, 7 and 16 tokens beside the one-workgroup-per-sample pair at the
same inputs.

Reference: the attention core in float64 under torch autograd (k scaled by hd^-1/2, softmax, P v).  Gates: tests/helpers.assert_close's
defaults for the forward's outputs, 2e-3 of a tensor's largest entry for every gradient -- those of tests/test_gpu_module_envelope.py."""
import pytest
import torch

from mdt_policy_amd import _lib, synthetic
from tests.guarded import GuardedSet, bits, canary
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

NEW, OLD = 1, 0
# (Q, N, D, H): the shipped head at 34 tokens; the widest head at the token limit; 64 heads of 8; head dim 3 at the first token count
# of the family; head dim 1 at an odd one
SHAPES = [(1, 34, 384, 16), (16, 64, 512, 2), (16, 64, 512, 64), (3, 17, 48, 16), (5, 63, 16, 16)]
_REF = {}


def operands(Q, N, D, H, B, seed):
    q = torch.from_numpy(synthetic.normal("map_q", (Q, D), seed))
    kv = torch.from_numpy(synthetic.normal("map_kv", (B, N, 2 * D), seed + 1))
    d_out = torch.from_numpy(synthetic.normal("map_dout", (B, Q, D), seed + 2))
    return q, kv, d_out


def reference(Q, N, D, H, B, seed):
    """float64: out (B, Q, D), probs (B, Q, H, N), dq_part (B, Q, D), d_kv (B, N, 2 D); computed once per shape and shared."""
    key = (Q, N, D, H, B, seed)
    if key not in _REF:
        q, kv, d_out = operands(Q, N, D, H, B, seed)
        hd = D // H
        qb = q.double().expand(B, Q, D).clone().requires_grad_()      # one copy per sample: its gradient is dq_part
        kv64 = kv.double().requires_grad_()
        k, v = kv64[..., :D].reshape(B, N, H, hd), kv64[..., D:].reshape(B, N, H, hd)
        s = torch.einsum("bqhc,bnhc->bqhn", qb.reshape(B, Q, H, hd), k * hd ** -0.5)
        p = s.softmax(dim=-1)
        out = torch.einsum("bqhn,bnhc->bqhc", p, v).reshape(B, Q, D)
        (out * d_out.double()).sum().backward()
        _REF[key] = tuple(t.detach() for t in (out, p, qb.grad, kv64.grad))
    return _REF[key]


def launch(family, Q, N, D, H, B, seed, kv=None, spare=1):
    """Forward, then backward on the forward's probs, every operand between guard bands; the outputs hold `spare` samples more
    than the call writes, canary-filled.  Returns the GuardedSets and the outputs (host)."""
    lib = _lib.load()
    q, kv0, d_out = operands(Q, N, D, H, B, seed)
    kv = kv0 if kv is None else kv
    stream = torch.cuda.current_stream().cuda_stream
    f = GuardedSet()
    gq, gkv = f.inp("q", q), f.inp("kv", kv.reshape(B * N, 2 * D))
    out = f.out("out", (B + spare) * Q, D, fill=canary((B + spare) * Q, D))
    probs = f.out("probs", (B + spare) * Q * H, N, fill=canary((B + spare) * Q * H, N))
    _lib.check(lib.mdt_op_map_attn_fwd(family, gq.ptr, gkv.ptr, out.ptr, probs.ptr, B, Q, N, D, H, stream))
    torch.cuda.synchronize()
    f.check(f"forward family {family} {(Q, N, D, H)}")
    b = GuardedSet()
    bq, bkv = b.inp("q", q), b.inp("kv", kv.reshape(B * N, 2 * D))
    bp = b.inp("probs", probs.host()[:B * Q * H])
    bdo = b.inp("d_out", d_out.reshape(B * Q, D))
    dq = b.out("dq_part", (B + spare) * Q, D, fill=canary((B + spare) * Q, D))
    dkv = b.out("d_kv", (B + spare) * N, 2 * D, fill=canary((B + spare) * N, 2 * D))
    _lib.check(lib.mdt_op_map_attn_bwd(family, bq.ptr, bkv.ptr, bp.ptr, bdo.ptr, dq.ptr, dkv.ptr, B, Q, N, D, H, stream))
    torch.cuda.synchronize()
    b.check(f"backward family {family} {(Q, N, D, H)}")
    got = dict(out=out.host().reshape(B + spare, Q, D), probs=probs.host().reshape(B + spare, Q, H, N),
               dq_part=dq.host().reshape(B + spare, Q, D), d_kv=dkv.host().reshape(B + spare, N, 2 * D))
    for name, t in got.items():   # the samples behind the batch: not one bit of the canary changed
        assert torch.equal(bits(t[B:]), bits(canary(*t[B:].shape))), f"family {family} {(Q, N, D, H)}: {name} written behind the batch"
    return {k: t[:B] for k, t in got.items()}


def check(got, Q, N, D, H, B, seed, what):
    out, p, dq, dkv = reference(Q, N, D, H, B, seed)
    assert_close(got["out"], out, what=f"{what} out")
    assert_close(got["probs"], p, what=f"{what} probs")
    assert abs(float(got["probs"].double().sum(dim=-1).sub(1).abs().max())) <= 1e-5
    for name, ref in (("dq_part", dq), ("d_kv", dkv)):
        assert_close(got[name], ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()) + 1e-9, what=f"{what} {name}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "q%d_n%d_d%d_h%d" % s)
def test_both_launches_stay_inside_their_buffers(shape):
    """Forward and backward of the head-group family at B = 3: inputs unchanged bit for bit, guard bands intact, every element
    the call owns written (no canary NaN left: d_kv is not zero-filled first), the sample behind the batch untouched; results
    against float64."""
    Q, N, D, H = shape
    got = launch(NEW, Q, N, D, H, 3, 101)
    for name, t in got.items():
        assert not bool(t.isnan().any()), f"{shape}: {name} keeps canary NaNs"
    check(got, Q, N, D, H, 3, 101, f"{shape}")


@pytest.mark.parametrize("shape", [(1, 34, 384, 16), (16, 64, 512, 2), (3, 17, 48, 16)], ids=lambda s: "q%d_n%d_d%d_h%d" % s)
def test_nans_in_one_samples_keys_and_values_stay_in_that_sample(shape):
    """A twin run with every K | V entry of sample 1 replaced by NaN: samples 0 and 2 keep their bits in all four outputs, and
    sample 1 shows the NaNs in out, dq_part and d_kv (a kernel that read a neighbour's rows, or skipped its own, would not)."""
    Q, N, D, H = shape
    clean = launch(NEW, Q, N, D, H, 3, 111)
    _, kv, _ = operands(Q, N, D, H, 3, 111)
    kv = kv.clone()
    kv[1] = float("nan")
    twin = launch(NEW, Q, N, D, H, 3, 111, kv=kv)
    for name in clean:
        for b in (0, 2):
            assert torch.equal(bits(clean[name][b]), bits(twin[name][b])), f"{shape}: {name} of sample {b} changed"
        assert bool(twin[name][1].isnan().all()), f"{shape}: {name} of sample 1 does not show the NaNs"


@pytest.mark.parametrize("N", [1, 7, 16])
@pytest.mark.parametrize("QDH", [(1, 384, 16), (16, 48, 2), (4, 48, 16), (3, 16, 16)], ids=lambda s: "q%d_d%d_h%d" % s)
def test_both_families_at_equal_shapes_up_to_16_tokens(N, QDH):
    """The head-group kernels are reachable at 1 .. 16 tokens through the hooks: there they and the one-workgroup-per-sample pair
    are held to the same float64 gate at the same inputs (not to each other's bits: a softmax row is summed by 16 lanes in one
    family and by one thread in the other)."""
    Q, D, H = QDH
    for family in (OLD, NEW):
        got = launch(family, Q, N, D, H, 5, 121)
        check(got, Q, N, D, H, 5, 121, f"family {family} {(Q, N, D, H)}")
