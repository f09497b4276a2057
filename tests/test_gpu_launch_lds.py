"""mdt_launch_lds (csrc/mdt_launch.h) keeps one dynamic-LDS high-water mark per kernel instantiation and device and raises the
kernel's limit only when a launch asks for more.  The marks are process-global and the surrounding pytest process has usually
raised them already, so the check runs in ONE fresh child process: for every family whose LDS size follows the runtime shape
it launches first the smaller shape, then the larger, and compares both with a float64 torch reference at the tolerance of the
family's own test.  A launch that asks for more LDS than its limit allows returns an error status (a failed check, not a fault).

Run as a script (`--child`) this file is that child."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_lds_limit_follows_the_largest_launch_in_a_fresh_process():
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), "--child"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "launch_lds child ok" in r.stdout, r.stdout[-3000:]


def _child():
    sys.path.insert(0, ROOT)
    import torch

    from mdt_policy_amd import _lib as L
    from tests.helpers import assert_close

    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream

    # ---- row-tile GEMM at geometry 1 (k_gemm<2, 1, 4, plain, no residual>): the activation chunk is the whole K, 64 then 384 floats
    lib.mdt_op_set_gemm_geometry(1)
    for K in (64, 384):
        M = N = 64
        g = torch.Generator().manual_seed(K)
        A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
        Ad, Wd, bd = A.cuda(), W.cuda(), b.cuda()
        P = torch.zeros(N * K, device="cuda")
        L.check(lib.mdt_op_pack_weight(Wd.data_ptr(), N, K, P.data_ptr(), 0, N, s))
        out = torch.full((M, N), float("nan"), device="cuda")
        a = L.GemmArgs()
        a.A, a.lda, a.Wp, a.bias, a.out, a.ldo = Ad.data_ptr(), K, P.data_ptr(), bd.data_ptr(), out.data_ptr(), N
        a.M, a.N, a.K = M, N, K
        a.shift_off, a.scale_off, a.gate_off, a.rows_per_sample = -1, -1, -1, 1
        a.gin, a.gout, a.goff = 1, 1, 0
        L.check(lib.mdt_op_gemm(C.byref(a), s))
        want = Ad.double() @ Wd.double().T + bd.double()
        assert_close(out.cpu(), want.cpu(), rtol=1e-4, atol=1e-4, what=f"gemm geometry 1, K = {K}")   # test_gpu_ops.py: test_gemm_plain_bias
        print(f"gemm K={K} ok", flush=True)
    lib.mdt_op_set_gemm_geometry(0)

    def ref_attn(qkv, do, H, hd):
        B, T, D3 = qkv.shape
        D = D3 // 3
        q64 = qkv.double().requires_grad_()
        q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in q64.split(D, dim=-1))
        sc = q @ k.transpose(-1, -2) * hd ** -0.5
        ref = (sc.softmax(-1) @ v).transpose(1, 2).reshape(B, T, D)
        ref.backward(do.double())
        return ref.detach(), sc.logsumexp(-1).detach(), q64.grad

    def inputs(B, H, hd, T, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(B, T, 3 * H * hd, generator=g).cuda(), torch.randn(B, T, H * hd, generator=g).cuda()

    # ---- masked-image attention (test_mae.py: test_attention_mid_forward_and_backward).  Head width 24 at the shortest and the
    # longest T of that test; and head width 48, whose kernels (k_attn_mid_fwd<48> / _bwd<48>) are ONE instantiation for every T
    # and size their LDS by T rounded up to 16: 7 (that test's) then 64
    for B, H, hd, T in [(2, 2, 24, 1), (1, 3, 24, 113), (5, 8, 48, 7), (2, 2, 48, 64)]:
        D = H * hd
        qd, dod = inputs(B, H, hd, T, 161 + T)
        ref, _, dref = ref_attn(qd, dod, H, hd)
        out = torch.full((B, T, D), float("nan"), device="cuda")
        L.check(lib.mdt_op_attn_mid_fwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, B, H, hd, T, hd ** -0.5, s))
        assert_close(out.cpu(), ref.cpu(), what=f"attn_mid hd {hd} T {T} output")
        dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
        L.check(lib.mdt_op_attn_mid_bwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, dod.data_ptr(), D, dq.data_ptr(), 3 * D, B, H, hd, T,
                                        hd ** -0.5, s))
        assert_close(dq.cpu(), dref.cpu(), rtol=1e-3, atol=1e-4, what=f"attn_mid hd {hd} T {T} d_qkv")
        print(f"attn_mid hd={hd} T={T} ok", flush=True)

    # ---- long attention (test_mae_long.py: test_attention_long_forward_and_backward): its shortest and its longest T
    for B, H, hd, T in [(2, 2, 64, 1), (1, 2, 64, 4096)]:
        D = H * hd
        qd, dod = inputs(B, H, hd, T, 261 + T)
        ref, ref_lse, dref = ref_attn(qd, dod, H, hd)
        out = torch.full((B, T, D), float("nan"), device="cuda")
        lse = torch.full((B, H, T), float("nan"), device="cuda")
        L.check(lib.mdt_op_attn_long_fwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), B, H, hd, T, hd ** -0.5, s))
        assert_close(out.cpu(), ref.cpu(), what=f"attn_long T {T} output")
        assert_close(lse.cpu(), ref_lse.cpu(), what=f"attn_long T {T} log-sum-exp")
        dq = torch.full((B, T, 3 * D), float("nan"), device="cuda")
        scratch = torch.empty(lib.mdt_op_attn_long_bwd_scratch(B, H, T), device="cuda")
        L.check(lib.mdt_op_attn_long_bwd(qd.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), dod.data_ptr(), D, dq.data_ptr(), 3 * D,
                                         B, H, hd, T, hd ** -0.5, scratch.data_ptr(), s))
        assert_close(dq.cpu(), dref.cpu(), rtol=1e-3, atol=1e-4, what=f"attn_long T {T} d_qkv")
        print(f"attn_long T={T} ok", flush=True)
    torch.cuda.synchronize()
    print("launch_lds child ok", flush=True)


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
