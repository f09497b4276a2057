"""The long self-attention op (mdt_op_attn_long_fwd / _bwd) alone, against torch's scaled_dot_product_attention in fp32 on
the same GPU: time per call from events over repeated launches, and the fraction of the fp32 matrix peak from algorithmic
FLOPs (4 B H T^2 hd forward, 8 B H T^2 hd backward).  Run under `rocprofv3 --kernel-trace --stats` for per-kernel rows.
usage: python tools/mae_long_attn.py [B [H [hd [T ...]]]]   (defaults 1024 8 24 132 396)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from mdt_policy_amd import _lib as L

PEAK = 157.3e12   # fp32 MFMA, dense


def timed(fn, it=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(it):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / it * 1e-3


def main():
    args = [int(x) for x in sys.argv[1:]]
    B, H, hd = (args[:3] + [1024, 8, 24][len(args[:3]):])
    Ts = args[3:] or [132, 396]
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    for T in Ts:
        D = H * hd
        sc = hd ** -0.5
        qkv = torch.randn(B, T, 3 * D, device="cuda")
        do = torch.randn(B, T, D, device="cuda")
        out = torch.empty(B, T, D, device="cuda")
        lse = torch.empty(B, H, T, device="cuda")
        dq = torch.empty(B, T, 3 * D, device="cuda")
        scratch = torch.empty(lib.mdt_op_attn_long_bwd_scratch(B, H, T), device="cuda")
        fwd = lambda: L.check(lib.mdt_op_attn_long_fwd(qkv.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), B, H, hd, T, sc, s))
        bwd = lambda: L.check(lib.mdt_op_attn_long_bwd(qkv.data_ptr(), 3 * D, out.data_ptr(), D, lse.data_ptr(), do.data_ptr(), D,
                                                      dq.data_ptr(), 3 * D, B, H, hd, T, sc, scratch.data_ptr(), s))
        tf, tb = timed(fwd), timed(bwd)
        q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2).contiguous().requires_grad_() for t in qkv.split(D, dim=-1))
        o = F.scaled_dot_product_attention(q, k, v)
        g = do.reshape(B, T, H, hd).transpose(1, 2).contiguous()
        sf = timed(lambda: F.scaled_dot_product_attention(q, k, v))
        sb = timed(lambda: torch.autograd.grad(o, (q, k, v), g, retain_graph=True))
        ff, fb = 4.0 * B * H * T * T * hd, 8.0 * B * H * T * T * hd
        print(f"B={B} H={H} hd={hd} T={T}: long fwd {tf*1e6:8.1f} us ({ff/tf/PEAK:.3f} of peak)  bwd {tb*1e6:8.1f} us "
              f"({fb/tb/PEAK:.3f})  |  sdpa fp32 fwd {sf*1e6:8.1f} us ({ff/sf/PEAK:.3f})  bwd {sb*1e6:8.1f} us ({fb/sb/PEAK:.3f})",
              flush=True)


if __name__ == "__main__":
    main()
