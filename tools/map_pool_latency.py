"""What the MAP pooling block costs per token count on the GPU, in one process.

  block : ms per host-synchronised call of the shipped head (MAPBlock(1, 384, 8, 384): one latent, 16 heads of 24, synthetic 'rich'
          weights) at every token count of --tokens and batch of --batch: the inference forward, and forward_train + backward
          under torch autograd with d(x).  Beside each, oracle/cla_oracle.map_block -- the reference's arithmetic restated in
          torch -- in float32 on the same GPU, the same two ways.  Device events around each call, 3 warm-up calls, the median of
          --iters calls.  16 tokens run the one-workgroup-per-sample attention kernels, 17 the (sample, head group) kernels.
  attn  : the two attention launches alone through the hooks of mdt_hip_debug.h, one-workgroup-per-sample family against
          head-group family, at N = 4 and 16 and every batch of --batch; us per launch from device events around --op-iters
          launches.  Informative: it tells whether the older pair still earns its keep.
  bytes : the head-group forward at N = 64, B = 1024: K | V read once (B N 2 D floats) plus out written, over the launch time, as
          a fraction of the 8.0 TB/s HBM3E peak.  The launches rotate over four K | V buffers (805 MB), more than the 256 MB
          Infinity Cache holds, so that the figure is HBM's.

    python tools/map_pool_latency.py [--tokens 4,16,17,34,64] [--batch 1,128,1024] [--iters 20] [--op-iters 50]
                                     [--time-limit 480] [--skip-block] [--skip-ops]

Prints one line per measurement and one JSON line with everything.  --time-limit: seconds after which the process ends itself."""
import argparse
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.long_chunk_latency import event_ms  # noqa: E402
from tools.long_context_latency import many  # noqa: E402

HBM_PEAK = 8.0e12   # bytes per second, HBM3E of the MI355X as specified
SHIPPED = dict(n_latents=1, embed_dim=384, n_heads=8, output_dim=384, mlp_ratio=4.0)


def block(args):
    from mdt_policy_amd import synthetic
    from mdt_policy_amd.models.networks.transformers.map_pool import MAPBlock
    from oracle import cla_oracle as CO
    m = MAPBlock(**SHIPPED)
    shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    P = {k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()}
    m.load_state_dict(P)
    m = m.cuda()
    PT = {k: v.cuda().requires_grad_() for k, v in P.items()}
    res = {}
    for N in args.tokens:
        for B in args.batch:
            x = torch.from_numpy(synthetic.normal("ctx", (B, N, SHIPPED["embed_dim"]), 6)).cuda()
            xg = x.clone().requires_grad_()
            cot = torch.from_numpy(synthetic.normal("cotangent", (B, SHIPPED["output_dim"]), 7)).cuda()

            def hip_fwd():
                with torch.no_grad():
                    m(x)

            def hip_step():
                m.zero_grad(set_to_none=True)
                xg.grad = None
                (m(xg) * cot).sum().backward()

            def torch_fwd():
                with torch.no_grad():
                    CO.map_block(PT, "", x, SHIPPED["n_heads"])

            def torch_step():
                for p in PT.values():
                    p.grad = None
                xg.grad = None
                (CO.map_block(PT, "", xg, SHIPPED["n_heads"]) * cot).sum().backward()
            row = {}
            for name, fn in (("hip_fwd", hip_fwd), ("hip_step", hip_step), ("torch_fwd", torch_fwd), ("torch_step", torch_step)):
                med, best = event_ms(fn, args.iters, 3)
                row[name + "_ms"], row[name + "_ms_min"] = round(med, 4), round(best, 4)
            res[f"n{N}_b{B}"] = row
            print(f"N {N:2d}  B {B:4d}  forward HIP {row['hip_fwd_ms']:7.3f} ms  torch {row['torch_fwd_ms']:7.3f} ms   "
                  f"forward + backward HIP {row['hip_step_ms']:7.3f} ms  torch {row['torch_step_ms']:7.3f} ms", flush=True)
    return res


def attn(args):
    from mdt_policy_amd import _lib
    lib = _lib.load()
    Q, D, H = 1, 384, 16
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1)
    res = {}

    def buffers(B, N, copies=1):
        q = torch.randn(Q, D, generator=g).cuda()
        kvs = [torch.randn(B * N, 2 * D, generator=g).cuda() for _ in range(copies)]
        out, probs = torch.empty(B * Q, D, device="cuda"), torch.empty(B * Q * H, N, device="cuda")
        do, dq, dkv = torch.randn(B * Q, D, generator=g).cuda(), torch.empty(B * Q, D, device="cuda"), torch.empty(B * N, 2 * D, device="cuda")
        return q, kvs, out, probs, do, dq, dkv

    for N in (4, 16):
        for B in args.batch:
            q, (kv,), out, probs, do, dq, dkv = buffers(B, N)
            row = {}
            for _ in range(2):   # old, new, old, new: the second pass is the one reported
                for fam, tag in ((0, "sample"), (1, "group")):
                    fwd = lambda: _lib.check(lib.mdt_op_map_attn_fwd(fam, q.data_ptr(), kv.data_ptr(), out.data_ptr(), probs.data_ptr(),
                                                                     B, Q, N, D, H, s))
                    bwd = lambda: _lib.check(lib.mdt_op_map_attn_bwd(fam, q.data_ptr(), kv.data_ptr(), probs.data_ptr(), do.data_ptr(),
                                                                     dq.data_ptr(), dkv.data_ptr(), B, Q, N, D, H, s))
                    row[tag + "_fwd_us"] = round(event_ms(many(fwd, args.op_iters), 5, 1)[0] * 1e3 / args.op_iters, 2)
                    row[tag + "_bwd_us"] = round(event_ms(many(bwd, args.op_iters), 5, 1)[0] * 1e3 / args.op_iters, 2)
            res[f"n{N}_b{B}"] = row
            print(f"attention alone N {N:2d} B {B:4d}: forward per-sample {row['sample_fwd_us']:8.2f} us  head-group {row['group_fwd_us']:8.2f} us   "
                  f"backward per-sample {row['sample_bwd_us']:8.2f} us  head-group {row['group_bwd_us']:8.2f} us", flush=True)

    B, N = 1024, 64
    q, kvs, out, probs, do, dq, dkv = buffers(B, N, copies=4)
    turn = [0]

    def fwd():
        kv = kvs[turn[0] % len(kvs)]
        turn[0] += 1
        _lib.check(lib.mdt_op_map_attn_fwd(1, q.data_ptr(), kv.data_ptr(), out.data_ptr(), None, B, Q, N, D, H, s))
    us = event_ms(many(fwd, args.op_iters), 5, 1)[0] * 1e3 / args.op_iters
    moved = 4 * (B * N * 2 * D + B * Q * D + Q * D)
    res["bytes_n64_b1024"] = dict(us=round(us, 2), bytes=moved, tb_per_s=round(moved / us / 1e6, 3), of_hbm_peak=round(moved / (us * 1e-6) / HBM_PEAK, 3))
    print(f"head-group forward N 64 B 1024: {us:.2f} us for {moved / 1e6:.1f} MB = {moved / us / 1e6:.2f} TB/s "
          f"= {100 * moved / (us * 1e-6) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="4,16,17,34,64")
    ap.add_argument("--batch", default="1,128,1024")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--time-limit", type=int, default=480)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-block", action="store_true")
    args = ap.parse_args()
    args.tokens = [int(v) for v in args.tokens.split(",")]
    args.batch = [int(v) for v in args.batch.split(",")]
    assert torch.cuda.is_available(), "map_pool_latency measures on the GPU; there is no CPU fallback"
    signal.alarm(args.time_limit)   # SIGALRM's default action ends the process
    res = {}
    if not args.skip_block:
        res["block"] = block(args)
    if not args.skip_ops:
        res["attn"] = attn(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
