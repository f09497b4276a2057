"""What a longer action chunk costs on the GPU, in one process.

  calls : ms per host-synchronised call of 10-step sample_ddim (exponential schedule 0.001 .. 80; shipped MDT-V d = 384, synthetic
          'rich' weights) for every action_seq_len of --ta and batch of --batch: device events around each call, 3 warm-up calls
          (the third identical rollout-sized call captures its graph), the median of --iters calls; ms per call and ns per step
          and decoder row (B * Ta rows); the step from 16 to 17 rows -- where the fused one-sample launches and the collapsed
          cross-attention hand over to the explicit q GEMM -> attention -> c_proj sequence -- is named.
  ops   : the three attention ops alone at B = 256, H = 8, head dim 48, T = 64 (mdt_op_attention, mdt_op_attn_fwd_train with p = 0.3,
          mdt_op_attn_bwd; causal), us per launch from device events around --op-iters launches, the FLOPs counted from the shapes
          (forward 4 B H T^2 hd for q k^T and P V, backward 10 B H T^2 hd for P, dP, dQ, dK, dV; the causal half is not discounted)
          and torch's fp32 scaled_dot_product_attention (forward, and forward + backward minus forward) on the same shape beside them.

    python tools/long_chunk_latency.py [--ta 10,16,17,32,64] [--batch 1,64,256] [--iters 20] [--op-iters 50] [--skip-ops]

Prints one line per measurement and one JSON line with everything."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, iters, warmup):
    """Median and minimum milliseconds of fn() between two device events, each call synchronised on its own."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def calls(args):
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    res = {}
    for ta in args.ta:
        cfg = configs.mdtv_default(action_seq_len=ta)
        model = GCDenoiser(cfg, sigma_data=0.5)
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
        model = model.cuda().eval()
        for B in args.batch:
            t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
            state, x, goal = {"state_images": t["state_images"], "modality": "lang"}, t["noise"] * 80.0, t["goal"]

            def one():
                with torch.no_grad():
                    gs.sample_ddim(model, state, x, goal, sig)
            med, best = event_ms(one, args.iters, 3)
            per_row = med * 1e6 / (10 * B * ta)
            res[f"ta{ta}_b{B}"] = dict(ms_per_call=round(med, 4), ms_min=round(best, 4), ns_per_step_and_row=round(per_row, 1))
            print(f"Ta {ta:2d}  B {B:3d}  {med:8.3f} ms per call (min {best:.3f})  {per_row:9.1f} ns per step and decoder row", flush=True)
        del model
    for B in args.batch:
        a, b = res.get(f"ta16_b{B}"), res.get(f"ta17_b{B}")
        if a and b:
            print(f"step from Ta = 16 to Ta = 17 at B = {B}: {a['ms_per_call']:.3f} -> {b['ms_per_call']:.3f} ms per call "
                  f"({b['ms_per_call'] / a['ms_per_call']:.2f} x for 1.06 x the rows)")
            res[f"step_16_to_17_b{B}"] = round(b["ms_per_call"] / a["ms_per_call"], 3)
    return res


def ops(args):
    from mdt_policy_amd import _lib
    lib = _lib.load()
    B, H, hd, T = 256, 8, 48, 64
    D = H * hd
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B * T, 3 * D, generator=g).cuda()
    do, out = torch.randn(B * T, D, generator=g).cuda(), torch.empty(B * T, D, device="cuda")
    dqkv = torch.empty(B * T, 3 * D, device="cuda")
    tab = torch.zeros(64 * 16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, col=0: t.data_ptr() + 4 * col
    a = _lib.AttnArgs(q=p(qkv), ldq=3 * D, k=p(qkv, D), v=p(qkv, 2 * D), ldkv=3 * D, out=p(out), ldo=D, B=B, H=H, hd=hd, Tq=T, Tk=T, causal=1, rope=0)
    kw = dict(B=B, H=H, hd=hd, Tq=T, Tk=T, causal=1, p=0.3, site=7, seed=12345, rope=0, rope_cos=p(tab), rope_sin=p(tab))
    t = _lib.AttnTrainArgs(q=p(qkv), ldq=3 * D, k=p(qkv, D), v=p(qkv, 2 * D), ldkv=3 * D, out=p(out), ldo=D, **kw)
    gb = _lib.AttnBwdArgs(q=p(qkv), ldq=3 * D, k=p(qkv, D), v=p(qkv, 2 * D), ldkv=3 * D, d_out=p(do), ld_do=D, dq=p(dqkv), ld_dq=3 * D,
                          dk=p(dqkv, D), dv=p(dqkv, 2 * D), ld_dkv=3 * D, accumulate_kv=0, **kw)
    fwd_flops, bwd_flops = 4 * B * H * T * T * hd, 10 * B * H * T * T * hd
    n = args.op_iters

    def many(fn):
        def run():
            for _ in range(n):
                fn()
        return run
    res = {}
    for name, fn, flops in (("mdt_op_attention", lambda: _lib.check(lib.mdt_op_attention(C.byref(a), s)), fwd_flops),
                            ("mdt_op_attn_fwd_train", lambda: _lib.check(lib.mdt_op_attn_fwd_train(C.byref(t), s)), fwd_flops),
                            ("mdt_op_attn_bwd", lambda: _lib.check(lib.mdt_op_attn_bwd(C.byref(gb), s)), bwd_flops)):
        med, _ = event_ms(many(fn), 5, 1)
        us = med * 1e3 / n
        res[name] = dict(us=round(us, 2), flops=flops, tflops=round(flops / us * 1e-6, 2))
        print(f"{name:24s} {us:8.2f} us per launch  {flops / 1e9:6.2f} GFLOP  {flops / us * 1e-6:6.2f} TFLOP/s", flush=True)
    # torch's fp32 SDPA on the same shape
    q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(B, T, H, hd).transpose(1, 2).contiguous() for i in range(3))
    sd = lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    with torch.no_grad():
        med, _ = event_ms(many(sd), 5, 1)
    res["sdpa_fwd_us"] = round(med * 1e3 / n, 2)
    qg, kg, vg = (x.clone().requires_grad_() for x in (q, k, v))
    dog = do.reshape(B, T, H, hd).transpose(1, 2).contiguous()

    def fb():
        o = torch.nn.functional.scaled_dot_product_attention(qg, kg, vg, is_causal=True)
        torch.autograd.grad(o, (qg, kg, vg), dog)
    med2, _ = event_ms(many(fb), 5, 1)
    res["sdpa_fwd_bwd_us"] = round(med2 * 1e3 / n, 2)
    res["sdpa_bwd_us"] = round((med2 - med) * 1e3 / n, 2)
    print(f"torch fp32 SDPA, same shape: forward {res['sdpa_fwd_us']:.2f} us, forward + backward {res['sdpa_fwd_bwd_us']:.2f} us "
          f"(backward alone ~ {res['sdpa_bwd_us']:.2f} us)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ta", default="10,16,17,32,64")
    ap.add_argument("--batch", default="1,64,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    args.ta = [int(v) for v in args.ta.split(",")]
    args.batch = [int(v) for v in args.batch.split(",")]
    assert torch.cuda.is_available(), "long_chunk_latency measures on the GPU; there is no CPU fallback"
    res = {}
    if not args.skip_calls:
        res["calls"] = calls(args)
    if not args.skip_ops:
        res["ops"] = ops(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
