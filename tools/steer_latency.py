"""What the native steered call buys on the GPU, in one process: ms per host-synchronised 10-step steered sampler call (MDT-V d = 384,
synthetic 'rich' weights, the exponential schedule 80 .. 0.001, an overlap steer with 3 hard and 2 soft tokens, beta = 5) for K
action chunks per observation,

  host   : the host loop over GCDenoiser.forward(..., steer=) -- what gc_sampling.sample_<kind> runs with a callback: the
           observations encoded once per call, per evaluation a taped decoder forward, the error in torch, the
           input-gradient-only backward, the update in torch
  native : gs.sample_<kind>(extra_args={"steer": steer, "candidates": K}) -> mdt_sample_ddim_steer (ddim) or mdt_sample_steer (every
           other fixed-schedule kind: heun, dpmpp_2m, lms, ...), one enqueue

for every (B, K) of --legs.

    python tools/steer_latency.py [--kind ddim] [--calls 20] [--warmup 3] [--steps 10] [--legs 1x1,1x8,64x1] [--out FILE]
Every call sits between two device events and is waited for (what a controller waits for); the figure is the median over --calls
calls after --warmup untimed ones, the forms alternating per leg.  Each timed loop also sits between two mdt_op_clock_stamp
records: the shader clock the chip sustained over exactly those calls is printed beside the time.  Prints one line per leg, the
table as it stands in DESIGN.md, and one JSON line; --out writes the table and the JSON line there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", default="ddim", help="the gc_sampling function name without 'sample_' (fixed-schedule kinds)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--legs", default="1x1,1x8,64x1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 20, "the median of at least 20 calls"
    assert torch.cuda.is_available(), "steer_latency measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import _lib, configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.utils.action_steer import ActionSteer

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    sigmas = gs.get_sigmas_exponential(args.steps, 0.001, 80.0)
    legs = [tuple(int(v) for v in leg.split("x")) for leg in args.legs.split(",")]

    def inputs(B, K):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        prev = torch.from_numpy(synthetic.loss_inputs(B, cfg, 7)["actions"]).cuda()
        x = 80.0 * torch.from_numpy(synthetic.normal("steer_latency", (B * K,) + tuple(prev.shape[1:]), 8)).cuda()
        return {"state_images": t["state_images"], "modality": "lang"}, x, t["goal"], ActionSteer.overlap(prev, 2, 3, 2, plan_native=True)

    sample = getattr(gs, "sample_" + args.kind)

    def host(state, x, goal, steer, K):
        return sample(model, state, x, goal, sigmas, extra_args={"steer": steer, "candidates": K}, callback=lambda d: None)

    def native(state, x, goal, steer, K):
        return sample(model, state, x, goal, sigmas, extra_args={"steer": steer, "candidates": K})

    def mhz(stamps):
        """Median over the XCDs of the shader clock between the two records (bench.py sustained_mhz)."""
        st = stamps.cpu().view(2, 8, 2)
        v = sorted((int(st[1, x, 0] - st[0, x, 0]) / int(st[1, x, 1] - st[0, x, 1]) * 100.0 for x in range(8)
                    if int(st[0, x, 1]) and int(st[1, x, 1]) and int(st[1, x, 1] - st[0, x, 1]) > 0))
        return round(v[len(v) // 2]) if v else None

    def timed(fn, a):
        with torch.no_grad():
            for _ in range(args.warmup):
                out = fn(*a)
            stamps = torch.zeros(2, 16, dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            torch.cuda.synchronize()
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[0].data_ptr(), stream))
            ms = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*a)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[1].data_ptr(), stream))
            torch.cuda.synchronize()
        ms.sort()
        return ms[len(ms) // 2], ms[0], mhz(stamps), out

    rows = []
    for B, K in legs:
        a = inputs(B, K) + (K,)
        h_ms, h_min, h_clk, h_out = timed(host, a)
        n_ms, n_min, n_clk, n_out = timed(native, a)
        diff = float((h_out - n_out).abs().max())
        rows.append(dict(kind=args.kind, B=B, K=K, steps=args.steps, host_ms=round(h_ms, 3), host_min_ms=round(h_min, 3), host_mhz=h_clk,
                         native_ms=round(n_ms, 3), native_min_ms=round(n_min, 3), native_mhz=n_clk,
                         native_ms_per_step=round(n_ms / args.steps, 3), speedup=round(h_ms / n_ms, 2), max_diff=round(diff, 6)))
        print(f"({B:3d}, {K:2d}) host {h_ms:8.3f} ms ({h_clk} MHz)   native {n_ms:8.3f} ms ({n_clk} MHz, {n_ms / args.steps:.3f} ms / step)"
              f"   x{h_ms / n_ms:.2f}   max |host - native| {diff:.2e}", flush=True)
    table = ["| B | K | host loop ms | native ms | native ms / step | speed-up |", "|---|---|---|---|---|---|"]
    table += [f"| {r['B']} | {r['K']} | {r['host_ms']:.2f} | {r['native_ms']:.2f} | {r['native_ms_per_step']:.3f} | {r['speedup']:.2f}x |"
              for r in rows]
    line = json.dumps({"kind": args.kind, "calls": args.calls, "warmup": args.warmup, "rows": rows})
    print("\n".join(table))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(table) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
