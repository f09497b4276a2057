"""What the native log-likelihood call buys on the GPU, in one process: ms per call of log_likelihood (MDT-V d = 384, synthetic
'rich' weights, sigma 0.001 .. 80 at the default tolerances rtol = atol = 1e-4) for K action chunks per observation and P probes,

  host   : what log_likelihood ran before mdt_log_likelihood -- gs._dopri5 on the host over a flow made of
           GCDenoiser.denoise_vjp (encoder + decoder forward + input-gradient-only backward per evaluation and probe), on
           observations expanded with repeat_interleave
  native : gs.log_likelihood(extra_args={"candidates": K, "probes": v}) -> mdt_log_likelihood

for every (B, K, P) of --legs, and the denoiser evaluations (fevals) each took.

    python tools/loglik_bench.py [--calls 20] [--warmup 3] [--legs 1x1x1,1x8x1,1x8x4,64x1x1] [--out FILE]
Every call sits between two device events (the call is blocking: the events bracket what the user waits for); the figure is the
median over --calls calls after --warmup untimed ones, the forms alternating per leg.  Each timed loop also sits between two
mdt_op_clock_stamp records: the shader clock the chip sustained over exactly those calls is printed beside the time.  Prints one
line per leg and form, the table as it stands in DESIGN.md, and one JSON line; --out writes the table and the JSON line there."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="1x1x1,1x8x1,1x8x4,64x1x1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 20, "the median of at least 20 calls"
    assert torch.cuda.is_available(), "loglik_bench measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import _lib, configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    smin, smax, tol = 0.001, 80.0, 1e-4
    legs = [tuple(int(v) for v in leg.split("x")) for leg in args.legs.split(",")]

    def inputs(B, K, P):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        x = torch.from_numpy(synthetic.loss_inputs(B * K, cfg, 7)["actions"]).cuda()
        gen = torch.Generator().manual_seed(8)
        v = (torch.randint(0, 2, (P,) + tuple(x.shape), generator=gen) * 2 - 1).float().cuda()
        return {"state_images": t["state_images"], "modality": "lang"}, x, t["goal"], v

    def host(state, x, goal, v, K):
        """The parent's path: the Dormand-Prince loop in Python, every evaluation a full mdt_denoise_vjp per probe."""
        st = {"state_images": state["state_images"].repeat_interleave(K, 0), "modality": "lang"}
        g = goal.repeat_interleave(K, 0)
        n = [0]

        def flow(sigma, y):
            n[0] += 1
            sg = torch.full((y[0].shape[0],), sigma, device=y[0].device, dtype=y[0].dtype)
            div = 0
            for p in range(v.shape[0]):
                den, jtv = model.denoise_vjp(st, y[0], g, sg, v[p])
                div = div + (v[p] * ((v[p] - jtv) / sigma)).flatten(1).sum(1)
            return gs.to_d(y[0], sigma, den), div / v.shape[0]

        latent, delta = gs._dopri5(flow, (x, x.new_zeros([x.shape[0]])), smin, smax, tol, tol)
        return torch.distributions.Normal(0, smax).log_prob(latent).flatten(1).sum(1) + delta, n[0]

    def native(state, x, goal, v, K):
        ll, info = gs.log_likelihood(model, state, x, goal, smin, smax, extra_args={"candidates": K, "probes": v}, atol=tol, rtol=tol)
        return ll, info["fevals"]

    def mhz(stamps):
        """Median over the XCDs of the shader clock between the two records (bench.py sustained_mhz)."""
        st = stamps.cpu().view(2, 8, 2)
        v = sorted((int(st[1, x, 0] - st[0, x, 0]) / int(st[1, x, 1] - st[0, x, 1]) * 100.0 for x in range(8)
                    if int(st[0, x, 1]) and int(st[1, x, 1]) and int(st[1, x, 1] - st[0, x, 1]) > 0))
        return round(v[len(v) // 2]) if v else None

    def timed(fn, a):
        with torch.no_grad():
            for _ in range(args.warmup):
                ll, fe = fn(*a)
            stamps = torch.zeros(2, 16, dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            torch.cuda.synchronize()
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[0].data_ptr(), stream))
            ms = []
            for _ in range(args.calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ll, fe = fn(*a)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[1].data_ptr(), stream))
            torch.cuda.synchronize()
        ms.sort()
        return ms[len(ms) // 2], ms[0], fe, mhz(stamps), ll

    rows = []
    for B, K, P in legs:
        a = inputs(B, K, P) + (K,)
        h_ms, h_min, h_fe, h_clk, h_ll = timed(host, a)
        n_ms, n_min, n_fe, n_clk, n_ll = timed(native, a)
        diff = float((h_ll - n_ll).abs().max())
        rows.append(dict(B=B, K=K, P=P, host_ms=round(h_ms, 3), host_min_ms=round(h_min, 3), host_fevals=h_fe, host_mhz=h_clk,
                         native_ms=round(n_ms, 3), native_min_ms=round(n_min, 3), native_fevals=n_fe, native_mhz=n_clk,
                         speedup=round(h_ms / n_ms, 2), max_ll_diff=round(diff, 5)))
        print(f"({B:3d}, {K:2d}, {P}) host {h_ms:9.3f} ms ({h_fe} fevals, {h_clk} MHz)   native {n_ms:9.3f} ms ({n_fe} fevals, {n_clk} MHz)"
              f"   x{h_ms / n_ms:.2f}   max |ll host - native| {diff:.2e}", flush=True)
    table = ["| B | K | P | host loop ms | fevals | native ms | fevals | speed-up |", "|---|---|---|---|---|---|---|---|"]
    table += [f"| {r['B']} | {r['K']} | {r['P']} | {r['host_ms']:.2f} | {r['host_fevals']} | {r['native_ms']:.2f} | {r['native_fevals']} | "
              f"{r['speedup']:.2f}x |" for r in rows]
    line = json.dumps({"calls": args.calls, "warmup": args.warmup, "rows": rows})
    print("\n".join(table))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(table) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
