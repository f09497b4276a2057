"""What the forward-only scorer costs beside log_likelihood on the GPU, in one process: ms per call on the shipped MDT-V (d = 384,
synthetic 'rich' weights) at B observations x K chunks,

  score   : gs.denoising_score(extra_args={"candidates": K}) -> mdt_denoising_score, S levels log-uniform in [0.001, 80], M draws,
            eager (one enqueue; the events bracket it and the wait for it)
  replay  : the same call captured once with torch.cuda.graph and replayed
  loglik  : gs.log_likelihood(extra_args={"candidates": K}) on the same chunks, sigma 0.001 .. 80, rtol = atol = 1e-4, one probe
            (the setup of tools/loglik_bench.py)

    python tools/score_bench.py [--calls 20] [--warmup 3] [--legs 1x8] [--levels 16] [--draws 2] [--seeds 5] [--out FILE]
The three forms alternate call by call inside one timed loop, each call between two device events; the figure is the median over
--calls rounds after --warmup untimed ones.  Then, for --seeds seeds (other chunks, other noise rows, other probes), Spearman's rank
correlation between the two scorers over each observation's K chunks.  With synthetic weights the network is no trained denoiser,
so that correlation says little about either scorer; it is printed as found.  Prints one line per leg and one JSON line."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spearman(a, b):
    ra, rb = a.argsort().argsort().double(), b.argsort().argsort().double()
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra * rb).sum() / (ra.norm() * rb.norm()).clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="1x8")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--draws", type=int, default=2)
    ap.add_argument("--seeds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 20, "the median of at least 20 calls"
    assert torch.cuda.is_available(), "score_bench measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    smin, smax, tol = 0.001, 80.0, 1e-4
    S, M = args.levels, args.draws
    levels = [smin] if S == 1 else [math.exp(math.log(smax) + (math.log(smin) - math.log(smax)) * i / (S - 1)) for i in range(S)]

    def inputs(B, K, seed):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        x = torch.from_numpy(synthetic.loss_inputs(B * K, cfg, seed)["actions"]).cuda()
        gen = torch.Generator().manual_seed(seed + 1)
        v = (torch.randint(0, 2, (1,) + tuple(x.shape), generator=gen) * 2 - 1).float().cuda()
        if M % 2 == 0:  # antithetic pairs, -n directly after each n, as denoising_score draws them
            half = torch.randn((S, M // 2) + tuple(x.shape[1:]), generator=gen)
            noise = torch.stack((half, -half), 2).reshape((S, M) + tuple(x.shape[1:])).cuda()
        else:
            noise = torch.randn((S, M) + tuple(x.shape[1:]), generator=gen).cuda()
        return {"state_images": t["state_images"], "modality": "lang"}, x, t["goal"], v, noise

    rows = []
    with torch.no_grad():
        for B, K in [tuple(int(v) for v in leg.split("x")) for leg in args.legs.split(",")]:
            state, x, goal, v, noise = inputs(B, K, 7)
            score = lambda: gs.denoising_score(model, state, x, goal, levels, extra_args={"candidates": K}, noise=noise)
            loglik = lambda: gs.log_likelihood(model, state, x, goal, smin, smax, extra_args={"candidates": K, "probes": v}, atol=tol,
                                               rtol=tol)
            loglik()  # first: it prepares the handle's training state, which the capture below must not precede
            eager = score()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured = score()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(captured, eager), "the replay must give the eager call's bits"
            forms = {"score": score, "replay": graph.replay, "loglik": loglik}
            ms = {k: [] for k in forms}
            fevals = None
            for i in range(args.warmup + args.calls):
                for k, fn in forms.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    r = fn()
                    e1.record()
                    e1.synchronize()
                    if k == "loglik":
                        fevals = r[1]["fevals"]
                    if i >= args.warmup:
                        ms[k].append(e0.elapsed_time(e1))
            med = {k: sorted(t)[len(t) // 2] for k, t in ms.items()}
            low = {k: min(t) for k, t in ms.items()}
            rho = []
            for seed in range(args.seeds):
                st, xs, g, vs, nz = inputs(B, K, 100 + 10 * seed)
                a = gs.denoising_score(model, st, xs, g, levels, extra_args={"candidates": K}, noise=nz).reshape(B, K).cpu()
                b = gs.log_likelihood(model, st, xs, g, smin, smax, extra_args={"candidates": K, "probes": vs}, atol=tol,
                                      rtol=tol)[0].reshape(B, K).cpu()
                rho.append(sum(spearman(a[i], b[i]) for i in range(B)) / B)
            rows.append(dict(B=B, K=K, S=S, M=M, decoder_rows=B * K * S * M, score_ms=round(med["score"], 4),
                             score_min_ms=round(low["score"], 4), replay_ms=round(med["replay"], 4), replay_min_ms=round(low["replay"], 4),
                             loglik_ms=round(med["loglik"], 3), loglik_min_ms=round(low["loglik"], 3), loglik_fevals=fevals,
                             spearman=[round(r, 3) for r in rho]))
            print(f"({B:3d}, {K:2d}) S = {S}, M = {M} ({B * K * S * M} decoder rows): score {med['score']:.4f} ms eager, "
                  f"{med['replay']:.4f} ms replayed; log_likelihood {med['loglik']:.3f} ms ({fevals} fevals); x{med['loglik'] / med['score']:.1f} "
                  f"eager, x{med['loglik'] / med['replay']:.1f} replayed; Spearman per seed {[round(r, 3) for r in rho]}", flush=True)
    line = json.dumps({"calls": args.calls, "warmup": args.warmup, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
