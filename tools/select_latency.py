"""What the replan-and-select loop costs as one call beside the three calls it replaces, on the GPU, in one process: ms from "noise
in" to "chunk out" on the shipped MDT-V (d = 384, synthetic 'rich' weights) at B observations x K chunks, --steps DDIM steps, S
levels log-uniform in [0.001, 80], M antithetic draws,

  a  three calls, eager   : gs.sample_ddim(candidates=K) -> gs.denoising_score(candidates=K) -> gs.best_candidates, MDT_HIP_GRAPH=0
  b  three calls, replayed: the same sequence with both native calls replayed as graphs as they can be today -- sample_ddim through
                            the facade's own GraphedDDIM, mdt_denoising_score captured once with torch.cuda.graph on a static copy
                            of the chunks (one copy launch in front of its replay) -- and best_candidates eager
  c  one call, eager      : gs.sample_select, MDT_HIP_GRAPH=0
  d  one call, replayed   : gs.sample_select through its GraphedSelect

    python tools/select_latency.py [--calls 200] [--warmup 20] [--leg 1x8] [--steps 10] [--levels 16] [--draws 2] [--out FILE]
The four forms alternate call by call inside one timed loop; a call is timed on the host between two device synchronisations.  Per
form: the median, the quartiles and the minimum over --calls rounds after --warmup untimed ones.  The four give the same chunks,
scores and index, which is checked first.  Prints one line per form and one JSON line."""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--leg", default="1x8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--draws", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.calls >= 200, "the median of at least 200 calls per form"
    assert torch.cuda.is_available(), "select_latency measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    smin, smax = 0.001, 80.0
    B, K = (int(v) for v in args.leg.split("x"))
    S, M = args.levels, args.draws
    levels = [smin] if S == 1 else [math.exp(math.log(smax) + (math.log(smin) - math.log(smax)) * i / (S - 1)) for i in range(S)]
    sig = gs.get_sigmas_exponential(args.steps, smin, smax)
    t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
    state, goal = {"state_images": t["state_images"], "modality": "lang"}, t["goal"]
    x_T = smax * torch.from_numpy(synthetic.loss_inputs(B * K, cfg, 7)["actions"]).cuda()
    gen = torch.Generator().manual_seed(8)
    half = torch.randn((S, max(M // 2, 1)) + tuple(x_T.shape[1:]), generator=gen)
    noise = (torch.stack((half, -half), 2).reshape((S, M) + tuple(x_T.shape[1:])) if M % 2 == 0 else
             torch.randn((S, M) + tuple(x_T.shape[1:]), generator=gen)).cuda()
    extra = {"candidates": K}

    def mode(graph):
        gs._GRAPH_MODE, gs._GRAPH_SAMPLER = ("1", True) if graph else ("0", False)

    def three(graph):
        mode(graph)
        cands = gs.sample_ddim(model, state, x_T, goal, sig, extra_args=extra)
        score = gs.denoising_score(model, state, cands, goal, levels, extra_args=extra, noise=noise)
        chunk, index = gs.best_candidates(cands, score, K)
        return chunk, index, score, cands

    def one(graph):
        mode(graph)
        return gs.sample_select(model, state, x_T, goal, sig, levels, extra_args=extra, noise=noise)

    with torch.no_grad():
        want = three(False)   # eager first: it sizes the workspace for the capture below
        static = want[3].clone()
        torch.cuda.synchronize()
        sgraph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(sgraph):
            sscore = gs.denoising_score(model, state, static, goal, levels, extra_args=extra, noise=noise)

        def three_replayed():
            mode(True)
            cands = gs.sample_ddim(model, state, x_T, goal, sig, extra_args=extra)   # the facade's GraphedDDIM
            static.copy_(cands)
            sgraph.replay()
            chunk, index = gs.best_candidates(cands, sscore, K)
            return chunk, index, sscore, cands

        forms = {"a_three_eager": lambda: three(False), "b_three_replayed": three_replayed, "c_one_eager": lambda: one(False),
                 "d_one_replayed": lambda: one(True)}
        for k, fn in forms.items():
            got = fn()
            torch.cuda.synchronize()
            for what, a, b in zip(("chunk", "index", "scores", "chunks"), got, want):
                assert torch.equal(a, b), f"{k}: {what} differs from the eager three calls"
        ms = {k: [] for k in forms}
        for i in range(args.warmup + args.calls):
            for k, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
    rows = {}
    for k, v in ms.items():
        v = sorted(v)
        rows[k] = dict(median_ms=round(v[len(v) // 2], 4), p25_ms=round(v[len(v) // 4], 4), p75_ms=round(v[3 * len(v) // 4], 4),
                       min_ms=round(v[0], 4))
        print(f"{k:17s} median {rows[k]['median_ms']:.4f} ms  quartiles {rows[k]['p25_ms']:.4f} .. {rows[k]['p75_ms']:.4f}  "
              f"min {rows[k]['min_ms']:.4f}", flush=True)
    line = json.dumps({"B": B, "K": K, "steps": args.steps, "S": S, "M": M, "calls": args.calls, "warmup": args.warmup, "forms": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
