"""What sharing the context buys on the GPU, in one process: ms per host-synchronised call of 10-step sample_ddim (MDT-V d = 384,
synthetic 'rich' weights) for K action chunks per observation,

  replicated : the plain call at batch B*K on state / goal replicated with repeat_interleave -- what a caller did before
               ``candidates``: the encoder, the cross K|V product and the cross-attention fold run B*K times
  candidates : extra_args={"candidates": K} on the B observations -- they run B times

for every (B, K) of --legs.  Rollout-sized legs (B*K <= 8) are graph-replayed from the third identical call on, as in a rollout.

    python tools/candidates_latency.py [--iters 100] [--rounds 3] [--legs 1x8,1x32,32x8,64x4] [--replicated-only | --candidates-only]
                                       [--root DIR]
--replicated-only measures the first form alone (a tree without ``candidates``, e.g. the parent commit as the baseline),
--candidates-only the second (one form per process: a kernel trace of it);
--root imports the package from another checkout.  The legs are run alternately, --rounds times; prints one line per leg and
round and one JSON line with every round, the fastest round per leg and the candidates / replicated ratios."""
import argparse
import json
import os
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="1x8,1x32,32x8,64x4")
    ap.add_argument("--replicated-only", action="store_true")
    ap.add_argument("--candidates-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    assert torch.cuda.is_available(), "candidates_latency measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    legs = [tuple(int(v) for v in leg.split("x")) for leg in args.legs.split(",")]

    def inputs(B, K):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        x = torch.from_numpy(synthetic.sampler_inputs(B * K, cfg, seed=7)["noise"]).cuda() * 80.0
        return {"state_images": t["state_images"], "modality": "lang"}, x, t["goal"]

    def timed(state, x, goal, iters, **kw):
        with torch.no_grad():
            for _ in range(5):  # warm-up: the auto rule captures the graph on the third identical call
                gs.sample_ddim(model, state, x, goal, sig, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                gs.sample_ddim(model, state, x, goal, sig, **kw)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    rounds = {}
    for r in range(args.rounds):
        for B, K in legs:
            state, x, goal = inputs(B, K)
            iters = args.iters if B * K <= 64 else max(10, args.iters // 4)
            wide = {"state_images": state["state_images"].repeat_interleave(K, 0), "modality": "lang"}
            forms = [] if args.candidates_only else [("replicated", (wide, x, goal.repeat_interleave(K, 0)), {})]
            if not args.replicated_only:
                forms.append(("candidates", (state, x, goal), {"extra_args": {"candidates": K}}))
            for form, a, kw in forms:
                ms = timed(*a, iters, **kw)
                rounds.setdefault(f"{B}x{K}_{form}", []).append(ms)
                print(f"round {r}  ({B:3d}, {K:2d}) {form:10s} {ms:8.3f} ms per call", flush=True)
    res = {"rounds": {k: [round(v, 4) for v in vs] for k, vs in rounds.items()},
           "best": {k: round(min(vs), 4) for k, vs in rounds.items()}}
    if not (args.replicated_only or args.candidates_only):
        res["ratio_candidates_over_replicated"] = {f"{B}x{K}": round(min(rounds[f"{B}x{K}_candidates"]) /
                                                                      min(rounds[f"{B}x{K}_replicated"]), 4) for B, K in legs}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
