"""Classifier-free guidance cost on the GPU, in one process: ms per host-synchronised call of 10-step sample_ddim (MDT-V d = 384,
synthetic 'rich' weights).

  B = 1 (rollout size, graph-replayed from the third identical call on): unguided, unguided B = 2, guided
      (extra_args={"cond_lambda": 2}), and the guided host loop (a no-op callback forces it: two denoiser calls per step)
  guided B = 256 against unguided B = 512 (the same network work plus the two-row head)

    python tools/guided_latency.py [--iters 200] [--lam 2.0]
Prints one line per leg and one JSON line with every number and the ratios the guided path is judged by."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lam", type=float, default=2.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "guided_latency measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)

    def inputs(B):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        return {"state_images": t["state_images"], "modality": "lang"}, t["noise"] * 80.0, t["goal"]

    def timed(B, iters, **kw):
        state, x, goal = inputs(B)
        with torch.no_grad():
            for _ in range(5):  # warm-up: the auto rule captures the graph on the third identical call
                gs.sample_ddim(model, state, x, goal, sig, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                gs.sample_ddim(model, state, x, goal, sig, **kw)
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    guided = {"extra_args": {"cond_lambda": args.lam}}
    host = {"extra_args": {"cond_lambda": args.lam}, "callback": lambda d: None}
    big = max(10, args.iters // 10)
    res = {}
    # alternate the legs twice and keep the faster pass of each (other work shares the host)
    for _ in range(2):
        for name, B, n, kw in (("b1_unguided", 1, args.iters, {}), ("b2_unguided", 2, args.iters, {}),
                               ("b1_guided", 1, args.iters, guided), ("b1_guided_host_loop", 1, max(10, args.iters // 4), host),
                               ("b256_guided", 256, big, guided), ("b512_unguided", 512, big, {})):
            ms = timed(B, n, **kw)
            res[name] = min(ms, res.get(name, float("inf")))
    for k, v in res.items():
        print(f"{k:22s} {v:8.3f} ms per call")
    res["ratio_b1_guided_over_b2_unguided"] = res["b1_guided"] / res["b2_unguided"]
    res["ratio_b1_host_loop_over_guided"] = res["b1_guided_host_loop"] / res["b1_guided"]
    res["ratio_b256_guided_over_b512_unguided"] = res["b256_guided"] / res["b512_unguided"]
    print(json.dumps({k: round(v, 4) for k, v in res.items()}))


if __name__ == "__main__":
    main()
