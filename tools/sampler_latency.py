"""Host-synchronised latency of the other samplers through the entry points a user calls (gc_sampling.sample_*): the host loop
(forced with a no-op callback), the routed native call kept eager (the automatic graph rule's call counter is reset before
every call) and the routed call as it runs in a rollout (from the third identical call on, B <= 8, it replays a HIP graph by
itself; larger batches stay eager, reported as null).  Bench model (MDT-V d = 384), exponential schedule on the device as the
agent builds it; sample_dpm_fast takes its two levels (0.001, 80) and its evaluation count as `steps`; sample_dpm_adaptive runs
the agent's defaults over sigma 0.001..80 (`steps`: its evaluation count; it never replays a graph).  One JSON line per
(sampler, B, steps).

    python tools/sampler_latency.py [--iters 20] [--out sampler_latency.jsonl]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from mdt_policy_amd import synthetic  # noqa: E402
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs  # noqa: E402

SAMPLERS = [("euler", {}), ("heun", {}), ("dpmpp_2m", {}), ("euler_ancestral", dict(eta=1.)), ("dpm_2_ancestral", dict(eta=1.))]
CASES = [(1, 10), (1, 20), (256, 10)]
DPM_FAST_CASES = [(1, 10), (1, 11), (256, 10), (256, 11)]  # (B, evaluations)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t.sort()
    return 1e3 * t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    cfg, P, model = bench.build_model(dev)
    rows = []

    def measure(name, B, n, call, graphable=True):
        """call(**extra) runs the sampler once; callback=... forces the host loop."""
        host = timed(lambda: call(callback=lambda d: None), a.iters)

        def eager():
            model.__dict__.pop("_graph_seen", None)  # never reaches the graph rule's third call
            return call()
        native = timed(eager, a.iters)
        graph = None
        if graphable and B <= gs._GRAPH_AUTO_MAX_BATCH:
            model.__dict__.pop("_graphed_native", None)
            model.__dict__.pop("_graph_seen", None)
            graph = timed(call, a.iters)  # warm-up calls build the graph
            assert model.__dict__.get("_graphed_native"), "the routed call did not take the graph path"
        row = dict(sampler=name, B=B, steps=n, host_loop_ms=round(host, 3), native_ms=round(native, 3),
                   graph_ms=None if graph is None else round(graph, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)

    def inputs(B):
        inp = {k: torch.from_numpy(v).to(dev) for k, v in synthetic.sampler_inputs(B, cfg, seed=1).items()}
        return {"state_images": inp["state_images"], "modality": "lang"}, inp["noise"] * 80, inp["goal"]

    with torch.no_grad():
        for B, n in CASES:
            st, x, goal = inputs(B)
            sig = gs.get_sigmas_exponential(n, 0.001, 80.0, device=dev)
            for name, kw in SAMPLERS:
                fn = getattr(gs, "sample_" + name)
                measure(name, B, n, lambda fn=fn, kw=kw, **extra: fn(model, st, x, goal, sig, **kw, **extra))
        for B, n in DPM_FAST_CASES:
            st, x, goal = inputs(B)
            measure("dpm_fast", B, n, lambda **extra: gs.sample_dpm_fast(model, st, x, goal, 0.001, 80.0, n, **extra))
        for B in (1, 256):
            st, x, goal = inputs(B)
            nfe = gs.sample_dpm_adaptive(model, st, x, goal, 0.001, 80.0, return_info=True)[1]["nfe"]
            measure("dpm_adaptive", B, nfe, lambda **extra: gs.sample_dpm_adaptive(model, st, x, goal, 0.001, 80.0, **extra),
                    graphable=False)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
