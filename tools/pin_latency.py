"""Cost of pinned actions on the GPU, in one process: ms per host-synchronised call of 10-step sample_ddim (MDT-V d = 384,
synthetic 'rich' weights) at B = 1 (rollout size, graph-replayed from the third identical call on, calls back to back; and
eager, GCDenoiser.sample_ddim itself, where the host's work per call shows) and at B = 256, without a pin and with one
(extra_args={"pin": ActionPin.overlap(...)}: 2 B Ta A floats more read per step).

    python tools/pin_latency.py [--iters 400] [--passes 3]
The unpinned legs run on a tree without the feature too (the pinned legs are skipped there), which is how a commit is compared
with its parent.  Every timed loop sits between two mdt_op_clock_stamp records on its stream: the shader clock the chip
sustained over exactly those calls is printed beside the time.  Prints every pass of every leg and one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pin_latency measures on the GPU; there is no CPU fallback"
    from mdt_policy_amd import _lib, configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    try:
        from mdt_policy_amd.utils.action_pin import ActionPin
    except ImportError:
        ActionPin = None

    cfg = configs.mdtv_default()
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    model = model.cuda().eval()
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)

    def inputs(B):
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        return {"state_images": t["state_images"], "modality": "lang"}, t["noise"] * 80.0, t["goal"]

    def mhz(stamps):
        """Median over the XCDs of (d s_memtime / d s_memrealtime) x 100 MHz between the two records (bench.py sustained_mhz)."""
        st = stamps.cpu().view(2, 8, 2)
        v = sorted((int(st[1, x, 0] - st[0, x, 0]) / int(st[1, x, 1] - st[0, x, 1]) * 100.0 for x in range(8)
                    if int(st[0, x, 1]) and int(st[1, x, 1]) and int(st[1, x, 1] - st[0, x, 1]) > 0))
        return round(v[len(v) // 2]) if v else None

    def timed(B, iters, pinned, eager=False):
        state, x, goal = inputs(B)
        kw = {"extra_args": {"pin": ActionPin.overlap(x / 80.0, executed=4, hard=2, soft=3)}} if pinned else {}
        call = (lambda: model.sample_ddim(state, x, goal, sig)) if eager else (lambda: gs.sample_ddim(model, state, x, goal, sig, **kw))
        with torch.no_grad():
            for _ in range(5):  # warm-up: the auto rule captures the graph on the third identical call
                call()
            stamps = torch.zeros(2, 16, dtype=torch.int64, device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[0].data_ptr(), stream))
            for _ in range(iters):
                call()
            _lib.check(_lib.load().mdt_op_clock_stamp(stamps[1].data_ptr(), stream))
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3, mhz(stamps)

    def host_us(iters):
        """The eager B = 1 call's host path alone: the stream is drained before every call and only the call's own return is
        timed (Python, ctypes and the enqueue; nothing of the GPU's).  The median over the calls, in microseconds."""
        state, x, goal = inputs(1)
        ts = []
        with torch.no_grad():
            for i in range(iters + 20):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.sample_ddim(state, x, goal, sig)
                ts.append(time.perf_counter() - t0)
        return round(sorted(ts[20:])[iters // 2] * 1e6, 1)

    legs = [("b1_unpinned", 1, args.iters, False), ("b1_eager", 1, args.iters, False, True),
            ("b256_unpinned", 256, max(10, args.iters // 4), False)]
    if ActionPin is not None:
        legs += [("b1_pinned", 1, args.iters, True), ("b256_pinned", 256, max(10, args.iters // 4), True)]
    res = {name: [] for name, *_ in legs}
    clk = {name: [] for name, *_ in legs}
    for _ in range(args.passes):  # the legs alternate: other work shares the host
        for name, *leg in legs:
            ms, f = timed(*leg)
            res[name].append(round(ms, 4))
            clk[name].append(f)
    for k, v in res.items():
        print(f"{k:16s} " + " ".join(f"{ms:8.4f}" for ms in v) + " ms per call   " + " ".join(str(f) for f in clk[k]) + " MHz")
    host = [host_us(max(100, args.iters // 5)) for _ in range(args.passes)]
    print("b1_eager_host    " + " ".join(f"{us:8.1f}" for us in host) + " us of host time per call (stream drained before each)")
    print(json.dumps(dict(res, mhz=clk, b1_eager_host_us=host)))


if __name__ == "__main__":
    main()
