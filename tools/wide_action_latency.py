"""What a wider action vector costs on the GPU, in one process.

  calls : ms per host-synchronised call of 10-step sample_ddim (exponential schedule 0.001 .. 80; shipped MDT-V d = 384, synthetic
          'rich' weights) for every action_dim of --a and batch of --batch: device events around each call, 3 warm-up calls (the
          third identical rollout-sized call captures its graph), the median of --iters calls; the step from 16 to 17 elements --
          where head_rows (one wave per row, every column's weight fragments in registers) hands over to the tiled head of
          mdt_head_wide.hip -- is named.
  head  : the head launch alone (mdt_op_head, DDIM mode with the next input's embedding, D = 384) at A = 16 (head_rows), 17 and
          64 (k_head_wide) on 10, 640 and 2560 rows: us per launch from device events around --op-iters launches.

    python tools/wide_action_latency.py [--a 7,16,17,32,64] [--batch 1,64,256] [--iters 20] [--op-iters 200] [--skip-head]

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
    for A in args.a:
        cfg = configs.mdtv_default(action_dim=A)
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
            res[f"a{A}_b{B}"] = dict(ms_per_call=round(med, 4), ms_min=round(best, 4))
            print(f"A {A:2d}  B {B:3d}  {med:8.3f} ms per call (min {best:.3f})", flush=True)
        del model
    for B in args.batch:
        a, b = res.get(f"a16_b{B}"), res.get(f"a17_b{B}")
        if a and b:
            print(f"step from A = 16 to A = 17 at B = {B}: {a['ms_per_call']:.3f} -> {b['ms_per_call']:.3f} ms per call "
                  f"({b['ms_per_call'] / a['ms_per_call']:.3f} x)")
            res[f"step_16_to_17_b{B}"] = round(b["ms_per_call"] / a["ms_per_call"], 3)
    return res


def head(args):
    from mdt_policy_amd import _lib
    lib = _lib.load()
    D, T = 384, 10
    s = torch.cuda.current_stream().cuda_stream
    n = args.op_iters
    res = {}
    for M in (10, 640, 2560):
        for A in (16, 17, 64):
            g = torch.Generator().manual_seed(A)
            t = dict(y=torch.randn(M, D, generator=g), ln_w=torch.ones(D), ln_b=torch.zeros(D), Wp=torch.randn(A, D, generator=g) / 20,
                     bp=torch.zeros(A), x=torch.randn(M, A, generator=g), sigma=torch.full((M // T,), 2.0), step=torch.tensor([0.3, 0.7, 1.0]),
                     Wa=torch.randn(A, D, generator=g), ba=torch.zeros(D), out=torch.empty(M, A), y_next=torch.empty(M, D))
            t = {k: v.cuda() for k, v in t.items()}
            a = _lib.HeadArgs()
            a.y, a.ln_w, a.ln_b, a.Wp, a.bp, a.x = (t[k].data_ptr() for k in ("y", "ln_w", "ln_b", "Wp", "bp", "x"))
            a.sigma, a.sigma_stride, a.out = t["sigma"].data_ptr(), 1, t["out"].data_ptr()
            a.M, a.D, a.A, a.rows_per_sample, a.mode, a.sigma_data, a.step = M, D, A, T, _lib.HEAD["ddim"], 0.5, t["step"].data_ptr()
            a.y_next, a.Wa, a.ba = t["y_next"].data_ptr(), t["Wa"].data_ptr(), t["ba"].data_ptr()

            def run():
                for _ in range(n):
                    _lib.check(lib.mdt_op_head(C.byref(a), s))
            med, _ = event_ms(run, 5, 1)
            res[f"m{M}_a{A}"] = round(med * 1e3 / n, 2)
            print(f"head  M {M:4d}  A {A:2d}  {med * 1e3 / n:7.2f} us per launch ({'head_rows' if A <= 16 else 'k_head_wide'})", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", default="7,16,17,32,64")
    ap.add_argument("--batch", default="1,64,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op-iters", type=int, default=200)
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    args.a = [int(v) for v in args.a.split(",")]
    args.batch = [int(v) for v in args.batch.split(",")]
    assert torch.cuda.is_available(), "wide_action_latency measures on the GPU; there is no CPU fallback"
    res = {}
    if not args.skip_calls:
        res["calls"] = calls(args)
    if not args.skip_head:
        res["head"] = head(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
