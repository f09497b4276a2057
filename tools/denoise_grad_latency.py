"""Forward + backward of GCDenoiser.denoise_grad under an MSE objective next to GCDenoiser.loss forward + backward, MDT-V default
at B = 1024 (BASELINE configs[2]), eval mode, the same event timing for both in one process ("denoise_grad").

    python tools/denoise_grad_latency.py [--batch 1024] [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warm, n):
    """Mean milliseconds per call between two events on the current stream, behind `warm` warm-ups."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    cfg = configs.mdtv_default()
    torch.manual_seed(0)
    model = GCDenoiser(cfg, 0.5).cuda().eval()
    B = a.batch
    inp = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, 1).items()}
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, 2).items()}
    state = {"state_images": inp["state_images"], "modality": "lang"}
    noised = li["actions"] + li["noise_train"] * li["sigma"][:, None, None]

    def loss_step():
        model.zero_grad(set_to_none=True)
        loss, _ = model.loss(state, li["actions"], inp["goal"], li["noise_train"], li["sigma"])
        loss.backward()

    def denoise_step(x=noised, sigma=li["sigma"]):
        model.zero_grad(set_to_none=True)
        den = model.denoise_grad(state, x, inp["goal"], sigma)
        ((den - li["actions"]) ** 2).mean().backward()

    xg, sg = noised.clone().requires_grad_(), li["sigma"].clone().requires_grad_()

    def denoise_step_inputs():
        xg.grad = sg.grad = None
        denoise_step(xg, sg)

    out = {"batch": B,
           "loss_fwd_bwd_ms": round(timed(loss_step, 3, a.iters), 3),
           "denoise_grad_fwd_bwd_ms": round(timed(denoise_step, 3, a.iters), 3),
           "denoise_grad_fwd_bwd_with_dx_dsigma_ms": round(timed(denoise_step_inputs, 3, a.iters), 3)}
    out["ratio"] = round(out["denoise_grad_fwd_bwd_ms"] / out["loss_fwd_bwd_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
