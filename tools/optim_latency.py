"""Latency of the optimizer tail of a training step on the MDT-V default parameter list (about 22.5 M elements), with real
gradients from one backward.  Four comparisons, all in one process, per repeat one pair of device events and a host clock that
ends in a device synchronise:

  (a) amp_tail_host    unscale_ + clip_grad_norm_ + GradScaler.step(FusedAdamW without the AMP protocol): the tail before
                       the device-driven step existed (two read-modify-write passes over the gradients, found_inf.item())
  (b) amp_tail_device  GradScaler.step(FusedAdamW(max_grad_norm=...)): mdt_op_multi_sumsq + mdt_op_multi_adamw_dev
  (c) plain_step       FusedAdamW.step() without scaler or clipping (compare across two checkouts with --package-root)
  (d) norms_hook       the agent's on_before_zero_grad loop (one .item() per tensor) against total_norms + one .item()

and the achieved read rate of the sum-of-squares launches alone.  Prints one JSON line.

    python tools/optim_latency.py [--reps 50] [--warmup 10] [--only plain] [--package-root DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--only", choices=["all", "plain"], default="all")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to import mdt_policy_amd from (plain_step of another commit)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    from mdt_policy_amd.optim import FusedAdamW
    if not torch.cuda.is_available():
        raise SystemExit("optim_latency needs a GPU: a CPU run says nothing about these times")

    cfg = configs.mdtv_default()
    torch.manual_seed(0)
    model = GCDenoiser(cfg, 0.5).cuda().train()
    inp = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(args.batch, cfg, 1).items()}
    li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(args.batch, cfg, 2).items()}
    state = {"state_images": inp["state_images"], "modality": "lang"}
    model.loss(state, li["actions"], inp["goal"], li["noise_train"], li["sigma"])[0].backward()
    params = [p for p in model.parameters() if p.grad is not None]
    true_grads = [p.grad.clone() for p in params]
    numel = sum(p.numel() for p in params)
    scale = 1024.0

    def set_grads(mult):
        torch._foreach_copy_([p.grad for p in params], true_grads)
        if mult != 1.0:
            torch._foreach_mul_([p.grad for p in params], mult)

    def timed(body, before=lambda: None):
        """Median device-event and host-clock milliseconds of body() over the repeats; before() runs untimed."""
        ev, wall = [], []
        for i in range(args.warmup + args.reps):
            before()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            body()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= args.warmup:
                ev.append(a.elapsed_time(b))
                wall.append((t1 - t0) * 1e3)
        q = statistics.quantiles(ev, n=10)
        return {"event_ms": round(statistics.median(ev), 4), "event_p10_ms": round(q[0], 4), "event_p90_ms": round(q[-1], 4),
                "host_ms": round(statistics.median(wall), 4)}

    res = {"numel": numel, "tensors": len(params), "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    plain = FusedAdamW(params, lr=1e-4, weight_decay=0.05)
    res["plain_step"] = timed(plain.step, lambda: set_grads(1.0))
    if args.only == "plain":
        print(json.dumps(res))
        return

    from mdt_policy_amd.optim import total_norms
    from mdt_policy_amd.optim.norms import multi_sumsq

    class HostTail(FusedAdamW):  # what GradScaler saw before: no protocol, so it unscales and reads found_inf back itself
        _step_supports_amp_scaling = False

    host_opt = HostTail(params, lr=1e-4, weight_decay=0.05)
    host_scaler = torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=10 ** 9)
    host_scaler.scale(torch.zeros((), device="cuda"))

    def host_tail():
        host_scaler.unscale_(host_opt)
        torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        host_scaler.step(host_opt)
        host_scaler.update()

    dev_opt = FusedAdamW(params, lr=1e-4, weight_decay=0.05, max_grad_norm=args.max_norm)
    dev_scaler = torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=10 ** 9)
    dev_scaler.scale(torch.zeros((), device="cuda"))

    def dev_tail():
        dev_scaler.step(dev_opt)
        dev_scaler.update()

    # interleaved: a, b, a, b, plain again -- the spread between the two rounds is the noise to read the difference against
    for rnd in range(2):
        res[f"amp_tail_host_{rnd}"] = timed(host_tail, lambda: set_grads(scale))
        res[f"amp_tail_device_{rnd}"] = timed(dev_tail, lambda: set_grads(scale))
    res["plain_step_again"] = timed(plain.step, lambda: set_grads(1.0))

    set_grads(1.0)
    allp = list(model.parameters())

    def hook_loop():
        total_grad_norm = total_param_norm = 0.0
        for p in allp:
            if p.grad is not None:
                total_grad_norm += p.grad.norm().item() ** 2
            total_param_norm += p.norm().item() ** 2
        return total_grad_norm ** 0.5, total_param_norm ** 0.5

    def fused_norms():
        gn, pn = total_norms(allp)
        return torch.stack((gn, pn)).tolist()  # the one read-back

    res["norms_hook"] = timed(hook_loop)
    res["norms_fused"] = timed(fused_norms)
    res["norms_values"] = {"hook": list(hook_loop()), "fused": fused_norms()}

    grads = [p.grad for p in params]
    partials = torch.empty(2 * sum((g.numel() + 4095) // 4096 for g in grads), device="cuda")
    t = timed(lambda: multi_sumsq(grads, 0, partials))
    t["read_GBps"] = round(4.0 * numel / (t["event_ms"] * 1e-3) / 1e9, 1)  # the bytes the reduction has to read, over its time
    res["sumsq_launches"] = t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
