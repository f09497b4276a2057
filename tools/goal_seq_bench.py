"""What a goal of G tokens costs on the GPU against the same context length built from state tokens, in one process.

  calls : ms per host-synchronised call of 10-step sample_ddim (exponential schedule 0.001 .. 80; shipped MDT-V d = 384, synthetic
          'rich' weights) at every batch of --batch (B <= 8: the third identical call captures its graph, the timed calls replay
          it) for every G of --g with n_obs_token = 3 -- the goal form, Te = G + 3 -- and for a goal_seq_len = 1 model with
          n_obs_token = 3 + G - 1 -- the state form, the same Te.  The two forms do the same work apart from the embedder's weight
          matrix (goal_emb: Linear-GELU-Linear on goal_dim = 512; tok_emb: one Linear on obs_dim = 384).  The two models are timed
          in ALTERNATING runs of --iters calls each (goal, state, goal, state ... --rounds times, device events around each
          call); reported per form: the median over all its calls and the interquartile spread of its per-run medians, and the
          difference of the two medians.
  pos   : MDT (mdt_tiny) at G = 3 with and without use_abs_pos_emb at B = 1, the same way: the position rows of a goal of several
          tokens are one row-add launch of their own, and this is what it costs.
  train : ms per training step (GCDenoiser.loss and its backward under autograd, train() mode at the shipped dropouts) of shipped
          MDT-V at --train-batch for G = 2 and G = 1, alternating, for orientation.

    python tools/goal_seq_bench.py [--g 1,2,8,32] [--batch 1,256] [--iters 20] [--rounds 5] [--train-batch 1024] [--skip-train]

Prints one line per measurement and one JSON line with everything."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(cfg, arch="mdtv"):
    from mdt_policy_amd import synthetic
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    model = GCDenoiser(cfg, sigma_data=0.5)
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
    return model.cuda().eval()


def sampler_call(model, cfg, B, arch="mdtv"):
    from mdt_policy_amd import synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6, arch=arch).items()}
    state = {k: v for k, v in t.items() if k not in ("goal", "noise")}
    state["modality"] = "lang"
    x, goal = t["noise"] * 80.0, t["goal"]

    def one():
        with torch.no_grad():
            gs.sample_ddim(model, state, x, goal, sig)
    return one


def timed(fn, iters):
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(fns, iters, rounds, warmup=4):
    """{name: (median of all calls, interquartile spread of the per-run medians, per-run medians)} of the callables of ``fns``,
    timed in alternating runs of ``iters`` calls."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    every = {k: [] for k in fns}
    runs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms = timed(fn, iters)
            every[k] += ms
            runs[k].append(statistics.median(ms))
    res = {}
    for k in fns:
        q = statistics.quantiles(runs[k], n=4) if len(runs[k]) >= 2 else [runs[k][0]] * 3
        res[k] = dict(ms=round(statistics.median(every[k]), 4), iqr=round(q[2] - q[0], 4), runs=[round(v, 4) for v in runs[k]])
    return res


def calls(args):
    from mdt_policy_amd import configs
    res = {}
    for G in args.g:
        cfg_goal = configs.mdtv_default(goal_seq_len=G, n_obs_token=3)
        cfg_state = configs.mdtv_default(goal_seq_len=1, n_obs_token=3 + G - 1)
        m_goal, m_state = build(cfg_goal), build(cfg_state)
        for B in args.batch:
            r = alternate({"goal": sampler_call(m_goal, cfg_goal, B), "state": sampler_call(m_state, cfg_state, B)}, args.iters, args.rounds)
            r["diff_ms"] = round(r["goal"]["ms"] - r["state"]["ms"], 4)
            res[f"g{G}_b{B}"] = r
            print(f"G {G:2d} (Te {G + 3:2d})  B {B:3d}  goal form {r['goal']['ms']:8.3f} ms (iqr {r['goal']['iqr']:.3f})  "
                  f"state form {r['state']['ms']:8.3f} ms (iqr {r['state']['iqr']:.3f})  goal - state {r['diff_ms']:+.3f} ms", flush=True)
        del m_goal, m_state
    return res


def pos(args):
    from mdt_policy_amd import configs
    cfgs = {"pos": configs.mdt_tiny(goal_seq_len=3, use_abs_pos_emb=True), "nopos": configs.mdt_tiny(goal_seq_len=3, use_abs_pos_emb=False)}
    models = {k: build(c, "mdt") for k, c in cfgs.items()}
    r = alternate({k: sampler_call(models[k], cfgs[k], 1, "mdt") for k in cfgs}, args.iters, args.rounds)
    r["diff_ms"] = round(r["pos"]["ms"] - r["nopos"]["ms"], 4)
    print(f"MDT tiny G 3 B 1  with position rows {r['pos']['ms']:.3f} ms (iqr {r['pos']['iqr']:.3f})  without {r['nopos']['ms']:.3f} ms "
          f"(iqr {r['nopos']['iqr']:.3f})  pos - nopos {r['diff_ms']:+.3f} ms", flush=True)
    return r


def train(args):
    from mdt_policy_amd import configs, synthetic
    B = args.train_batch
    fns = {}
    for G in (2, 1):
        cfg = configs.mdtv_default(goal_seq_len=G)
        model = build(cfg).train()
        t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
        li = {k: torch.from_numpy(v).cuda() for k, v in synthetic.loss_inputs(B, cfg, seed=7).items()}
        state = {"state_images": t["state_images"], "modality": "lang"}

        def step(model=model, state=state, t=t, li=li):
            model.zero_grad(set_to_none=True)
            loss, _ = model.loss(state, li["actions"], t["goal"], li["noise_train"], li["sigma"])
            loss.backward()
        fns[f"g{G}"] = step
    r = alternate(fns, max(5, args.iters // 2), args.rounds)
    print(f"training step B {B}: G 2 {r['g2']['ms']:.3f} ms (iqr {r['g2']['iqr']:.3f})  G 1 {r['g1']['ms']:.3f} ms (iqr {r['g1']['iqr']:.3f})", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g", default="1,2,8,32")
    ap.add_argument("--batch", default="1,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--train-batch", type=int, default=1024)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    args.g = [int(v) for v in args.g.split(",")]
    args.batch = [int(v) for v in args.batch.split(",")]
    assert torch.cuda.is_available(), "goal_seq_bench measures on the GPU; there is no CPU fallback"
    res = {"calls": calls(args), "pos": pos(args)}
    if not args.skip_train:
        res["train"] = train(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
