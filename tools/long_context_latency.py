"""What a longer context costs on the GPU, in one process.

  calls : ms per host-synchronised call of 10-step sample_ddim (exponential schedule 0.001 .. 80; shipped MDT-V d = 384, synthetic
          'rich' weights) for every context length of --te (goal + Te - 1 state tokens) and batch of --batch: device events around
          each call, 3 warm-up calls (the third identical rollout-sized call captures its graph), the median of --iters calls.
          Beside it the once-per-call prefix alone -- forward_context_only: the embeddings, the encoder and the cross K|V product
          of every decoder block -- timed the same way.  The step from 16 to 17 tokens is named.
  xattn : the decoder's cross-attention launch alone at B = 256, H = 8, head dim 48, Ta = 10, Te = 64 in the model's layout (K | V
          rows of stride Ld * 2 * D): every key staged (kv_rows = 0) against the visible prefix (kv_rows = 10), through the hooks of
          mdt_hip_debug.h, for the inference forward, the training forward at p = 0.3 and the backward; us per launch from device
          events around --op-iters launches, and the ratio.
  kv    : the cross K|V product (B * rows x Ld * 2 * D columns, K = D, mdt_op_gemm) on all 64 rows of a context against the 10 a
          decoder query can see -- what restricting the product to the visible rows could save at best -- at every batch of --batch.

    python tools/long_context_latency.py [--te 4,16,17,32,64] [--batch 1,64,256] [--iters 20] [--op-iters 50]
                                         [--skip-calls] [--skip-ops]

Prints one line per measurement and one JSON line with everything."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.long_chunk_latency import event_ms  # noqa: E402


def calls(args):
    from mdt_policy_amd import configs, synthetic
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    from mdt_policy_amd.models.edm_diffusion.score_wrappers import GCDenoiser
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    res = {}
    for te in args.te:
        cfg = configs.mdtv_default(n_obs_token=te - 1)
        model = GCDenoiser(cfg, sigma_data=0.5)
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic.fill_state_dict(shapes, seed=5, profile="rich").items()})
        model = model.cuda().eval()
        for B in args.batch:
            t = {k: torch.from_numpy(v).cuda() for k, v in synthetic.sampler_inputs(B, cfg, seed=6).items()}
            state, x, goal = {"state_images": t["state_images"], "modality": "lang"}, t["noise"] * 80.0, t["goal"]
            s0 = torch.full((B,), 80.0, device="cuda")

            def one():
                with torch.no_grad():
                    gs.sample_ddim(model, state, x, goal, sig)

            def prefix():
                with torch.no_grad():
                    model.forward_context_only(state, None, goal, s0)
            med, best = event_ms(one, args.iters, 3)
            pre, pre_best = event_ms(prefix, args.iters, 3)
            res[f"te{te}_b{B}"] = dict(ms_per_call=round(med, 4), ms_min=round(best, 4), prefix_ms=round(pre, 4), prefix_ms_min=round(pre_best, 4))
            print(f"Te {te:2d}  B {B:3d}  {med:8.3f} ms per call (min {best:.3f})  prefix alone {pre:7.3f} ms (min {pre_best:.3f})", flush=True)
        del model
    for B in args.batch:
        a, b = res.get(f"te16_b{B}"), res.get(f"te17_b{B}")
        if a and b:
            print(f"step from Te = 16 to Te = 17 at B = {B}: {a['ms_per_call']:.3f} -> {b['ms_per_call']:.3f} ms per call "
                  f"({b['ms_per_call'] / a['ms_per_call']:.2f} x)")
            res[f"step_16_to_17_b{B}"] = round(b["ms_per_call"] / a["ms_per_call"], 3)
    return res


def many(fn, n):
    def run():
        for _ in range(n):
            fn()
    return run


def xattn(args):
    from mdt_policy_amd import _lib
    lib = _lib.load()
    B, H, hd, Ta, Te, Ld = 256, 8, 48, 10, 64, 4
    D, ldkv = H * hd, Ld * 2 * H * hd
    g = torch.Generator().manual_seed(1)
    q, kv = torch.randn(B * Ta, D, generator=g).cuda(), torch.randn(B * Te, ldkv, generator=g).cuda()
    do, out, dq = torch.randn(B * Ta, D, generator=g).cuda(), torch.empty(B * Ta, D, device="cuda"), torch.empty(B * Ta, D, device="cuda")
    dkv = torch.empty(B * Te, ldkv, device="cuda")
    tab = torch.zeros(64 * 16, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t, col=0: t.data_ptr() + 4 * col
    a = _lib.AttnArgs(q=p(q), ldq=D, k=p(kv), v=p(kv, D), ldkv=ldkv, out=p(out), ldo=D, B=B, H=H, hd=hd, Tq=Ta, Tk=Te, causal=1, rope=0)
    kw = dict(B=B, H=H, hd=hd, Tq=Ta, Tk=Te, causal=1, p=0.3, site=7, seed=12345, rope=0, rope_cos=p(tab), rope_sin=p(tab))
    t = _lib.AttnTrainArgs(q=p(q), ldq=D, k=p(kv), v=p(kv, D), ldkv=ldkv, out=p(out), ldo=D, **kw)
    gb = _lib.AttnBwdArgs(q=p(q), ldq=D, k=p(kv), v=p(kv, D), ldkv=ldkv, d_out=p(do), ld_do=D, dq=p(dq), ld_dq=D, dk=p(dkv), dv=p(dkv, D),
                          ld_dkv=ldkv, accumulate_kv=0, **kw)
    res = {}
    forms = (("forward", lambda rows: _lib.check(lib.mdt_op_attention_prefix(C.byref(a), 1, rows, s))),
             ("training forward", lambda rows: _lib.check(lib.mdt_op_attn_fwd_train_prefix(C.byref(t), rows, s))),
             ("backward", lambda rows: _lib.check(lib.mdt_op_attn_bwd_prefix(C.byref(gb), rows, s))))
    for name, fn in forms:
        us = {}
        for _ in range(2):   # full, prefix, full, prefix: the second pass is the one reported
            for rows in (0, Ta):
                med, _ = event_ms(many(lambda: fn(rows), args.op_iters), 5, 1)
                us[rows] = med * 1e3 / args.op_iters
        res[name] = dict(full_us=round(us[0], 2), prefix_us=round(us[Ta], 2), ratio=round(us[Ta] / us[0], 3))
        print(f"cross-attention {name:17s} every key {us[0]:8.2f} us  visible prefix {us[Ta]:8.2f} us  ({us[Ta] / us[0]:.3f} x)", flush=True)
    return res


def kv(args):
    from mdt_policy_amd import _lib
    lib = _lib.load()
    D, Ld, Te, Tv = 384, 4, 64, 10
    N = Ld * 2 * D
    g = torch.Generator().manual_seed(2)
    s = torch.cuda.current_stream().cuda_stream
    W = (torch.randn(N, D, generator=g) * 0.05).cuda()
    P = torch.zeros(N * D, device="cuda")
    _lib.check(lib.mdt_op_pack_weight(W.data_ptr(), N, D, P.data_ptr(), 0, N, s))
    res = {}
    for B in args.batch:
        ctx, out = torch.randn(B * Te, D, generator=g).cuda(), torch.empty(B * Te, N, device="cuda")
        us = {}
        for rows in (Te, Tv):
            a = _lib.GemmArgs()
            a.A, a.lda, a.Wp, a.out, a.ldo, a.M, a.N, a.K = ctx.data_ptr(), D, P.data_ptr(), out.data_ptr(), N, B * rows, N, D
            a.shift_off = a.scale_off = a.gate_off = -1
            a.rows_per_sample = a.gin = a.gout = 1
            med, _ = event_ms(many(lambda: _lib.check(lib.mdt_op_gemm(C.byref(a), s)), args.op_iters), 5, 1)
            us[rows] = med * 1e3 / args.op_iters
        res[f"b{B}"] = dict(whole_us=round(us[Te], 2), visible_us=round(us[Tv], 2))
        print(f"K|V product B {B:3d}: {B * Te:5d} rows {us[Te]:8.2f} us  {B * Tv:5d} visible rows {us[Tv]:8.2f} us  "
              f"(saves at best {us[Te] - us[Tv]:.2f} us per call)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--te", default="4,16,17,32,64")
    ap.add_argument("--batch", default="1,64,256")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    args = ap.parse_args()
    args.te = [int(v) for v in args.te.split(",")]
    args.batch = [int(v) for v in args.batch.split(",")]
    assert torch.cuda.is_available(), "long_context_latency measures on the GPU; there is no CPU fallback"
    res = {}
    if not args.skip_calls:
        res["calls"] = calls(args)
    if not args.skip_ops:
        res["xattn"] = xattn(args)
        res["kv"] = kv(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
