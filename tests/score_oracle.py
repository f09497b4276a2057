"""The denoising score of gc_sampling.denoising_score / mdt_denoising_score over the oracle network (oracle/mdt_oracle.py), in
the residual form the kernel uses:

    q = sigma / (sigma^2 + sd^2) x0 - c_skip n - sd / sqrt(sigma^2 + sd^2) F,     score = - sum_s w_s (1 / M) sum_m sum_e q^2

with F the network's raw output at x0 + sigma n.  Shared by tests/test_score_float64.py (the algebra against the D form) and
tests/test_gpu_denoising_score.py (the yardstick of the native call, in float64 and -- for the tolerance -- in float32)."""
import math

import torch

from oracle import mdt_oracle as O


def trapezoid(levels):
    """The default weights: half the distance in ln sigma to each neighbour; 1 for a single level."""
    ln = [math.log(v) for v in levels]
    if len(ln) == 1:
        return [1.0]
    d = [abs(b - a) for a, b in zip(ln, ln[1:])]
    return [d[0] / 2] + [(a + b) / 2 for a, b in zip(d, d[1:])] + [d[-1] / 2]


def residual_score(P, cfg, arch, state, goal, x0, levels, noise, weights=None, K=1, sd=0.5, dtype=torch.float64):
    """(score (B*K,), sum of |terms| (B*K,)) in ``dtype``.  ``state`` / ``goal`` hold B observations, ``x0`` (B*K, Ta, A) the chunks,
    chunk k of observation b at row b*K + k; ``noise`` (S, M, Ta, A).  The terms w_s / M q^2 are all >= 0: their absolute sum is
    -score."""
    P = O.to_dtype(P, dtype)
    st = {k: (v.to(dtype).repeat_interleave(K, 0) if torch.is_tensor(v) else v) for k, v in state.items()}
    g = goal.to(dtype).repeat_interleave(K, 0)
    x0, noise = x0.to(dtype), noise.to(dtype)
    w = trapezoid(levels) if weights is None else [float(v) for v in weights]
    R, M = x0.shape[0], noise.shape[1]
    total = torch.zeros(R, dtype=dtype)
    for s, sg in enumerate(levels):
        sigma = torch.full((R,), float(sg), dtype=dtype)
        den2 = sigma[0] * sigma[0] + sd * sd
        c_x, c_n, c_f = sigma[0] / den2, sd * sd / den2, sd / den2.sqrt()
        level = torch.zeros(R, dtype=dtype)
        for m in range(M):
            trace = {}
            O.denoise(P, cfg, st, x0 + sigma[0] * noise[s, m], g, sigma, sd, arch, trace=trace)
            q = c_x * x0 - c_n * noise[s, m] - c_f * trace["action_pred"]
            level = level + (q * q).flatten(1).sum(1)
        total = total + torch.tensor(w[s] / M, dtype=dtype) * level
    return -total, total
