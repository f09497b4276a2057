"""The Brownian tree behind sample_dpmpp_sde's default noise sampler (include/mdt_hip.h mdt_brownian_noise_host, csrc/mdt_brownian.h)
on the CPU: against a float64 numpy restatement of its definition, its law, the tree's own properties, the seed modes, and the
default noise sampler without torchsde."""
import importlib.util
import math

import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from tests.dropout_masks import philox4
from tests.helpers import load_fixture


def normal(seed, e, node):
    w0, w1, w2, w3 = philox4(seed, e, node)
    k1 = (w0 >> np.uint64(5)) * np.uint64(1 << 26) + (w1 >> np.uint64(6))
    k2 = (w2 >> np.uint64(5)) * np.uint64(1 << 26) + (w3 >> np.uint64(6))
    u1 = (k1 + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = k2.astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def tree_value(seed, e, lo, hi, tol, t):
    """W(t) of the tree (seed, e) on [lo, hi]: the Levy midpoint walk, float64 (the path is the same for every element)."""
    t = min(max(t, lo), hi)
    a, b, wa, wb, node, depth = lo, hi, np.zeros(np.shape(e)), math.sqrt(hi - lo) * normal(seed, e, 0), 1, 0
    while depth < 62 and b - a > tol:
        m = a + (b - a) / 2
        wm = (wa + wb) / 2 + 0.5 * math.sqrt(b - a) * normal(seed, e, node)
        if t < m:
            b, wb, node = m, wm, 2 * node
        else:
            a, wa, node = m, wm, 2 * node + 1
        depth += 1
    return wa + (t - a) / (b - a) * (wb - wa)


def restated(seeds, lo, hi, tol, pairs, batch, per_row):
    """(n_q, batch, per_row) float32 noise values of the definition in include/mdt_hip.h."""
    out = np.empty((len(pairs), batch, per_row), dtype=np.float32)
    for q, (f, t) in enumerate(pairs):
        for b in range(batch):
            if len(seeds) == 1:
                seed, e = seeds[0], np.arange(b * per_row, (b + 1) * per_row, dtype=np.uint64)
            else:
                seed, e = seeds[b], np.arange(per_row, dtype=np.uint64)
            w = (tree_value(seed, e, lo, hi, tol, t) - tree_value(seed, e, lo, hi, tol, f)) / math.sqrt(abs(t - f))
            out[q, b] = w.astype(np.float32)
    return out


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


LO, HI, TOL = 0.001, 80.0, 1e-6
PAIRS = [(80.0, 35.2), (80.0, 12.5), (12.5, 5.1), (12.5, 2.0), (0.0123, 0.0041), (0.0041, 0.001), (2.0, 80.0), (0.5, 0.5000001)]


@pytest.mark.parametrize("seeds,batch,per_row", [([12345], 64, 70), ([2 ** 63 - 5], 3, 11), ([7, 8, 9, 2 ** 62 + 1, 0], 5, 70)])
def test_host_helper_matches_the_numpy_restatement(seeds, batch, per_row):
    got = _lib.brownian_noise_host(seeds, LO, HI, TOL, PAIRS, batch, per_row)
    want = restated(seeds, LO, HI, TOL, PAIRS, batch, per_row)
    assert got.shape == want.shape
    assert int(ulps(got, want).max()) <= 1, f"max {int(ulps(got, want).max())} ulp"


def test_coarse_tolerance_and_clamped_points_match_the_restatement():
    pairs = [(-1.0, 3.0), (90.0, 0.5), (7.25, 7.5)]
    got = _lib.brownian_noise_host([99], 0.002, 60.0, 0.37, pairs, 2, 9)
    want = restated([99], 0.002, 60.0, 0.37, pairs, 2, 9)
    assert int(ulps(got, want).max()) <= 1


def _sde_points(sig, i, r=0.5):
    """(sigma(t), sigma(s), sigma(t_next)) of dpmpp_sde's step i as its loop forms them (fp32 0-dim tensors)."""
    t, tn = -torch.log(sig[i]), -torch.log(sig[i + 1])
    s = t + (tn - t) * r
    return float(torch.exp(-t)), float(torch.exp(-s)), float(torch.exp(-tn))


def test_law_over_a_million_elements():
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    sig = gs.get_sigmas_exponential(10, LO, HI)
    f0, s0, n0 = _sde_points(sig, 0)
    f5, s5, n5 = _sde_points(sig, 5)
    N = 1 << 20
    v = _lib.brownian_noise_host([2024], float(sig[-2]), float(sig[0]), TOL, [(f0, s0), (f0, n0), (f5, s5), (f5, n5)], 1, N)[:, 0]
    v = v.astype(np.float64)
    se = 1.0 / math.sqrt(N)
    for row in v:
        assert abs(row.mean()) < 6 * se
        assert abs(row.var() - 1.0) < 6 * math.sqrt(2.0) * se
    for (a, b, fr, s, n) in ((0, 1, f0, s0, n0), (2, 3, f5, s5, n5)):
        rho = math.sqrt(abs(fr - s) / abs(fr - n))
        got = np.corrcoef(v[a], v[b])[0, 1]
        assert abs(got - rho) < 6 * (1 - rho * rho) * se + 1e-4, (got, rho)
    for a, b in ((0, 2), (1, 3), (0, 3), (1, 2)):
        assert abs(np.corrcoef(v[a], v[b])[0, 1]) < 6 * se


def test_additivity_antisymmetry_and_query_independence():
    pts = [80.0, 31.7, 9.25, 0.73, 0.0419, 0.001]
    per_row = 500
    for a, b, c in [(pts[0], pts[2], pts[4]), (pts[5], pts[3], pts[1]), (pts[1], pts[2], pts[3])]:
        n = _lib.brownian_noise_host([31337], LO, HI, TOL, [(a, b), (b, c), (a, c)], 1, per_row)[:, 0].astype(np.float64)
        lhs = math.sqrt(abs(b - a)) * n[0] + math.sqrt(abs(c - b)) * n[1]
        rhs = math.sqrt(abs(c - a)) * n[2]
        scale = math.sqrt(abs(b - a)) * np.abs(n[0]) + math.sqrt(abs(c - b)) * np.abs(n[1]) + np.abs(rhs)
        assert np.all(np.abs(lhs - rhs) <= 4 * 2.0 ** -24 * scale + 1e-12)
        rev = _lib.brownian_noise_host([31337], LO, HI, TOL, [(b, a)], 1, per_row)[0, 0]
        assert np.array_equal(rev, -n[0].astype(np.float32))
    pairs = [(pts[i], pts[j]) for i in range(len(pts)) for j in range(len(pts)) if i != j]
    together = _lib.brownian_noise_host([5], LO, HI, TOL, pairs, 2, 40)
    rng = np.random.default_rng(0)
    for q in rng.permutation(len(pairs))[:8]:
        alone = _lib.brownian_noise_host([5], LO, HI, TOL, [pairs[q]], 2, 40)[0]
        assert np.array_equal(alone, together[q])
    shuffled = rng.permutation(len(pairs))
    again = _lib.brownian_noise_host([5], LO, HI, TOL, [pairs[q] for q in shuffled], 2, 40)
    assert np.array_equal(again, together[shuffled])


def test_per_row_seeds_make_each_sample_independent_of_the_batch():
    seeds = [11, 2 ** 63 - 2, 0, 424242]
    batched = _lib.brownian_noise_host(seeds, LO, HI, TOL, PAIRS[:4], len(seeds), 70)
    for b, s in enumerate(seeds):
        alone = _lib.brownian_noise_host([s], LO, HI, TOL, PAIRS[:4], 1, 70)
        assert np.array_equal(batched[:, b], alone[:, 0])
    # one seed for the whole tensor: element index runs across the batch
    one = _lib.brownian_noise_host([11], LO, HI, TOL, PAIRS[:2], 4, 70)
    flat = _lib.brownian_noise_host([11], LO, HI, TOL, PAIRS[:2], 1, 280)
    assert np.array_equal(one.reshape(2, -1), flat.reshape(2, -1))


def test_refusals():
    with pytest.raises(_lib.MDTHipError):
        _lib.brownian_noise_host([1], LO, HI, 1e-30, PAIRS[:1], 1, 4)  # more than 62 levels
    with pytest.raises(_lib.MDTHipError):
        _lib.brownian_noise_host([1], HI, LO, TOL, PAIRS[:1], 1, 4)  # lo >= hi
    with pytest.raises(_lib.MDTHipError):
        _lib.brownian_noise_host([1, 2], LO, HI, TOL, PAIRS[:1], 3, 4)  # n_seeds neither 1 nor batch
    with pytest.raises(_lib.MDTHipError):
        _lib.brownian_noise_host([1], LO, HI, 0.0, PAIRS[:1], 1, 4)


def test_sampler_object_values_and_seed_draw():
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    x = torch.zeros(3, 10, 7)
    torch.manual_seed(77)
    ns = gs.NativeBrownianTreeNoiseSampler(x, torch.tensor(0.001), torch.tensor(80.0))
    after = torch.rand(4)
    torch.manual_seed(77)
    seed = torch.randint(0, 2 ** 63 - 1, []).item()
    assert torch.equal(torch.rand(4), after), "seed=None must take exactly one randint draw"
    assert ns.seeds == [seed]
    got = ns(torch.tensor(80.0), torch.tensor(12.5))
    assert got.shape == x.shape and got.dtype == x.dtype
    want = _lib.brownian_noise_host([seed], float(torch.tensor(0.001)), 80.0, TOL, [(80.0, 12.5)], 1, x.numel())
    assert np.array_equal(got.numpy().reshape(-1), want.reshape(-1))
    per = gs.NativeBrownianTreeNoiseSampler(x, 0.001, 80.0, seed=[4, 5, 6])
    v = per(80.0, 12.5)
    assert np.array_equal(v[1].numpy().reshape(-1),
                          _lib.brownian_noise_host([5], float(torch.tensor(0.001)), 80.0, TOL, [(80.0, 12.5)], 1, 70).reshape(-1))
    with pytest.raises(ValueError):
        gs.NativeBrownianTreeNoiseSampler(x, 0.001, 80.0, seed=[1, 2])
    dec = gs.NativeBrownianTreeNoiseSampler(x, 0.001, 80.0, seed=9, transform=lambda s: -s)  # reversed orientation: reference sign
    inc = gs.NativeBrownianTreeNoiseSampler(x, -80.0, -0.001, seed=9)
    assert torch.equal(dec(80.0, 12.5), -inc(-80.0, -12.5))


def _oracle_model(meta):
    from oracle import mdt_oracle as O
    from tests.helpers import cfg_of, inputs_of, params_of
    cfg, P = cfg_of(meta), params_of(meta)
    state, goal, noise = inputs_of(meta)
    ctx = O.encode(P, cfg, state, goal)
    return (lambda s, x, g, sigma: O.denoise(P, cfg, s, x, g, sigma, ctx=ctx)), state, goal, noise


@pytest.mark.skipif(importlib.util.find_spec("torchsde") is not None, reason="torchsde is installed: the default is its tree")
def test_default_noise_sampler_runs_without_torchsde():
    """The reference's call form -- no noise_sampler -- used to raise ImportError here; it now walks the native tree."""
    from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
    assert isinstance(gs.BrownianTreeNoiseSampler(torch.zeros(2), 0.001, 80.0, seed=1), gs.NativeBrownianTreeNoiseSampler)
    meta, _ = load_fixture("g7c_samplers.npz")
    model, state, goal, noise = _oracle_model(meta)
    x0 = noise * 80.0
    sig = gs.get_sigmas_exponential(10, 0.001, 80.0)
    torch.manual_seed(5)
    got = gs.sample_dpmpp_sde(model, state, x0.clone(), goal, sig)
    torch.manual_seed(5)
    seed = torch.randint(0, 2 ** 63 - 1, []).item()
    ns = gs.NativeBrownianTreeNoiseSampler(x0, sig[sig > 0].min(), sig.max(), seed=seed)
    want = gs.sample_dpmpp_sde(model, state, x0.clone(), goal, sig, noise_sampler=ns)
    assert torch.equal(got, want)
    assert torch.isfinite(got).all()
    det = gs.sample_dpmpp_sde(model, state, x0.clone(), goal, sig, eta=0., noise_sampler=lambda a, b: None)
    assert not torch.equal(got, det)  # the noise reached the result
