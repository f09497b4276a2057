"""gc_sampling.denoising_score on the host (no device): the definition

    score = - sum_s w_s (1 / M) sum_m || (x0 - D(x0 + sigma_s n[s, m]; sigma_s)) / sigma_s ||^2

through the foreign-model path against closed forms -- a linear denoiser, the default trapezoid weights in ln sigma, the
antithetic noise layout and what it draws from the generator, the refusals, both action layouts -- and on a Gaussian-mixture toy
with its exact posterior-mean denoiser, where the score must rank candidates like the exact log p."""
import math

import numpy as np
import pytest
import torch

from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.helpers import assert_close

TA, A = 10, 7
LEVELS16 = [math.exp(v) for v in np.linspace(math.log(80.0), math.log(0.001), 16)]


def trapezoid(levels):
    """The default weights by hand: half the distance in ln sigma to each neighbour."""
    ln = [math.log(v) for v in levels]
    if len(ln) == 1:
        return [1.0]
    d = [abs(b - a) for a, b in zip(ln, ln[1:])]
    return [d[0] / 2] + [(a + b) / 2 for a, b in zip(d, d[1:])] + [d[-1] / 2]


def test_a_linear_denoiser_gives_the_closed_form():
    """D = a(sigma) x, a = s^2 / (s^2 + sigma^2): q = (1 - a) x0 / sigma - a n, summed by hand in float64."""
    s2 = 0.7 ** 2
    model = lambda state, x, goal, sigma: x * (s2 / (s2 + sigma ** 2)).reshape(-1, 1, 1)
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(5, TA, A, dtype=torch.float64, generator=g) * 0.7
    levels, w = [30.0, 1.5, 0.2, 0.004], [0.3, 1.0, 0.0, 2.5]
    noise = torch.randn(len(levels), 3, TA, A, dtype=torch.float64, generator=g)
    got = gs.denoising_score(model, {}, x0, None, levels, weights=w, noise=noise)
    want = torch.zeros(5, dtype=torch.float64)
    for s, (sg, ws) in enumerate(zip(levels, w)):
        a = s2 / (s2 + sg * sg)
        for m in range(3):
            want -= ws / 3 * (((1 - a) / sg * x0 - a * noise[s, m]) ** 2).flatten(1).sum(1)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,)
    assert_close(got, want, rtol=1e-12, atol=1e-12, what="linear denoiser")


@pytest.mark.parametrize("levels", [[0.3], [80.0, 2.0, 0.05, 0.001], [0.001, 0.05, 2.0, 80.0], [5.0, 0.5]])
def test_the_default_weights_are_the_trapezoid_rule_in_ln_sigma(levels):
    """With D = 0 and n = 0 the score is - sum_s w_s |x0|^2 / sigma_s^2: the weights can be read off."""
    model = lambda state, x, goal, sigma: torch.zeros_like(x)
    x0 = torch.randn(3, TA, A, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    noise = torch.zeros(len(levels), 1, TA, A, dtype=torch.float64)
    got = gs.denoising_score(model, {}, x0, None, levels, noise=noise)
    want = -sum(w / sg ** 2 for w, sg in zip(trapezoid(levels), levels)) * (x0 ** 2).flatten(1).sum(1)
    assert_close(got, want, rtol=1e-12, atol=0, what="default weights")
    explicit = gs.denoising_score(model, {}, x0, None, levels, noise=noise, weights=trapezoid(levels))
    assert_close(got, explicit, rtol=1e-12, atol=0, what="default against explicit weights")


def test_default_weights_need_monotone_levels_and_given_weights_do_not():
    model = lambda state, x, goal, sigma: torch.zeros_like(x)
    x0 = torch.ones(2, TA, A)
    with pytest.raises(ValueError, match=r"sigmas\[2\].*monotone"):
        gs.denoising_score(model, {}, x0, None, [80.0, 2.0, 3.0])
    with pytest.raises(ValueError, match=r"sigmas\[1\].*monotone"):
        gs.denoising_score(model, {}, x0, None, [2.0, 2.0])
    gs.denoising_score(model, {}, x0, None, [80.0, 2.0, 3.0], weights=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match=r"sigmas\[1\]"):
        gs.denoising_score(model, {}, x0, None, [80.0, 0.0])
    with pytest.raises(ValueError, match=r"weights\[0\]"):
        gs.denoising_score(model, {}, x0, None, [80.0, 1.0], weights=[-1.0, 1.0])
    with pytest.raises(ValueError, match="weights hold 1"):
        gs.denoising_score(model, {}, x0, None, [80.0, 1.0], weights=[1.0])


class Recorder:
    """A model that keeps sigma n = x - x0 of every call."""

    def __init__(self, x0):
        self.x0, self.seen = x0, []

    def __call__(self, state, x, goal, sigma):
        self.seen.append(((x - self.x0) / sigma.reshape(-1, 1, 1), float(sigma[0])))
        return torch.zeros_like(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_antithetic_rows_follow_their_partner_and_cost_half_the_draws(dtype):
    S, M = 3, 4
    levels = [4.0, 1.0, 0.25]
    x0 = torch.zeros(2, TA, A, dtype=dtype)
    rec = Recorder(x0)
    torch.manual_seed(5)
    gs.denoising_score(rec, {}, x0, None, levels, draws=M)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    want = torch.randn(S, M // 2, TA, A, dtype=dtype)
    assert torch.equal(after, torch.get_rng_state()), "the call must leave the generator where S * M / 2 rows of randn leave it"
    assert len(rec.seen) == S * M and [sg for _, sg in rec.seen] == [v for v in levels for _ in range(M)]
    for s in range(S):
        for i in range(M // 2):
            n, neg = rec.seen[s * M + 2 * i][0], rec.seen[s * M + 2 * i + 1][0]
            assert n.dtype == dtype and torch.equal(n, -neg)  # powers of two: sigma n / sigma is exact
            assert torch.equal(n[0], want[s, i]) and torch.equal(n[1], want[s, i]), "the same rows serve every chunk, in (S, M) order"
    # without the pairs: S * M independent rows
    rec = Recorder(x0)
    torch.manual_seed(5)
    gs.denoising_score(rec, {}, x0, None, levels, draws=M, antithetic=False)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    want = torch.randn(S, M, TA, A, dtype=dtype)
    assert torch.equal(after, torch.get_rng_state())
    assert all(torch.equal(rec.seen[s * M + m][0][0], want[s, m]) for s in range(S) for m in range(M))


def test_refusals():
    model = lambda state, x, goal, sigma: torch.zeros_like(x)
    x0 = torch.ones(4, TA, A)
    with pytest.raises(ValueError, match="draws is 3"):
        gs.denoising_score(model, {}, x0, None, [1.0], draws=3)
    gs.denoising_score(model, {}, x0, None, [1.0], draws=3, antithetic=False)
    with pytest.raises(ValueError, match="draws must be an int >= 1"):
        gs.denoising_score(model, {}, x0, None, [1.0], draws=0)
    for key in ("cond_lambda", "pin", "probes", "steer"):
        with pytest.raises(NotImplementedError, match=key):
            gs.denoising_score(model, {}, x0, None, [1.0], extra_args={key: 1})
    with pytest.raises(NotImplementedError, match="cond_lambda"):
        gs.denoising_score(model, {}, x0, None, [1.0], extra_args={"candidates": 2, "cond_lambda": 2.0})
    with pytest.raises(ValueError, match="candidates"):  # a foreign model has no shared context
        gs.denoising_score(model, {}, x0, None, [1.0], extra_args={"candidates": 2})
    with pytest.raises(ValueError, match="noise is"):
        gs.denoising_score(model, {}, x0, None, [1.0, 0.5], noise=torch.zeros(3, 2, TA, A))
    with pytest.raises(ValueError, match="at least one level"):
        gs.denoising_score(model, {}, x0, None, [])


def test_both_action_layouts():
    s2 = 0.25
    model = lambda state, x, goal, sigma: x * (s2 / (s2 + sigma ** 2)).reshape(-1, 1, 1)
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(6, TA, A, dtype=torch.float64, generator=g)
    noise = torch.randn(2, 2, TA, A, dtype=torch.float64, generator=g)
    flat = gs.denoising_score(model, {}, x0, None, [2.0, 0.1], noise=noise)
    grid = gs.denoising_score(model, {}, x0.reshape(2, 3, TA, A), None, [2.0, 0.1], noise=noise)
    assert tuple(flat.shape) == (6,) and tuple(grid.shape) == (2, 3)
    assert torch.equal(flat.reshape(2, 3), grid)
    best, index = gs.best_candidates(x0, grid, 3)
    assert torch.equal(index, grid.argmax(1)) and torch.equal(best, x0.reshape(2, 3, TA, A)[torch.arange(2), index])


# ---- the mixture toy -----------------------------------------------------------------------------------------------------------
MU, SC, E = 0.6, 0.3, TA * A


def mixture_denoiser(state, x, goal, sigma):
    """The posterior mean of x0 given x = x0 + sigma n for x0 ~ 1/2 N(+MU 1, SC^2 I) + 1/2 N(-MU 1, SC^2 I)."""
    v = (SC ** 2 + sigma ** 2).reshape(-1, 1, 1)
    # log responsibilities: -|x -+ MU|^2 / (2 v); their difference is 2 MU sum(x) / v
    t = 2 * MU * x.flatten(1).sum(1).reshape(-1, 1, 1) / v
    r_plus = torch.sigmoid(t)
    mean = (2 * r_plus - 1) * MU
    return mean + SC ** 2 / v * (x - mean)


def mixture_log_p(x0):
    d_plus = ((x0 - MU) ** 2).flatten(1).sum(1)
    d_minus = ((x0 + MU) ** 2).flatten(1).sum(1)
    return torch.logsumexp(torch.stack((-d_plus, -d_minus)) / (2 * SC ** 2), 0) - math.log(2) - E / 2 * math.log(2 * math.pi * SC ** 2)


def spearman(a, b):
    ra, rb = a.argsort().argsort().double(), b.argsort().argsort().double()
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra * rb).sum() / (ra.norm() * rb.norm()))


def mixture_trial(seed, antithetic):
    g = torch.Generator().manual_seed(1000 + seed)
    sign = torch.randint(0, 2, (8, 1, 1), generator=g).double() * 2 - 1
    x0 = sign * MU + SC * torch.randn(8, TA, A, dtype=torch.float64, generator=g)
    x0[3] *= 0.5  # one candidate off the data: halfway to the saddle between the components
    torch.manual_seed(seed)
    score = gs.denoising_score(mixture_denoiser, {}, x0, None, LEVELS16, draws=2, antithetic=antithetic)
    return spearman(score, mixture_log_p(x0))


def test_the_score_ranks_mixture_candidates_like_the_exact_log_p():
    """16 levels log-uniform in [0.001, 80], 2 draws, 8 candidates, 20 fixed seeds, the exact denoiser: mean Spearman against the
    exact log p of at least 0.9 with antithetic pairs, and lower without them."""
    paired = [mixture_trial(seed, True) for seed in range(20)]
    plain = [mixture_trial(seed, False) for seed in range(20)]
    print(f"mean Spearman over 20 seeds: antithetic {np.mean(paired):.4f} (min {min(paired):.4f}), independent {np.mean(plain):.4f}")
    assert np.mean(paired) >= 0.9
    assert np.mean(plain) < np.mean(paired)
