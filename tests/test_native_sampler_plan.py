"""The sampler plans behind mdt_sample (CPU tier): mdt_sampler_plan's evaluation sigmas and coefficient table, applied in
numpy with a closed-form toy denoiser, against the gc_sampling host loop driving the same toy model -- every routed sampler,
exponential / karras / linear / vp schedules, 1..20 steps, s_churn, eta in {0, 1} with given noise, LMS orders 1..4 -- and
the plan's noise-draw count against the loop's use of the generator."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.steer_ops_cases import apply_plan as interpret_plan

B, TA, A = 2, 3, 4
NREG = _lib.SAMPLER_NREG


def toy(x, s):
    """D(x; sigma) = a(sigma) x + b(sigma), numpy float64."""
    return x / (1 + s * s) + 0.3 * (s / (1 + s)) * np.sin(np.arange(A))


def toy_model(state, x, goal, sigma):
    """The same denoiser as the host loops call it: sigma a (B,) tensor."""
    s = sigma.to(x.dtype).reshape(-1, 1, 1)
    return x / (1 + s * s) + 0.3 * (s / (1 + s)) * torch.sin(torch.arange(A, dtype=x.dtype))


def schedule(name, n):
    if name == "exp":
        return gs.get_sigmas_exponential(n, 0.001, 80.0)
    if name == "karras":
        return gs.get_sigmas_karras(n, 0.01, 80.0)
    if name == "linear":
        return gs.get_sigmas_linear(n, 0.002, 20.0)
    return gs.get_sigmas_vp(n)


def apply_plan(plan, x_T, noise):
    """The plan kernels' per-element update in float64 (tests/steer_ops_cases.apply_plan, shared with the steered plan tests) around
    the toy denoiser."""
    return interpret_plan(plan, x_T, noise, lambda y, s, k: toy(y, s))[0]


class _Recorder:
    """A noise_sampler that hands out seeded Gaussian rows and records them (dpmpp_2s_ancestral / dpmpp_sde)."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.rows = []

    def __call__(self, s0, s1):
        z = torch.randn((B, TA, A), generator=self.g, dtype=torch.float64)
        self.rows.append(z.numpy())
        return z


CASES = [
    ("euler", {}), ("euler", dict(s_churn=0.8, s_tmin=0.05, s_tmax=50.0, s_noise=1.003)),
    ("heun", {}), ("heun", dict(s_churn=1.0, s_noise=0.9)),
    ("dpm_2", {}), ("dpm_2", dict(s_churn=0.5)),
    ("euler_ancestral", dict(eta=0.)), ("euler_ancestral", dict(eta=1.)),
    ("dpm_2_ancestral", dict(eta=0.)), ("dpm_2_ancestral", dict(eta=1.)),
    ("dpmpp_2s_ancestral", dict(eta=0.)), ("dpmpp_2s_ancestral", dict(eta=1., s_noise=0.8)),
    ("dpmpp_2m", {}), ("dpmpp_2_with_lms", {}), ("dpmpp_2s", {}),
    ("lms", dict(order=1)), ("lms", dict(order=2)), ("lms", dict(order=3)), ("lms", dict(order=4)),
    ("dpmpp_sde", dict(eta=0.)), ("dpmpp_sde", dict(eta=1.)), ("dpmpp_sde", dict(eta=0.7, s_noise=1.1, r=0.4)),
]


@pytest.mark.parametrize("sched", ["exp", "karras", "linear", "vp"])
@pytest.mark.parametrize("n", [1, 3, 5, 10, 20])
@pytest.mark.parametrize("name,kw", CASES, ids=[f"{c[0]}-{'-'.join(f'{k}{v}' for k, v in c[1].items()) or 'default'}"
                                                for c in CASES])
def test_plan_applied_with_a_toy_denoiser_matches_the_host_loop(name, kw, n, sched):
    sig = schedule(sched, n)
    x_T = torch.from_numpy(np.random.default_rng(n).standard_normal((B, TA, A))) * float(sig[0])
    fn = getattr(gs, "sample_" + name)
    ns_kind = name in ("dpmpp_2s_ancestral", "dpmpp_sde")

    # host loop (float64 actions; its schedule scalars are fp32 as always), generator seeded
    torch.manual_seed(1234)
    rec = _Recorder(99)
    extra = dict(noise_sampler=rec) if ns_kind else {}
    want = fn(toy_model, {}, x_T.clone(), None, sig, **kw, **extra).numpy()
    after_loop = torch.randn(3)

    plan = _lib.sampler_plan(name, sig.tolist(), **{k: v for k, v in kw.items()})
    # the plan's noise rows: the loop's randn_like draws in order, or the noise_sampler's values
    torch.manual_seed(1234)
    if ns_kind:
        rows = rec.rows
        assert len(rows) == plan.n_noise, (len(rows), plan.n_noise)
    else:
        rows = [torch.randn_like(x_T).numpy() for _ in range(plan.n_noise)]
        assert torch.equal(torch.randn(3), after_loop), "the plan's draw count differs from the host loop's"
    noise = np.stack(rows) if rows else np.zeros((1, B, TA, A))
    got = apply_plan(plan, x_T.numpy(), noise)
    scale = float(np.abs(x_T.numpy()).max())
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6 * scale)
    # per-evaluation draw bookkeeping adds up to the total
    assert plan.y0_draws + sum(plan.e[k].draws for k in range(plan.n_evals)) == plan.n_noise


@pytest.mark.parametrize("name,evals", [("euler", lambda n: n), ("heun", lambda n: 2 * n - 1), ("lms", lambda n: n),
                                        ("dpmpp_sde", lambda n: 2 * n - 1)])
def test_plan_structure_depends_on_kind_and_steps_only(name, evals):
    for n in (1, 7, 64):
        a = _lib.sampler_plan(name, gs.get_sigmas_exponential(n, 0.001, 80.0).tolist())
        b = _lib.sampler_plan(name, gs.get_sigmas_karras(n, 0.03, 14.0).tolist())
        assert a.n_evals == b.n_evals == evals(n) and a.n_noise == b.n_noise
        assert [list(a.e[k].noise) for k in range(a.n_evals)] == [list(b.e[k].noise) for k in range(b.n_evals)]


def test_plan_rejects_bad_arguments():
    sig = gs.get_sigmas_exponential(3, 0.001, 80.0).tolist()
    with pytest.raises(_lib.MDTHipError):
        _lib.sampler_plan(42, sig)
    with pytest.raises(_lib.MDTHipError):
        _lib.sampler_plan("lms", sig, order=5)
    with pytest.raises(_lib.MDTHipError):
        _lib.sampler_plan("euler", gs.get_sigmas_exponential(65, 0.001, 80.0).tolist())
