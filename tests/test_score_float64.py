"""The algebra mdt_denoising_score's reduction uses, pinned in float64 on the host: over the oracle network of the log-likelihood
fixtures (tests.test_log_likelihood.OracleModel), the score in the residual form -- q from the raw network output F, with no
subtraction x0 - D (tests/score_oracle.py) -- equals the definition's D form, q = (x0 - D(x0 + sigma n; sigma)) / sigma, which
gc_sampling.denoising_score's host loop evaluates, to 1e-9 relative.  Levels from sigma_min = 0.001 to sigma_max = 80: in float64
the D form's cancellation at the small end costs 1e-16 / 1e-3, far inside that."""
import pytest
import torch

from mdt_policy_amd import synthetic
from mdt_policy_amd.models.edm_diffusion import gc_sampling as gs
from tests.score_oracle import residual_score, trapezoid
from tests.test_log_likelihood import OracleModel, case

LEVELS = [80.0, 9.0, 1.1, 0.13, 0.015, 0.001]


@pytest.mark.parametrize("weights", [None, [0.5, 0.0, 2.0, 1.0, 0.25, 3.0]], ids=["trapezoid", "given"])
@pytest.mark.parametrize("name", ["mdtv_tiny", "mdt_tiny"])
def test_the_residual_form_is_the_definition(name, weights):
    meta, _, cfg, state, goal, action = case(name)
    model = OracleModel(meta, cfg, torch.float64)
    noise = torch.from_numpy(synthetic.normal("score_noise", (len(LEVELS), 2) + tuple(action.shape[1:]), 23)).double()
    d_form = gs.denoising_score(model, state, action.double(), goal, LEVELS, noise=noise, weights=weights)
    res, terms = residual_score(model.P, cfg, meta["arch"], state, goal, action, LEVELS, noise, weights=weights)
    assert d_form.dtype == torch.float64 and res.dtype == torch.float64 and tuple(d_form.shape) == (action.shape[0],)
    rel = ((d_form - res).abs() / res.abs()).max()
    print(f"{name}: residual against D form, largest relative difference {float(rel):.3e}; scores {res.tolist()}")
    assert float(rel) <= 1e-9
    assert torch.equal(terms, -res) and bool((res < 0).all())
    if weights is None:  # the helper's default weights are the ones the package forms
        assert gs._score_levels(LEVELS, None)[1] == pytest.approx(trapezoid(LEVELS), rel=1e-15)
