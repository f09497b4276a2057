"""CPU tier of the MAP block at 17 .. 64 tokens (tests/map_long_configs.py): the float64 oracle the GPU tier compares against
(oracle/cla_oracle.map_block) is pinned to the REFERENCE's own outputs and gradients at these shapes
(tests/golden/g22_map_long_<name>.npz, written by tests/golden/make_golden_map_long.py).  Gates: those of
tests/test_module_envelope.py for the g18 MAP fixtures."""
import pytest
import torch

from oracle import cla_oracle as CO
from tests import map_long_configs as L
from tests.helpers import assert_close, check_grad_summaries
from tests.map_long_configs import map_long_fixture


@pytest.mark.parametrize("name", sorted(L.MAP_LONG_GOLDEN))
def test_map_block_oracle_matches_the_reference_above_16_tokens(name):
    meta, fx, P, x, cot = map_long_fixture(name)
    c = L.MAP_LONG[name]
    assert meta["kwargs"] == c["kwargs"] and meta["N"] == c["N"] > 16 and meta["B"] == L.MAP_LONG_GOLDEN[name]
    assert (meta["weight_seed"], meta["input_seed"], meta["cot_seed"]) == (L.WEIGHT_SEED, L.INPUT_SEED, L.COT_SEED)
    nh, Q, D = c["kwargs"]["n_heads"], c["kwargs"]["n_latents"], c["kwargs"]["output_dim"]
    shape = (meta["B"], D) if Q == 1 else (meta["B"], Q, D)   # the reference squeezes dim 1 of a single latent, and so does the oracle
    assert fx["out"].shape == shape
    assert_close(CO.map_block(P, "", x, nh), fx["out"], rtol=1e-4, atol=2e-5, what=name)
    P64 = {k: v.double().requires_grad_() for k, v in P.items()}
    x64 = x.double().requires_grad_()
    out = CO.map_block(P64, "", x64, nh)
    assert tuple(out.shape) == shape
    (out * cot.double()).sum().backward()
    check_grad_summaries({k: v.grad for k, v in P64.items()}, meta["grads"], name)
    assert_close(x64.grad, fx["d_x"], rtol=2e-3, atol=2e-3 * float(abs(fx["d_x"]).max()), what=name + " d_x")


def test_the_fixtures_cover_the_table_and_stay_small():
    import os

    from tests.helpers import GOLDEN
    assert set(L.MAP_LONG_GOLDEN) == set(L.MAP_LONG) - {"clip_n18"}
    for name in L.MAP_LONG_GOLDEN:
        assert os.path.getsize(os.path.join(GOLDEN, f"g22_map_long_{name}.npz")) <= 140 * 1024, name
