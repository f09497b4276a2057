"""CPU tier of the module envelope (tests/envelope_configs.py RESAMPLER_ENVELOPE / MAP_ENVELOPE): the two oracles the GPU
tier compares against are pinned to the REFERENCE's own outputs and gradients at these shapes (tests/golden/g18_*.npz, written
by tests/golden/make_golden.py g18), and the tables are checked against the documented LDS budgets they claim to sit on."""
import pytest
import torch

from oracle import cla_oracle as CO
from oracle import perceiver_oracle as PO
from tests import envelope_configs as E
from tests.helpers import assert_close, check_grad_summaries, map_envelope_fixture, resampler_envelope_fixture


@pytest.mark.parametrize("name", sorted(E.RESAMPLER_GOLDEN))
def test_perceiver_oracle_matches_the_reference_at_the_envelope(name):
    meta, fx, P, x, mask, cot = resampler_envelope_fixture(name)
    assert meta["kwargs"] == E.RESAMPLER_ENVELOPE[name]["kwargs"] and meta["B"] == E.RESAMPLER_GOLDEN[name]
    assert meta["mask"] == E.resampler_mask(E.RESAMPLER_ENVELOPE[name]["mask"], meta["B"], meta["T"])
    heads = meta["kwargs"]["heads"]
    assert_close(PO.perceiver_resampler(P, x, heads, mask), fx["out"], rtol=1e-4, atol=2e-5, what=name)
    P64 = {k: v.double().requires_grad_() for k, v in P.items()}
    x64 = x.double().requires_grad_()
    out = PO.perceiver_resampler(P64, x64, heads, mask)
    assert_close(out.detach(), fx["out"], rtol=1e-4, atol=2e-5, what=name + " float64")
    (out * cot.double()).sum().backward()
    check_grad_summaries({k: v.grad for k, v in P64.items()}, meta["grads"], name)
    dx = x64.grad
    assert_close(dx[:, :, :4, :], fx["d_x_head"], rtol=2e-3, atol=2e-3 * float(abs(fx["d_x_head"]).max()), what=name + " d_x_f")
    assert abs(float(dx.norm()) - meta["d_x_summary"][0]) <= 2e-3 * meta["d_x_summary"][0]
    assert abs(float(dx.sum()) - meta["d_x_summary"][1]) <= 2e-3 * meta["d_x_summary"][0]


@pytest.mark.parametrize("name", sorted(E.MAP_GOLDEN))
def test_map_block_oracle_matches_the_reference_at_the_envelope(name):
    meta, fx, P, x, cot = map_envelope_fixture(name)
    assert meta["kwargs"] == E.MAP_ENVELOPE[name]["kwargs"] and meta["N"] == E.MAP_ENVELOPE[name]["N"]
    nh = meta["kwargs"]["n_heads"]
    assert_close(CO.map_block(P, "", x, nh), fx["out"], rtol=1e-4, atol=2e-5, what=name)
    P64 = {k: v.double().requires_grad_() for k, v in P.items()}
    x64 = x.double().requires_grad_()
    out = CO.map_block(P64, "", x64, nh)
    assert tuple(out.shape) == (meta["B"], meta["kwargs"]["n_latents"], meta["kwargs"]["output_dim"])  # no squeeze
    (out * cot.double()).sum().backward()
    check_grad_summaries({k: v.grad for k, v in P64.items()}, meta["grads"], name)
    assert_close(x64.grad, fx["d_x"], rtol=2e-3, atol=2e-3 * float(abs(fx["d_x"]).max()), what=name + " d_x")


def test_the_golden_subsets_cover_what_they_must():
    R = [E.RESAMPLER_ENVELOPE[n] for n in E.RESAMPLER_GOLDEN]
    assert len(R) >= 4 and any(c["mask"] and c["T"] > 1 for c in R)
    assert any(c["kwargs"]["heads"] * c["kwargs"]["dim_head"] < c["kwargs"]["dim"] for c in R)
    M = [E.MAP_ENVELOPE[n]["kwargs"] for n in E.MAP_GOLDEN]
    assert len(M) >= 4 and any(k["n_latents"] > 1 for k in M) and any(k["embed_dim"] != k["output_dim"] for k in M)


def _keys(c):
    return c["T"] * c["n"] + c["kwargs"]["num_latents"]


def test_resampler_table_sits_on_the_documented_lds_budget():
    """160 KiB per workgroup with the buffers include/mdt_resampler.h lists: what each case's infer / train flag claims."""
    for name, c in E.RESAMPLER_ENVELOPE.items():
        kw = c["kwargs"]
        for train in (False, True):
            fits = E.resampler_lds_bytes(kw["num_latents"], kw["dim_head"], _keys(c), train) <= E.RESAMPLER_LDS_BUDGET
            assert fits == c["train" if train else "infer"], (name, train)
        assert _keys(c) <= 4096
    lds = lambda name, train: E.resampler_lds_bytes(16, 64, _keys(E.RESAMPLER_ENVELOPE[name]), train)
    # the boundaries the header quotes for 16 latents at dim_head 64
    assert [_keys(E.RESAMPLER_ENVELOPE[n]) for n in ("r_wide_k2236_infer_edge", "r_wide_k2237_refused", "r_wide_k1084_train_edge",
                                                     "r_wide_k1085_infer_only")] == [2236, 2237, 1084, 1085]
    assert lds("r_wide_k2236_infer_edge", False) <= 160 * 1024 < lds("r_wide_k2237_refused", False)
    assert lds("r_wide_k1084_train_edge", True) <= 160 * 1024 < lds("r_wide_k1085_infer_only", True)
    # which cases take the raised (> 64 KiB) dynamic limit
    c = E.RESAMPLER_ENVELOPE["r_lds_k1000"]
    assert E.resampler_lds_bytes(16, 64, _keys(c), False) > 64 * 1024
    c = E.RESAMPLER_ENVELOPE["r_q3_k4096"]
    assert _keys(c) == 4096
    assert E.resampler_lds_bytes(3, 64, 4096, False) <= 64 * 1024 < E.resampler_lds_bytes(3, 64, 4096, True) <= 160 * 1024
    assert sorted({_keys(c) % 4 for c in E.RESAMPLER_ENVELOPE.values() if c["kwargs"]["num_latents"] == 16}) == [0, 1, 2, 3]


def test_map_table_sits_on_the_documented_lds_budget():
    for name, c in E.MAP_ENVELOPE.items():
        kw = c["kwargs"]
        for train in (False, True):
            fits = E.map_lds_bytes(kw["n_latents"], kw["output_dim"], kw["n_heads"], c["N"], train) <= E.MAP_LDS_BUDGET
            assert fits == c["train" if train else "infer"], (name, train)
        assert int(kw["mlp_ratio"] * kw["output_dim"]) % 16 == 0
    assert E.map_lds_bytes(16, 256, 8, 16, False) == 65536
