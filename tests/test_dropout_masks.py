"""tests/dropout_masks.py on the CPU: the vectorised Philox against a scalar one written with Python integers, the keep rate
of ``scale``, and the site numbering."""
import numpy as np
import pytest

from mdt_policy_amd import configs
from tests import dropout_masks as DM


def philox4_scalar(seed, site, ctr):
    """Philox4x32-10 (Salmon et al., SC'11) with Python integers, laid out as csrc/mdt_device.h lays it out."""
    m = 0xFFFFFFFF
    c0, c1, c2, c3 = ctr & m, (ctr >> 32) & m, site & m, 0x9E3779B9
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & m, (p0 >> 32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    return c0, c1, c2, c3


def test_vectorised_philox_equals_the_scalar_one():
    rng = np.random.default_rng(3)
    ctrs = np.concatenate([np.arange(100, dtype=np.uint64), rng.integers(0, 2 ** 32, 100, dtype=np.uint64),
                           rng.integers(2 ** 32, 2 ** 63, 100, dtype=np.uint64),
                           np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 64 - 1], dtype=np.uint64)])
    for seed in (1, 987654321, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 12345, 2 ** 62 - 1, 2 ** 63 + 5):
        for site in (1, 5, 82, 2 ** 32 - 1):
            got = np.stack(DM.philox4(seed, site, ctrs), axis=1)
            want = np.array([philox4_scalar(seed, site, int(c)) for c in ctrs], dtype=np.uint64)
            assert np.array_equal(got, want), (seed, site)
    # arrays of sites against one counter (the Brownian tree's use)
    sites = np.arange(300, dtype=np.uint64)
    got = np.stack(DM.philox4(2 ** 41 + 7, sites, 2 ** 35 + 3), axis=1)
    assert np.array_equal(got, np.array([philox4_scalar(2 ** 41 + 7, int(s), 2 ** 35 + 3) for s in sites], dtype=np.uint64))


def test_words_take_word_e_and_3_of_block_e_shift_2():
    seed, site = 2 ** 33 + 11, 19
    idx = np.array([[0, 1, 2, 3], [4, 7, 2 ** 34 + 1, 2 ** 34 + 2], [13, 12, 5, 5]], dtype=np.uint64)
    got = DM.words(seed, site, idx)
    for e, w in zip(idx.reshape(-1), got.reshape(-1)):
        assert int(w) == philox4_scalar(seed, site, int(e) >> 2)[int(e) & 3]
    # a whole site (shape) and the same elements by index give the same multipliers; ragged tail (n % 4 != 0) included
    for shape in ((3, 7, 30), (2, 5, 3, 3), 11):
        n = int(np.prod(shape))
        a = DM.scale(seed, site, shape, 0.3)
        b = DM.scale(seed, site, np.arange(n).reshape(a.shape), 0.3)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("p", [0.05, 0.1, 0.3])
def test_scale_keeps_one_minus_p(p):
    n = 1 << 20
    m = DM.scale(123456789, 5, (n,), p)
    vals = np.unique(m)
    assert np.array_equal(vals, np.array([0.0, 1.0 / (1.0 - float(np.float32(p)))]))
    assert abs((m > 0).mean() - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5     # binomial, 5 sigma
    other = DM.scale(123456789, 6, (n,), p)
    assert abs(((m > 0) == (other > 0)).mean() - ((1 - p) ** 2 + p ** 2)) < 0.01   # another site: an independent mask


def test_scale_without_dropout_is_one():
    assert np.array_equal(DM.scale(77, 3, (4, 5), 0.0), np.ones((4, 5)))
    assert np.array_equal(DM.scale(0, 3, (4, 5), 0.3), np.ones((4, 5)))
    assert np.array_equal(DM.scale(0, 3, np.arange(6), 0.3), np.ones(6))


@pytest.mark.parametrize("Le,Ld", [(configs.mdt_default()["n_enc_layers"], configs.mdt_default()["n_dec_layers"]), (0, 1), (24, 24)])
def test_site_ids_are_distinct(Le, Ld):
    ids = [DM.site_id(b, pl) for b in range(Le) for pl in (DM.ATTN, DM.RESID, DM.MLP)]
    ids += [DM.site_id(Le + b, pl) for b in range(Ld) for pl in DM.PLACES.values()]
    ids += [DM.site_id(Le + Ld, DM.EMBED_CTX), DM.site_id(Le + Ld, DM.EMBED_ACTION)]
    assert len(set(ids)) == len(ids) and min(ids) >= 1 and max(ids) < 2 ** 32


def test_masks_layouts():
    mk = DM.Masks(2 ** 40 + 3, 1, 2, 4, 32, 0.3, 0.1, 0.05, 0.1)
    a = mk.attn(0, 3, 10, 4)
    assert tuple(a.shape) == (3, 4, 10, 4)
    b, h, i, j = 2, 3, 7, 1
    e = ((b * 4 + h) * 10 + i) * 4 + j
    assert float(a[b, h, i, j]) == float(DM.scale(mk.seed, DM.site_id(0, DM.ATTN), np.array([e]), 0.3)[0])
    assert not np.array_equal(mk.resid(1, 3, 10).numpy(), mk.xresid(1, 3, 10).numpy())
    c = mk.embed_ctx(3, 4, 1)
    assert tuple(c.shape) == (3, 4, 32) and bool((c[:, 0] == 1).all()) and bool((c[:, 1:] == 0).any())
    full = DM.scale(mk.seed, DM.site_id(3, DM.EMBED_CTX), (3, 4, 32), 0.1)
    assert np.array_equal(c[:, 1:].numpy(), full[:, 1:])                    # the rows keep their own flat index
    assert tuple(mk.embed_action(3, 10).shape) == (3, 10, 32)
