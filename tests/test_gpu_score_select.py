"""k_score_select through its hook mdt_op_score_select on the MI355X (pytest -m gpu): every operand between guard bands
(tests/guarded.py), index and best equal to the float64 restatement of the rule (tests/select_cases.py) exactly.

Shapes (B, K, E): (1, 1, 1); (1, 8, 70), the rollout's; (3, 5, 70), more than one workgroup; (2, 65, 70), K no multiple of a wave;
(1, 300, 7), K beyond the workgroup's 256 lanes (a second trip of the lane scan); (1, 2, 4096), Ta = A = 64 (sixteen trips of the
copy).  Every pattern of select_cases.patterns(K) -- ties at the first, middle and last k and across lanes 63 | 64 and 255 | 256,
one NaN, all NaN, -Inf beside NaN, +Inf, +Inf against FLT_MAX -- is one observation: the shape's B at a time, and all of them
as the observations of one launch."""
import numpy as np
import pytest
import torch

from mdt_policy_amd import _lib
from tests import select_cases as sc
from tests.guarded import GuardedSet, same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 8, 70), (3, 5, 70), (2, 65, 70), (1, 300, 7), (1, 2, 4096)]


def launch(scores, chunks, B, K, E, finite=True):
    """(best (B, E), index (B,) int32) of one launch between guard bands; the inputs keep their bits, nothing else is written."""
    gset = GuardedSet()
    s = gset.inp("scores", torch.from_numpy(scores).reshape(1, B * K))
    c = gset.inp("chunks", torch.from_numpy(chunks).reshape(B * K, E))
    best = gset.out("best", B, E)
    index = gset.out("index", 1, B)
    _lib.call(_lib.load().mdt_op_score_select, s.ptr, c.ptr, B, K, E, best.ptr, index.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gset.check(f"mdt_op_score_select B={B} K={K} E={E}")
    best.check("best", written=finite)
    return best.region.clone(), index.region.contiguous().view(torch.int32).reshape(-1).clone()


def check(scores, chunks, names, B, K, E):
    best, index = launch(scores, chunks, B, K, E)
    want_index, want_best = sc.select(scores, chunks, K)
    for b in range(B):
        assert int(index[b]) == int(want_index[b]), (names[b], (B, K, E), scores.reshape(B, K)[b].tolist(), int(index[b]))
    assert same_bits(best.cpu(), torch.from_numpy(np.ascontiguousarray(want_best)))
    return best, index


@pytest.mark.parametrize("B,K,E", SHAPES)
def test_index_and_best_are_the_float64_rule_exactly(B, K, E):
    cases = sc.patterns(K)
    rng = np.random.default_rng(5 + K + E)
    P = len(cases)
    chunks = rng.standard_normal((P * K, E)).astype(np.float32)
    scores = np.stack([s for _, s, _ in cases])
    names = [n for n, _, _ in cases]
    for at in range(0, P, B):   # the shape's own B observations at a time (the last group wraps round)
        rows = [(at + i) % P for i in range(B)]
        check(scores[rows].reshape(-1), chunks.reshape(P, K, E)[rows].reshape(B * K, E), [names[r] for r in rows], B, K, E)
    check(scores.reshape(-1), chunks, names, P, K, E)   # and all of them at once: one workgroup each


@pytest.mark.parametrize("B,K,E", [(3, 5, 70), (1, 300, 7)])
def test_two_runs_give_the_same_bits(B, K, E):
    cases = sc.patterns(K)[:B]
    rng = np.random.default_rng(9)
    chunks = rng.standard_normal((B * K, E)).astype(np.float32)
    scores = np.stack([s for _, s, _ in cases]).reshape(-1)
    a, b = launch(scores, chunks, B, K, E), launch(scores, chunks, B, K, E)
    assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_nan_in_the_winning_chunk_is_copied_as_it_is():
    B, K, E = 1, 3, 70
    chunks = np.random.default_rng(1).standard_normal((K, E)).astype(np.float32)
    chunks[1, 5] = np.nan
    chunks[1, 6] = np.inf
    best, index = launch(np.array([0.0, 2.0, 1.0], np.float32), chunks, B, K, E, finite=False)
    assert int(index[0]) == 1 and same_bits(best.cpu(), torch.from_numpy(chunks[1:2]))
