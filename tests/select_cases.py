"""The selection rule of mdt_sample*_select / k_score_select restated in float64, and the score patterns its tests use
(tests/test_cpu_select_abi.py against gc_sampling.best_candidates; tests/test_gpu_score_select.py against the kernel).

The rule, as include/mdt_hip.h states it: per observation the largest score wins, ties go to the lowest k, a NaN score loses to
every other, -Inf included, and K NaN scores select 0.  It is best_candidates' rule, whose torch.nan_to_num(scores, nan=-inf)
also reads +Inf as the largest finite float32 and -Inf as the lowest: +Inf ties with FLT_MAX, which the patterns include."""
import math

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
NAN, INF = float("nan"), float("inf")


def select_key(v):
    v = float(v)
    return -INF if math.isnan(v) else min(max(v, -F32_MAX), F32_MAX)


def select_index(scores):
    """The k the rule selects among one observation's scores."""
    keys = [select_key(v) for v in scores]
    return keys.index(max(keys))


def select(scores, chunks, K):
    """(index (B,) int64, best (B, E)) of float32 scores (B K) and chunks (B K, E), numpy."""
    sc = np.asarray(scores, dtype=np.float32).reshape(-1, K)
    rows = np.asarray(chunks).reshape(sc.shape[0], K, -1)
    index = np.array([select_index(r.astype(np.float64)) for r in sc], dtype=np.int64)
    return index, rows[np.arange(sc.shape[0]), index]


def anchors(K):
    """Where the patterns put their special values: the first and the last k, the middle, and both sides of a wave boundary
    (lanes 63 | 64) and of the workgroup's stride (255 | 256) where K reaches them."""
    return sorted({k for k in (0, K // 2, K - 1, 63, 64, 255, 256) if 0 <= k < K})


def patterns(K, seed=0):
    """(name, scores (K,) float32, expected index) for one observation: finite background in (-4, 4), the special values at the
    anchors.  Ties at the first, a middle and the last index; one NaN; all NaN; -Inf beside NaN; +Inf; +Inf against FLT_MAX."""
    rng = np.random.default_rng(1000 + 7 * K + seed)
    base = (rng.random(K) * 8 - 4).astype(np.float32)
    out = [("background", base.copy()), ("all nan", np.full(K, NAN, np.float32)),
           ("all equal", np.full(K, 1.5, np.float32)), ("all -inf", np.full(K, -INF, np.float32))]
    at = anchors(K)
    for a in at:
        s = base.copy(); s[a] = 10.0
        out.append((f"max at {a}", s))
        s = base.copy(); s[a] = NAN
        out.append((f"one nan at {a}", s))
        s = np.full(K, NAN, np.float32); s[a] = -INF
        out.append((f"-inf at {a} beside nan", s))
        s = np.full(K, NAN, np.float32); s[a] = -3.0
        out.append((f"one number at {a} beside nan", s))
        s = base.copy(); s[a] = INF
        out.append((f"+inf at {a}", s))
        for b in at:
            if b != a:
                s = base.copy(); s[a] = s[b] = 10.0
                out.append((f"tie at {a} and {b}", s))
                s = base.copy(); s[a] = INF; s[b] = np.float32(F32_MAX)
                out.append((f"+inf at {a}, float max at {b}", s))
                s = base.copy(); s[a] = 10.0; s[b] = NAN
                out.append((f"max at {a}, nan at {b}", s))
    return [(name, s, select_index(s.astype(np.float64))) for name, s in out]
