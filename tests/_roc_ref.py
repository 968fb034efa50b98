"""numpy statement of the weighted ROC counts (include/advhip.h: advhip_roc_counts), written from the definition: items (score,
pos, neg) sorted by a uint32 key whose ascending order is the floats' descending one (-0.0 folded onto +0.0 first), equal keys
merged, the weights accumulated as int64.  tests/test_auc_host.py holds it to metrics._ranked on the expanded frames; the GPU
tests import it as the truth where the expansion is too large to build (weights of 2^30)."""
import numpy as np


def keys(scores) -> np.ndarray:
    u = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0  # -0.0 == +0.0
    asc = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~asc


def weighted_counts(scores, pos, neg):
    """-> (thresholds fp32 (G,), tps int64 (G,), fps int64 (G,))"""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    k = keys(s)
    order = np.argsort(k, kind="stable")
    k = k[order]
    end = np.concatenate([k[1:] != k[:-1], [True]])
    tps = np.cumsum(np.asarray(pos, dtype=np.int64)[order])[end]
    fps = np.cumsum(np.asarray(neg, dtype=np.int64)[order])[end]
    return s[order][end], tps, fps


def expand(scores, pos, neg):
    """(labels, preds) of the frames the items stand for: item i as pos[i] frames of label 1 and neg[i] of label 0, all scored
    scores[i] -- np.repeat(scores, w) with the matching labels."""
    pos, neg = np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)
    w = pos + neg
    preds = np.repeat(np.asarray(scores, dtype=np.float32), w)
    within = np.arange(int(w.sum())) - np.repeat(np.cumsum(w) - w, w)
    return (within < np.repeat(pos, w)).astype(np.float32), preds


def distinct_descending(scores) -> np.ndarray:
    """The distinct scores, largest first (np.unique: -0.0 and +0.0 are one value), without the key mapping."""
    return np.unique(np.asarray(scores, dtype=np.float32).astype(np.float64))[::-1].astype(np.float32)


def same_thresholds(got, want) -> bool:
    """Equal as bits, except that a zero may carry either sign."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    return bool(np.all((gb == wb) | ((got == 0) & (want == 0))))


def case(m: int, seed: int, kind: str = "mixed", wmax: int = 5):
    """(scores, pos, neg) of m items with pos + neg >= 1.  kind: "mixed" (about half the scores repeat), "equal", "distinct",
    "eighths" (scores rounded to eighths: long tie runs)."""
    rng = np.random.default_rng(seed)
    if kind == "equal":
        scores = np.full(m, 0.375, np.float32)
    elif kind == "distinct":
        scores = rng.permutation(m).astype(np.float32) / np.float32(max(m, 1)) - np.float32(0.25)
    elif kind == "eighths":
        scores = (np.round(rng.random(m) * 8) / 8).astype(np.float32)
    else:
        pool = rng.standard_normal(m // 2 + 1).astype(np.float32)
        scores = pool[rng.integers(0, pool.size, m)]
    pos = rng.integers(0, wmax + 1, m).astype(np.int32)
    neg = rng.integers(0, wmax + 1, m).astype(np.int32)
    neg[(pos == 0) & (neg == 0)] = 1
    return scores, pos, neg
