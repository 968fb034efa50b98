"""CPU-only checks of the count-based AUC tails and of the host side of metrics.FrameAucPlan: the areas from `_ranked`'s counts
are roc_auc / pr_auc themselves, the weighted grouping by uint32 keys (tests/_roc_ref.py, the GPU tests' reference) gives
`_ranked`'s counts on the expanded frames, and FrameAucItems builds the per-window / per-frame counts and refuses a video whose
labels do not fit its windows."""
import numpy as np
import pytest

import _roc_ref as ref
from anomaly_detection_on_video_amd import metrics

SIZES = [1, 2, 257, 4097, 5000, 70001]


def _labels_preds(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(n) < 0.3).astype(np.float32), (np.round(rng.random(n) * 64) / 64).astype(np.float32)


@pytest.mark.parametrize("n", [2, 17, 1000, 50001])
def test_areas_from_counts_are_roc_auc_and_pr_auc(n):
    labels, preds = _labels_preds(n, n)
    labels[:2] = (1.0, 0.0)
    tps, fps = metrics._ranked(labels, preds)
    assert metrics.roc_auc_from_counts(tps, fps) == metrics.roc_auc(labels, preds)
    assert metrics.pr_auc_from_counts(tps, fps) == metrics.pr_auc(labels, preds)
    # integer counts (what the device returns) are the same float64s
    ti, fi = tps.astype(np.int64), fps.astype(np.int64)
    assert np.array_equal(ti, tps) and np.array_equal(fi, fps)
    assert metrics.roc_auc_from_counts(ti, fi) == metrics.roc_auc(labels, preds)
    assert metrics.pr_auc_from_counts(ti, fi) == metrics.pr_auc(labels, preds)


def test_areas_from_counts_one_class_only():
    """All-negative labels: tps[-1] = 0, the host's NaN; all-positive: its value."""
    preds = np.array([0.5, 0.25, 0.5, 0.75], np.float32)
    with np.errstate(all="ignore"):
        for labels in (np.zeros(4, np.float32), np.ones(4, np.float32)):
            tps, fps = metrics._ranked(labels, preds)
            for f, g in ((metrics.roc_auc_from_counts, metrics.roc_auc), (metrics.pr_auc_from_counts, metrics.pr_auc)):
                assert np.array_equal(f(tps, fps), g(labels, preds), equal_nan=True)


def _check_against_ranked(scores, pos, neg):
    labels, preds = ref.expand(scores, pos, neg)
    tps, fps = metrics._ranked(labels, preds)
    thr, wt, wf = ref.weighted_counts(scores, pos, neg)
    assert wt.dtype == np.int64 and wt.shape == tps.shape
    assert np.array_equal(wt, tps) and np.array_equal(wf, fps)
    assert ref.same_thresholds(thr, ref.distinct_descending(scores))


@pytest.mark.parametrize("m", SIZES)
@pytest.mark.parametrize("kind", ["mixed", "eighths"])
def test_weighted_grouping_equals_ranked_on_expanded_frames(m, kind):
    _check_against_ranked(*ref.case(m, m, kind))


def test_weighted_grouping_signed_zeros_denormals_and_neighbours():
    tiny = np.float32(1e-45)
    one = np.float32(1.0)
    scores = np.array([0.0, -0.0, tiny, -tiny, 0.0, -0.0, one, np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0)), -3.5, 7.25,
                       2 * tiny, -0.0], np.float32)
    pos = np.arange(1, scores.size + 1, dtype=np.int32) % 4
    neg = (np.arange(scores.size, dtype=np.int32) % 3) + (pos == 0)
    _check_against_ranked(scores, pos, neg)
    thr, tps, _ = ref.weighted_counts(scores, pos, neg)
    assert thr.size == 9  # five zeros are one group; the denormals and the neighbours of 1.0 stay apart
    k = ref.keys(scores)
    assert k[0] == k[1] and k[2] != k[0] and k[3] != k[0] and k[6] != k[7] and k[6] != k[8]


def test_frame_auc_items_default_stride():
    rng = np.random.default_rng(0)
    windows = [1, 3, 5]
    labels = [(rng.random(n * 16) < 0.4).astype(np.float32) for n in windows]
    it = metrics.FrameAucItems(labels, windows, 16)
    assert not it.per_frame and it.span == it.stride == 16 and it.pos.dtype == it.neg.dtype == np.int32
    assert it.window_offsets.tolist() == [0, 1, 4, 9] and it.frames == [16, 48, 80]
    want = np.concatenate([l.reshape(-1, 16).sum(1) for l in labels])
    assert np.array_equal(it.pos, want) and np.array_equal(it.neg, 16 - want)
    # the items reproduce the host path's counts for any scores
    scores = (np.round(rng.random(9) * 4) / 4).astype(np.float32)
    tps, fps = metrics._ranked(np.concatenate(labels), np.repeat(scores, 16))
    _, wt, wf = ref.weighted_counts(scores, it.pos, it.neg)
    assert np.array_equal(wt, tps) and np.array_equal(wf, fps)
    it2 = metrics.FrameAucItems([np.zeros(n * 32, np.float32) for n in windows], windows, 16, frame_step=2)
    assert it2.span == 32 and not it2.per_frame and np.array_equal(it2.neg, np.full(9, 32))


def test_frame_auc_items_overlapping_windows_and_cut():
    windows = [2, 4]
    labels = [np.ones(8 + 16, np.float32), np.r_[np.zeros(20), np.ones(3 * 8 + 16 - 20 - 5)].astype(np.float32)]  # the second ends 5 short
    it = metrics.FrameAucItems(labels, windows, 16, clip_stride=8)
    assert it.per_frame and it.stride == 8 and it.frames == [24, 35] and it.frame_offsets.tolist() == [0, 24, 59]
    assert np.array_equal(it.pos, np.concatenate(labels).astype(np.int32)) and np.array_equal(it.neg, 1 - it.pos)


def test_frame_auc_items_refusals():
    ok = np.zeros(32, np.float32)
    with pytest.raises(ValueError, match=r"video 1: 31 frame labels.* 2 windows of 16 frames cover 32"):
        metrics.FrameAucItems([ok, ok[:31]], [2, 2], 16)
    with pytest.raises(ValueError, match=r"video 0: 64 frame labels.* cover 32"):  # judged video by video, not by the total
        metrics.FrameAucItems([np.zeros(64, np.float32), ok], [2, 2], 16)
    with pytest.raises(ValueError, match=r"video 0: 8 frame labels"):  # ends before the last window starts
        metrics.FrameAucItems([np.zeros(8, np.float32)], [2], 16, clip_stride=8)
    with pytest.raises(ValueError, match=r"video 0: 25 frame labels"):
        metrics.FrameAucItems([np.zeros(25, np.float32)], [2], 16, clip_stride=8)
    with pytest.raises(ValueError, match="clip_stride 17"):
        metrics.FrameAucItems([ok], [2], 16, clip_stride=17)
    with pytest.raises(ValueError, match="frame_step"):
        metrics.FrameAucItems([ok], [2], 16, frame_step=0)
    with pytest.raises(ValueError, match="1 label arrays for 2 videos"):
        metrics.FrameAucItems([ok], [2, 2], 16)
    with pytest.raises(ValueError, match="video 0: 0 windows"):
        metrics.FrameAucItems([ok], [0], 16)


def test_frame_auc_plan_refuses_the_cpu():
    with pytest.raises(ValueError, match="HIP kernel"):
        metrics.FrameAucPlan([np.zeros(16, np.float32)], [1], 16, device="cpu")
