"""GPU tests of the weighted ROC counts (mil_ops.roc_counts, include/advhip.h: advhip_roc_counts) and of the frame-level AUC built
on them (metrics.FrameAucPlan / frame_level_auc_device).  The truth is metrics._ranked on the expanded frames
(np.repeat(scores, w) with the matching labels): tps / fps / G equal exactly, thresholds equal as bits except that a zero may
carry either sign.  Nothing is compared with a tolerance: the device returns integers and copied floats, the areas are the
host's float64 arithmetic on them.

Sizes: the wave (64), the workgroup's round (256), the scan tile (1024), the radix tile (2048), the largest size whose
(digit, tile) table is scanned by one workgroup (8192), a three-launch scan of the counts (70 001) and its five-launch form,
partials of partials (2^20 + 3 > 1024^2)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _roc_ref as ref
from anomaly_detection_on_video_amd import metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device_counts(scores, pos, neg, **kw):
    from anomaly_detection_on_video_amd import mil_ops

    out = mil_ops.roc_counts(torch.from_numpy(scores).to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(neg).to(DEV), **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == out[2].dtype == torch.int64 and all(t.is_cuda for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _check(scores, pos, neg):
    thr, tps, fps = _device_counts(scores, pos, neg)
    labels, preds = ref.expand(scores, pos, neg)
    want_tps, want_fps = metrics._ranked(labels, preds)
    print(f"M={scores.size} G={tps.size} (truth {want_tps.size}) frames={labels.size}")
    assert tps.shape == fps.shape == thr.shape == want_tps.shape
    assert np.array_equal(tps, want_tps.astype(np.int64)) and np.array_equal(fps, want_fps.astype(np.int64))
    assert ref.same_thresholds(thr, ref.distinct_descending(scores))
    with np.errstate(all="ignore"):
        assert np.array_equal(metrics.roc_auc_from_counts(tps, fps), metrics.roc_auc(labels, preds), equal_nan=True)
        assert np.array_equal(metrics.pr_auc_from_counts(tps, fps), metrics.pr_auc(labels, preds), equal_nan=True)
    return thr, tps, fps


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 8192, 8193, 70001])
def test_counts_equal_ranked_on_expanded_frames(m):
    _check(*ref.case(m, m))


def test_counts_two_equal_and_two_distinct():
    one = np.array([3, 0], np.int32), np.array([0, 2], np.int32)
    thr, tps, fps = _check(np.array([0.5, 0.5], np.float32), *one)
    assert thr.tolist() == [0.5] and tps.tolist() == [3] and fps.tolist() == [2]
    thr, tps, fps = _check(np.array([0.25, 0.5], np.float32), *one)
    assert thr.tolist() == [0.5, 0.25] and tps.tolist() == [0, 3] and fps.tolist() == [2, 2]


def test_counts_partials_of_partials():
    _check(*ref.case((1 << 20) + 3, 11, wmax=1))


@pytest.mark.parametrize("m", [1, 257, 5000])
@pytest.mark.parametrize("kind", ["equal", "distinct"])
def test_counts_all_equal_and_all_distinct(m, kind):
    thr, _, _ = _check(*ref.case(m, 3 * m, kind))
    assert thr.size == (1 if kind == "equal" else m)


def test_counts_tie_runs_across_blocks():
    """Scores in eighths at M = 5000: nine groups, runs of hundreds of items that span radix and scan tiles; the second case
    ends a run exactly at item 2048 of the sorted order (a tile edge of both)."""
    thr, _, _ = _check(*ref.case(5000, 5, "eighths"))
    assert thr.size == 9
    scores = np.concatenate([np.full(2048, 0.75, np.float32), np.full(1024, 0.5, np.float32), np.full(1928, 0.25, np.float32)])
    rng = np.random.default_rng(6)
    perm = rng.permutation(5000)
    pos, neg = rng.integers(0, 3, 5000).astype(np.int32), rng.integers(1, 3, 5000).astype(np.int32)
    thr, tps, fps = _check(scores[perm], pos, neg)
    assert thr.tolist() == [0.75, 0.5, 0.25]


def test_counts_signed_zeros_negatives_denormals_and_adjacent_floats():
    tiny, one = np.float32(1e-45), np.float32(1.0)
    special = np.array([0.0, -0.0, tiny, -tiny, 2 * tiny, np.float32(1.1754942e-38), one, np.nextafter(one, np.float32(2)),
                        np.nextafter(one, np.float32(0)), -3.5, 7.25, -1e30, 3e38, -0.0, 0.0], np.float32)
    rng = np.random.default_rng(8)
    scores = special[rng.integers(0, special.size, 700)]
    scores[:special.size] = special
    pos, neg = rng.integers(0, 4, 700).astype(np.int32), rng.integers(1, 4, 700).astype(np.int32)
    thr, _, _ = _check(scores, pos, neg)
    assert thr.size == special.size - 3  # the four zeros are one group, every other value its own
    assert thr[0] == np.float32(3e38) and thr[-1] == np.float32(-1e30)


def test_counts_zero_weights_and_one_class_only():
    scores, pos, neg = ref.case(3000, 21)
    pos[::2], neg[1::3] = 0, 0
    neg[(pos == 0) & (neg == 0)] = 2
    _check(scores, pos, neg)
    zeros = np.zeros_like(pos)
    _check(scores, zeros, np.maximum(neg, 1))  # all-negative labels: the host's NaN areas (every item keeps a frame: one without
    _check(scores, np.maximum(pos, 1), zeros)  # any has no counterpart among the expanded frames); all-positive


def test_counts_pass_two_to_the_31():
    scores = np.array([0.5, 0.75, 0.5], np.float32)
    w = np.full(3, 1 << 30, np.int32)
    thr, tps, fps = _device_counts(scores, w, w)
    want = ref.weighted_counts(scores, w, w)
    assert tps.tolist() == want[1].tolist() == [1 << 30, 3 << 30] and fps.tolist() == want[2].tolist() and thr.tolist() == [0.75, 0.5]


def test_counts_are_deterministic_and_keep_no_state():
    from anomaly_detection_on_video_amd import mil_ops

    a, b = ref.case(70001, 31), ref.case(4099, 32, "eighths")
    ws = mil_ops.roc_counts_workspace(70001, DEV)
    first = _device_counts(*a, workspace=ws)
    second = _device_counts(*a, workspace=ws)
    other = _device_counts(*b, workspace=ws)  # a different call in between, on the same workspace
    third = _device_counts(*a, workspace=ws)
    fresh = _device_counts(*a)
    for again in (second, third, fresh):
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(first, again))
    assert np.array_equal(other[1], ref.weighted_counts(*b)[1])


def test_wrapper_refusals():
    from anomaly_detection_on_video_amd import _lib, mil_ops

    s, p, n = (torch.from_numpy(x).to(DEV) for x in ref.case(100, 1))
    bad = s.clone()
    bad[3], bad[40], bad[41] = float("nan"), float("inf"), float("-inf")
    with pytest.raises(ValueError, match="3 non-finite scores"):
        mil_ops.roc_counts(bad, p, n)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        mil_ops.roc_counts(s.cpu(), p.cpu(), n.cpu())
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        mil_ops.roc_counts(s, p.cpu(), n)
    with pytest.raises(ValueError, match="scores must be a non-empty fp32"):
        mil_ops.roc_counts(s.double(), p, n)
    with pytest.raises(ValueError, match="scores must be a non-empty fp32"):
        mil_ops.roc_counts(s.view(10, 10), p, n)
    with pytest.raises(ValueError, match="scores must be a non-empty fp32"):
        mil_ops.roc_counts(s[:0], p[:0], n[:0])
    with pytest.raises(ValueError, match="pos must be int32"):
        mil_ops.roc_counts(s, p.long(), n)
    with pytest.raises(ValueError, match=r"neg must be int32 \(100,\)"):
        mil_ops.roc_counts(s, p, n[:99])
    with pytest.raises(_lib.HipExtensionError, match="workspace of 16 bytes"):
        mil_ops.roc_counts(s, p, n, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))


def test_c_abi_refuses_before_any_launch():
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    m = 3000
    need = lib.advhip_roc_counts_ws_bytes(m)
    assert need > 4 * 4 * m and lib.advhip_roc_counts_ws_bytes(1) > 0
    assert lib.advhip_roc_counts_ws_bytes(0) == -1 and lib.advhip_roc_counts_ws_bytes(1 << 31) == -1
    assert b"outside [1, 2^31)" in lib.advhip_last_error()
    s, p, n = (torch.from_numpy(x).to(DEV) for x in ref.case(m, 2))
    thr = torch.full((m,), -7.0, device=DEV)
    tps, fps, meta = (torch.full((k,), -7, device=DEV, dtype=torch.int64) for k in (m, m, 4))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    ptr, st = _lib.ptr, _lib.stream()
    args = lambda: [ptr(s), ptr(p), ptr(n), m, ptr(thr), ptr(tps), ptr(fps), ptr(meta), ptr(ws), need, st]
    for i in (0, 1, 2, 4, 5, 6, 7, 8):
        a = args()
        a[i] = None
        assert lib.advhip_roc_counts(*a) == -1 and b"null pointer" in lib.advhip_last_error(), i
    short = args()
    short[9] = need - 1
    assert lib.advhip_roc_counts(*short) == -1 and b"workspace" in lib.advhip_last_error()
    for bad_m in (0, -5, 1 << 31):
        a = args()
        a[3] = bad_m
        assert lib.advhip_roc_counts(*a) == -1
    torch.cuda.synchronize()
    assert (thr == -7).all() and (tps == -7).all() and (fps == -7).all() and (meta == -7).all() and not ws.any()
    assert lib.advhip_roc_counts(*args()) == 0  # the same arguments as given: accepted
    assert int(meta[0]) == ref.weighted_counts(*ref.case(m, 2))[0].size


# ------------------------------------------------------------------------------ end to end
T = [1, 7, 16, 23, 40, 33]  # windows of the six videos


def _videos(frames_of, seed):
    rng = np.random.default_rng(seed)
    preds = [(np.round(rng.random(t) * 32) / 32).astype(np.float32) for t in T]
    labels = []
    for t in T:
        l = np.zeros(frames_of(t), np.float32)
        a = int(rng.integers(0, l.size))
        l[a:a + int(rng.integers(1, 90))] = 1.0
        labels.append(l)
    return preds, labels


@pytest.mark.parametrize("name,kw,frames_of", [
    ("default", {}, lambda t: t * 16),
    ("frame_step", {"frame_step": 2}, lambda t: t * 32),
    ("clip_stride", {"clip_stride": 8}, lambda t: (t - 1) * 8 + 16 - (3 if t % 2 else 0)),  # every other video cut inside its last window
])
def test_frame_level_auc_device_equals_the_host_function(name, kw, frames_of):
    preds, labels = _videos(frames_of, len(name))
    want = metrics.frame_level_auc(preds, labels, 16, **kw)
    got = metrics.frame_level_auc_device([torch.from_numpy(p).to(DEV) for p in preds], labels, 16, **kw)
    print(name, got, want)
    assert isinstance(got[0], float) and isinstance(got[1], float) and np.isfinite(want).all()
    assert got == want


def test_frame_auc_plan_slots_curve_and_refusals():
    preds, labels = _videos(lambda t: t * 16, 4)
    plan = metrics.FrameAucPlan(labels, T, 16, device=DEV)
    assert len(plan) == 6 and plan.scores.shape == (sum(T),) and plan.slot(2).shape == (16,)
    assert plan.slot(1).data_ptr() == plan.scores.data_ptr() + 4 * T[0]
    for epoch in range(2):  # the plan is reused: new scores, same labels
        for i, p in enumerate(preds):
            plan.slot(i).copy_(torch.from_numpy(p + np.float32(epoch) / 64).to(DEV))
        want = metrics.frame_level_auc([p + np.float32(epoch) / 64 for p in preds], labels, 16)
        assert plan.compute() == want
    thr, tps, fps = plan.curve()
    want_tps, want_fps = metrics._ranked(np.concatenate(labels), np.repeat(np.concatenate(preds) + np.float32(1) / 64, 16))
    assert np.array_equal(tps, want_tps) and np.array_equal(fps, want_fps) and thr.size == tps.size and np.all(np.diff(thr) < 0)
    plan.slot(3)[5] = float("nan")
    with pytest.raises(ValueError, match="1 non-finite scores"):
        plan.compute()
    short = [l.copy() for l in labels]
    short[4] = short[4][:-16]
    with pytest.raises(ValueError, match=r"video 4: 624 frame labels.*40 windows of 16 frames cover 640"):
        metrics.frame_level_auc_device([torch.from_numpy(p).to(DEV) for p in preds], short, 16)
    with pytest.raises(ValueError, match="HIP kernel"):
        metrics.frame_level_auc_device([torch.from_numpy(p) for p in preds], labels, 16)
