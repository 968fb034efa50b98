"""Overlapping clip windows (clip_stride): the host-side rules -- window count, frame-score assembly, which segment of a long
video owns which window -- and the C ABI of the new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO


def _brute_n_windows(F, fpc, s):
    n = 1
    while (n - 1) * s + fpc < F:
        n += 1
    return n


def test_n_windows_against_a_brute_force_count_and_the_reference_rule():
    from anomaly_detection_on_video_amd.extract import n_windows

    for fpc in (8, 16):
        for s in range(1, fpc + 1):
            for F in range(1, 201):
                assert n_windows(F, fpc, s) == _brute_n_windows(F, fpc, s), (F, fpc, s)
        for F in range(1, 201):
            assert n_windows(F, fpc, fpc) == n_windows(F, fpc, None) == (F - 1) // fpc + 1  # src/dataset.py
    for bad in (0, -1, 17):
        with pytest.raises(ValueError):
            n_windows(40, 16, bad)
    with pytest.raises(ValueError):
        n_windows(0, 16, 8)


def frame_scores_np(scores, fpc, s, n_frames=None):
    """The rule, restated: fp32, the covering windows added in ascending order, one division by their count."""
    x = np.asarray(scores, dtype=np.float32)
    n = x.size
    nf = (n - 1) * s + fpc if n_frames is None else n_frames
    out = np.empty((nf,), dtype=np.float32)
    for f in range(nf):
        ws = [w for w in range(n) if w * s <= f < w * s + fpc]
        acc = x[ws[0]]
        for w in ws[1:]:
            acc = np.float32(acc + x[w])
        out[f] = np.float32(acc / np.float32(len(ws)))
    return out


def test_frame_score_rule_against_a_float64_mean():
    from anomaly_detection_on_video_amd import metrics

    rng = np.random.default_rng(3)
    for fpc in (8, 16):
        for s in range(1, fpc + 1):
            for n in (1, 2, 5, 23):
                x = rng.random(n).astype(np.float32)
                covered = (n - 1) * s + fpc
                for nf in (None, covered - min(fpc - 1, covered - 1)):
                    want32 = frame_scores_np(x, fpc, s, nf)
                    got = metrics.frame_scores(x, fpc, s, nf)
                    assert got.dtype == np.float32 and np.array_equal(got, want32), (fpc, s, n, nf)
                    length = covered if nf is None else nf
                    mean64 = np.array([np.mean([np.float64(x[w]) for w in range(n) if w * s <= f < w * s + fpc]) for f in range(length)])
                    assert got.shape == (length,)
                    # scores in [0, 1]: each of the <= 15 adds rounds a partial sum <= 16 (<= 16 * 2^-24 each, <= 15 * 2^-24 after
                    # the division by the count), the division itself rounds a mean <= 1 (<= 2^-24)
                    assert np.max(np.abs(got.astype(np.float64) - mean64)) <= 16 * 2.0 ** -24
        x = rng.random(9).astype(np.float32)
        assert np.array_equal(metrics.frame_scores(x, fpc, fpc), np.repeat(x, fpc))
        assert np.array_equal(frame_scores_np(x, fpc, fpc), np.repeat(x, fpc))
        assert np.array_equal(metrics.frame_scores(x, fpc), np.repeat(x, fpc))
    with pytest.raises(ValueError):
        metrics.frame_scores(np.zeros(3, np.float32), 16, 8, 33)  # three windows at stride 8 cover 32 frames
    with pytest.raises(ValueError):
        metrics.frame_scores(np.zeros(3, np.float32), 16, 0)
    with pytest.raises(ValueError):
        metrics.frame_scores(np.zeros(3, np.float32), 16, 17)


def test_frame_level_auc_is_unchanged_at_the_clip_length_and_uses_the_rule_below_it():
    from anomaly_detection_on_video_amd import metrics
    from oracle import host_oracle

    g = np.load(os.path.join(GOLDEN, "auc.npz"))
    labels, preds = g["labels"], g["preds"]
    # the known answers as one video of one-frame clips: frame_level_auc itself, with and without the argument
    for kw in ({}, {"clip_stride": 1}, {"clip_stride": None}):
        roc, pr = metrics.frame_level_auc([preds], [labels], frames_per_clip=1, **kw)
        assert abs(roc - float(g["roc_auc"])) < 1e-12 and abs(pr - float(g["pr_auc"])) < 1e-12
    rng = np.random.default_rng(0)
    p = [np.round(rng.random(7), 1), np.round(rng.random(11), 1)]
    l = [(rng.random(7 * 16) < 0.3).astype(float), (rng.random(11 * 16) < 0.3).astype(float)]
    assert metrics.frame_level_auc(p, l, clip_stride=16) == metrics.frame_level_auc(p, l) == metrics.frame_level_auc(p, l, clip_stride=None)
    want = host_oracle.frame_level_auc(p, l)
    got = metrics.frame_level_auc(p, l, clip_stride=16)
    assert abs(got[0] - want[0]) < 1e-12 and abs(got[1] - want[1]) < 1e-12
    # stride 8: 7 windows cover 64 frames, 11 cover 96; the second video's labels stop at its own length, inside the last window
    l8 = [(rng.random(64) < 0.3).astype(float), (rng.random(90) < 0.3).astype(float)]
    dense = np.concatenate([frame_scores_np(p[0], 16, 8), frame_scores_np(p[1], 16, 8, 90)])
    got = metrics.frame_level_auc(p, l8, clip_stride=8)
    assert got == (metrics.roc_auc(np.concatenate(l8), dense), metrics.pr_auc(np.concatenate(l8), dense))
    with pytest.raises(ValueError):
        metrics.frame_level_auc(p, l, clip_stride=8)  # labels of the back-to-back clips: too long for the windows


def test_segments_own_the_windows_that_start_in_them():
    from anomaly_detection_on_video_amd.extract import n_windows, segment_windows

    seg_len = 48
    lengths = sorted({F for m in range(0, 5) for F in range(m * seg_len - 17, m * seg_len + 18) if F >= 1})
    for fpc in (8, 16):
        for s in [s for s in range(1, fpc + 1) if seg_len % s == 0]:
            for F in lengths:
                n = n_windows(F, fpc, s)
                plan = segment_windows(F, seg_len, fpc, s)
                owned = []
                for seg, w0, w1, lo, hi in plan:
                    assert 0 <= seg <= F // seg_len and w0 < w1
                    assert all(seg * seg_len <= w * s < (seg + 1) * seg_len for w in range(w0, w1))  # the windows that START here
                    assert (lo, hi) == (seg * seg_len, min((seg + 1) * seg_len + fpc - s, F))
                    assert n_windows(hi - lo, fpc, s) == w1 - w0      # the segment's frames, as a video, have exactly those windows
                    for w in range(w0, w1):                           # ... and no window but the video's last is short
                        assert w * s + fpc <= hi or w == n - 1, (F, fpc, s, seg, w)
                    owned += list(range(w0, w1))
                assert owned == list(range(n)), (F, fpc, s)
                assert [p[0] for p in plan] == sorted(p[0] for p in plan)
    assert segment_windows(96, 48, 16, 16) == [(0, 0, 3, 0, 48), (1, 3, 6, 48, 96)]  # the reference's empty last segment is skipped
    assert segment_windows(100, 48, 16, 8) == [(0, 0, 6, 0, 56), (1, 6, 12, 48, 100)]  # frames 96..99: inside window 11, owned by 1
    for bad in ((100, 48, 16, 5), (100, 48, 16, 0), (100, 48, 16, 17), (100, 40, 16, 16)):
        with pytest.raises(ValueError):
            segment_windows(*bad)


NEW_SYMBOLS = {
    "advhip_tencrop_normalize_u8_strided": 12,
    "advhip_tencrop_normalize_planes_u8_strided": 14,
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32": 18,
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_strided_f32": 19,
    "advhip_frame_scores_f32": 7,
}


def _header_prototypes():
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(advhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_and_ctypes_agree_on_the_new_entry_points():
    """Each new symbol: declared in include/advhip.h, exported, and its ctypes signature has the header's argument list, type by
    type (int32_t / int64_t / float / pointer) -- an argument added on one side only would shift every later operand."""
    import ctypes as C

    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    protos = _header_prototypes()
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_float: "float"}
    for name, n_args in NEW_SYMBOLS.items():
        assert name in protos, f"{name} not declared in include/advhip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(argtypes) == n_args, name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p)
            else:
                assert p.split()[0] == kinds[t], (name, p, t)
    assert lib.advhip_abi_version() == 2  # (the ABI only gained entry points)


def test_new_entry_points_validate_before_any_launch():
    """Bad strides, ranges and frame counts are refused with a message (nothing below launches: every call fails validation)."""
    import ctypes as C

    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    p = C.c_void_p(4096)  # stands for a device pointer
    f = C.c_float
    assert lib.advhip_frame_scores_f32(p, p, 3, 16, 0, 32, None) == -1 and b"clip stride 0 outside [1, 16]" in lib.advhip_last_error()
    assert lib.advhip_frame_scores_f32(p, p, 3, 16, 17, 32, None) == -1 and b"clip stride 17" in lib.advhip_last_error()
    assert lib.advhip_frame_scores_f32(p, p, 3, 16, 8, 33, None) == -1 and b"cover 32" in lib.advhip_last_error()
    assert lib.advhip_frame_scores_f32(None, p, 3, 16, 8, 32, None) == -1
    assert lib.advhip_tencrop_normalize_u8_strided(p, p, 40, 256, 340, 3, 16, 17, 224, f(114.75), f(57.375), None) == -1
    assert b"clip stride 17 outside [1, 16]" in lib.advhip_last_error()
    # 40 frames at stride 8: 4 windows = 40 crop-clips
    assert lib.advhip_tencrop_normalize_planes_u8_strided(p, p, 40, 256, 340, 3, 16, 8, 224, 35, 6, f(114.75), f(57.375), None) == -1
    assert b"outside the video's 40" in lib.advhip_last_error()
    assert lib.advhip_tencrop_normalize_planes_u8_strided(p, p, 40, 256, 340, 3, 16, 0, 224, 0, 6, f(114.75), f(57.375), None) == -1
    stem = _lib.ConvDesc(8, 3, 16, 224, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    FH, FW = 256, 340
    taps = lambda F, s, first: (C.byref(stem), p, F, FH, FW, s, F * FH * FW * 3 + 4, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    byts = lambda F, s, first: (C.byref(stem), p, F, FH, FW, s, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    for fn, args in ((lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_strided_f32, taps),
                     (lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32, byts)):
        assert fn(*args(41, 8, 0)) == -1 and b"not whole clips of 16 at stride 8" in lib.advhip_last_error()
        assert fn(*args(40, 8, 33)) == -1 and b"outside the 4 clips x 10 crops" in lib.advhip_last_error()  # 33 + 8 > 40
        assert fn(*args(40, 0, 0)) == -1 and b"clip stride 0 outside [1, 16]" in lib.advhip_last_error()
        assert fn(*args(40, 17, 0)) == -1 and b"clip stride 17" in lib.advhip_last_error()
        assert fn(*args(8, 8, 0)) == -1 and b"not whole clips" in lib.advhip_last_error()  # shorter than one window
