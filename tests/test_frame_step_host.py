"""Temporal sampling (frame_step): the host-side rules -- which frames a window samples, window count, stride bound, segments,
file names, the whole-window buffer, frame scores on spans, the command line -- and the C ABI of the new entry points.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def brute_windows(F, fpc, s, d):
    """The issue's semantics, by enumeration: windows are added until one's span [w s, w s + fpc d) reaches the video's end;
    sampled frame t of window w is frame w s + t d while that exists, and the frames that exist are repeated (LoopPad)."""
    wins, w = [], 0
    while True:
        have = [w * s + t * d for t in range(fpc) if w * s + t * d < F]
        assert have, (F, fpc, s, d, w)
        wins.append([have[t % len(have)] for t in range(fpc)])
        if w * s + fpc * d >= F:
            return wins
        w += 1


def existing_windows(F, fpc, s):
    """What the existing path (no frame_step) does with a video of F frames, on indices."""
    from anomaly_detection_on_video_amd.ops import n_windows

    out = []
    for w in range(n_windows(F, fpc, s)):
        length = min(fpc, F - w * s)
        out.append([w * s + t % length for t in range(fpc)])
    return out


def test_the_two_identities_on_indices():
    """1. Row w is the existing path's one-clip video frames[w*s : w*s + fpc*d : d].  2. If d divides s, the whole result is the
    existing path on frames[::d] at clip_stride s // d, window counts included.  Every legal s, F up to 5 * fpc * d + 2."""
    from anomaly_detection_on_video_amd.ops import n_windows, window_frame_indices

    for fpc in (4, 8, 16):
        for d in (1, 2, 3, 8):
            for s in range(1, fpc * d + 1):
                for F in range(1, 5 * fpc * d + 3, 1 if fpc * d <= 32 else 7):
                    wins = brute_windows(F, fpc, s, d)
                    n = len(wins)
                    assert n == n_windows(F, fpc, s, frame_step=d) == 1 + max(0, -(-(F - fpc * d) // s)), (F, fpc, s, d)
                    for w in (0, n // 2, n - 1):
                        assert list(window_frame_indices(F, w, fpc, s, d)) == wins[w]
                        one_clip = list(range(F))[w * s : w * s + fpc * d : d]  # the slice ends with the video
                        assert len(one_clip) == min(fpc, -(-(F - w * s) // d)) >= 1
                        assert len(one_clip) == fpc or w == n - 1  # only the last window can be short
                        assert [one_clip[i] for i in existing_windows(len(one_clip), fpc, fpc)[0]] == wins[w]
                    if s % d == 0:
                        dec = list(range(F))[::d]
                        ex = existing_windows(len(dec), fpc, s // d)
                        assert len(ex) == n and [[dec[i] for i in win] for win in ex] == wins, (F, fpc, s, d)
                    # default stride: every frame lies in exactly one span
                    if s == fpc * d:
                        assert n_windows(F, fpc, None, frame_step=d) == n == -(-F // (fpc * d))


def test_resolve_frame_step_and_the_stride_bound():
    from anomaly_detection_on_video_amd import ops

    assert ops.resolve_frame_step(None) == 1 and ops.resolve_frame_step(1) == 1 and ops.resolve_frame_step(np.int64(8)) == 8
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError):
            ops.resolve_frame_step(bad)
    assert ops.resolve_clip_stride(16, None) == 16 and ops.resolve_clip_stride(16, None, 2) == 32 and ops.resolve_clip_stride(8, None, 8) == 64
    assert ops.resolve_clip_stride(16, 32, 2) == 32 and ops.resolve_clip_stride(16, 1, 2) == 1 and ops.resolve_clip_stride(16, 17, 2) == 17
    for fpc, s, d in ((16, 33, 2), (16, 0, 2), (16, 17, None), (16, 17, 1), (8, 65, 8)):
        with pytest.raises(ValueError):
            ops.resolve_clip_stride(fpc, s, d)
    assert ops.n_windows(70, 16, None, frame_step=2) == 3 and ops.n_windows(70, 16, 24, frame_step=2) == 3
    assert ops.n_windows(70, 16) == ops.n_windows(70, 16, frame_step=None) == ops.n_windows(70, 16, frame_step=1) == 5
    with pytest.raises(ValueError):
        ops.n_windows(0, 16, frame_step=2)
    with pytest.raises(ValueError):
        ops.n_windows(70, 16, 33, frame_step=2)


def test_segments_own_the_windows_that_start_in_them_with_frame_step():
    from anomaly_detection_on_video_amd.extract import n_windows, segment_windows

    seg_len = 48
    lengths = sorted({F for m in range(0, 5) for F in range(m * seg_len - 17, m * seg_len + 18) if F >= 1})
    for fpc, d in ((8, 2), (16, 2), (8, 3), (4, 8)):
        span = fpc * d
        for s in [s for s in range(1, span + 1) if seg_len % s == 0]:
            for F in lengths:
                n = n_windows(F, fpc, s, frame_step=d)
                plan = segment_windows(F, seg_len, fpc, s, frame_step=d)
                owned, full = [], brute_windows(F, fpc, s, d)
                for seg, w0, w1, lo, hi in plan:
                    part = brute_windows(hi - lo, fpc, s, d)
                    assert 0 <= seg <= F // seg_len and w0 < w1
                    assert all(seg * seg_len <= w * s < (seg + 1) * seg_len for w in range(w0, w1))  # the windows that START here
                    assert (lo, hi) == (seg * seg_len, min((seg + 1) * seg_len + span - s, F))
                    assert n_windows(hi - lo, fpc, s, frame_step=d) == w1 - w0  # the segment's frames, as a video, have exactly those
                    for w in range(w0, w1):  # ... sampling the same frames; no window but the video's last is short
                        assert [lo + i for i in part[w - w0]] == full[w]
                        assert w * s + (fpc - 1) * d < hi or w == n - 1, (F, fpc, s, d, seg, w)
                    owned += list(range(w0, w1))
                assert owned == list(range(n)), (F, fpc, s, d)  # the owned windows partition the video's
    assert segment_windows(70, 64, 16, None, frame_step=2) == [(0, 0, 2, 0, 64), (1, 2, 3, 64, 70)]
    assert segment_windows(70, 64, 16, 16, frame_step=2) == [(0, 0, 4, 0, 70)]
    assert segment_windows(100, 48, 16, 8) == [(0, 0, 6, 0, 56), (1, 6, 12, 48, 100)]  # unchanged without the argument
    for bad in ((100, 48, 16, 5, 2), (100, 48, 16, 33, 2), (100, 40, 16, None, 2), (100, 48, 16, 8, 0)):
        with pytest.raises(ValueError):
            segment_windows(*bad[:4], frame_step=bad[4])


def test_feature_tag_with_frame_step():
    from anomaly_detection_on_video_amd.extract import feature_tag

    assert feature_tag() == "" and feature_tag(16, 16) == "" and feature_tag(16, None, None, None) == "" and feature_tag(16, None, None, 1) == ""
    assert feature_tag(16, 8) == "_s8" and feature_tag(16, 8, "center") == "_s8_c4"  # names without frame_step are unchanged
    assert feature_tag(16, None, None, 2) == "_d2" and feature_tag(16, 32, None, 2) == "_d2"
    assert feature_tag(16, 8, "center", 2) == "_d2_s8_c4" and feature_tag(16, 16, None, 2) == "_d2_s16"
    assert feature_tag(8, None, "five", 8) == "_d8_c01234" and feature_tag(8, 8, None, 8) == "_d8_s8"
    with pytest.raises(ValueError):
        feature_tag(16, 33, None, 2)
    with pytest.raises(ValueError):
        feature_tag(16, None, None, 0)


def test_pad_windows_u8_on_cpu_tensors():
    """The slots the last window reads hold its LoopPad frames, the video itself is kept, and a whole last window is its input."""
    from anomaly_detection_on_video_amd.ops import n_windows, pad_windows_u8

    for fpc, d in ((16, 2), (16, 3), (8, 8), (4, 2)):
        for s in (None, 1, 5, fpc * d - 1, d, 2 * d):
            ss = fpc * d if s is None else s
            for F in (1, 5, (fpc - 1) * d, (fpc - 1) * d + 1, fpc * d, fpc * d + 1, 2 * fpc * d + 7):
                frames = torch.arange(F, dtype=torch.uint8).view(F, 1, 1, 1).expand(F, 2, 3, 3).contiguous()
                wins = brute_windows(F, fpc, ss, d)
                n = len(wins)
                out = pad_windows_u8(frames, fpc, s, d)
                assert out.shape[0] == (n - 1) * ss + (fpc - 1) * d + 1 and out.shape[1:] == frames.shape[1:]
                keep = min(F, out.shape[0])
                assert torch.equal(out[:keep], frames[:keep])
                for w in (0, n - 1):
                    slots = [w * ss + t * d for t in range(fpc)]
                    assert out[slots, 0, 0, 0].tolist() == [i % 256 for i in wins[w]], (fpc, d, s, F, w)
                if (n - 1) * ss + (fpc - 1) * d < F:  # whole: a view of the input, nothing copied
                    assert out.data_ptr() == frames.data_ptr()
                # the buffer is whole windows in the stems' sense: n of them
                assert (out.shape[0] - ((fpc - 1) * d + 1)) % ss == 0 and (out.shape[0] - ((fpc - 1) * d + 1)) // ss + 1 == n
                assert n == n_windows(F, fpc, s, frame_step=d)
    frames = torch.arange(37, dtype=torch.uint8).view(37, 1, 1, 1)
    assert torch.equal(pad_windows_u8(frames, 16, 8), pad_windows_u8(frames, 16, 8, None))  # d = 1: the existing rule
    assert torch.equal(pad_windows_u8(frames, 16, 8, 1), pad_windows_u8(frames, 16, 8))
    assert pad_windows_u8(frames, 16, 8).shape[0] == 3 * 8 + 16


def frame_scores_np(scores, fpc, s, d, n_frames=None):
    x = np.asarray(scores, dtype=np.float32)
    n = x.size
    nf = (n - 1) * s + fpc * d if n_frames is None else n_frames
    out = np.empty((nf,), dtype=np.float32)
    for f in range(nf):
        ws = [w for w in range(n) if w * s <= f < w * s + fpc * d]
        acc = x[ws[0]]
        for w in ws[1:]:
            acc = np.float32(acc + x[w])
        out[f] = np.float32(acc / np.float32(len(ws)))
    return out


def test_metrics_frame_scores_and_auc_on_spans():
    from anomaly_detection_on_video_amd import metrics

    rng = np.random.default_rng(5)
    for fpc, d in ((16, 2), (8, 8), (16, 3)):
        span = fpc * d
        for n in (1, 2, 9):
            x = rng.random(n).astype(np.float32)
            for s in (1, 5, d, span - 1, span):
                got = metrics.frame_scores(x, fpc, s, frame_step=d)
                assert got.dtype == np.float32 and np.array_equal(got, frame_scores_np(x, fpc, s, d))
                nf = (n - 1) * s + 1
                assert np.array_equal(metrics.frame_scores(x, fpc, s, nf, frame_step=d), frame_scores_np(x, fpc, s, d, nf))
            F = (n - 1) * span + 3
            assert np.array_equal(metrics.frame_scores(x, fpc, None, F, frame_step=d), np.repeat(x, span)[:F])
            assert np.array_equal(metrics.frame_scores(x, fpc, frame_step=d), np.repeat(x, span))
        with pytest.raises(ValueError):
            metrics.frame_scores(np.zeros(3, np.float32), fpc, span + 1, frame_step=d)
        with pytest.raises(ValueError):
            metrics.frame_scores(np.zeros(3, np.float32), fpc, frame_step=0)
    assert np.array_equal(metrics.frame_scores(x, 16, 8), metrics.frame_scores(x, 16, 8, frame_step=1))
    p = [np.round(rng.random(4), 1), np.round(rng.random(6), 1)]
    l = [(rng.random(4 * 32) < 0.3).astype(float), (rng.random(6 * 32) < 0.3).astype(float)]
    # default stride: np.repeat at the span; the same as one-frame-in-one clips of 32 frames
    assert metrics.frame_level_auc(p, l, frame_step=2) == metrics.frame_level_auc(p, l, frames_per_clip=32)
    assert metrics.frame_level_auc(p, l, frame_step=2, clip_stride=32) == metrics.frame_level_auc(p, l, frames_per_clip=32)
    l8 = [(rng.random(3 * 8 + 32) < 0.3).astype(float), (rng.random(5 * 8 + 20) < 0.3).astype(float)]  # the second ends inside its last span
    dense = np.concatenate([frame_scores_np(p[0], 16, 8, 2), frame_scores_np(p[1], 16, 8, 2, 60)])
    got = metrics.frame_level_auc(p, l8, clip_stride=8, frame_step=2)
    assert got == (metrics.roc_auc(np.concatenate(l8), dense), metrics.pr_auc(np.concatenate(l8), dense))
    with pytest.raises(ValueError):
        metrics.frame_level_auc(p, l, clip_stride=33, frame_step=2)


def test_frame_crops_key_carries_the_frame_step():
    from anomaly_detection_on_video_amd.pipeline import FrameCrops

    fr = torch.zeros((47, 72, 90, 3), dtype=torch.uint8)
    base = FrameCrops(fr, 0, 10, 16, 64)
    assert base.key() == FrameCrops(fr, 0, 10, 16, 64, frame_step=None).key() == FrameCrops(fr, 0, 10, 16, 64, frame_step=1).key()
    assert base.key() == ("u8", 10, (72, 90), 16, 64, 16)  # unchanged without the argument
    two = FrameCrops(fr, 0, 10, 16, 64, frame_step=2)
    assert two.clip_stride == 32 and two.frame_step == 2
    keys = {base.key(), two.key(), FrameCrops(fr, 0, 10, 16, 64, frame_step=2, clip_stride=16).key(), FrameCrops(fr, 0, 10, 16, 64, frame_step=3).key(),
            FrameCrops(fr, 0, 10, 16, 64, clip_stride=16, frame_step=2, crops="center").key()}
    assert len(keys) == 5
    assert FrameCrops(fr, 0, 10, 16, 64, clip_stride=32, frame_step=2).key() == two.key()
    for bad in (dict(frame_step=0), dict(frame_step=2, clip_stride=33), dict(clip_stride=17)):
        with pytest.raises(ValueError):
            FrameCrops(fr, 0, 10, 16, 64, **bad)


def test_cli_frame_step_argument_errors():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "extract_features.py"), *a], capture_output=True, text=True, cwd=REPO)
    r = run("--frame-step", "2")
    assert r.returncode == 2 and "--frame-step needs --frame-size" in r.stderr
    r = run("--frame-size", "240x320", "--frame-step", "0")
    assert r.returncode == 2 and "--frame-step 0 must be at least 1" in r.stderr
    r = run("--frame-size", "240x320", "--frame-step", "2", "--clip-stride", "33")
    assert r.returncode == 2 and "--clip-stride 33 outside [1, 32]" in r.stderr
    r = run("--frame-size", "240x320", "--clip-stride", "17")
    assert r.returncode == 2 and "--clip-stride 17 outside [1, 16]" in r.stderr

    import extract_features

    with pytest.raises(ValueError, match="--frame-step needs --frame-size"):
        extract_features.main(frame_step=2)
    with pytest.raises(ValueError, match="must be at least 1"):
        extract_features.main(frame_size=(240, 320), frame_step=0)
    with pytest.raises(ValueError, match=r"outside \[1, 32\]"):
        extract_features.main(frame_size=(240, 320), frame_step=2, clip_stride=33)
    with pytest.raises(ValueError, match=r"outside \[1, 16\]"):
        extract_features.main(frame_size=(240, 320), clip_stride=17)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = {
    "advhip_tencrop_normalize_u8_sampled": 15,
    "advhip_tencrop_normalize_planes_u8_sampled": 17,
    "advhip_conv3d_u8_build_tables_sampled": 9,
    "advhip_conv3d_u8_taps_build_tables_sampled": 10,
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32": 21,
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_sampled_f32": 22,
    "advhip_resize_u8_sampled": 19,
}


def _header_prototypes():
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(advhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _lib_built():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib, _lib.load()


def test_header_and_ctypes_agree_on_the_new_entry_points():
    """Every `_sampled` symbol of the header is exported and has a ctypes signature with the header's argument list, type by
    type; SIGNATURES covers every symbol the header declares; the ABI only gained entry points."""
    _lib, lib = _lib_built()
    protos = _header_prototypes()
    assert {n for n in protos if n.endswith("_sampled") or n.endswith("_sampled_f32")} == set(NEW_SYMBOLS)
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_float: "float", C.c_uint64: "uint64_t"}
    for name, n_args in NEW_SYMBOLS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(argtypes) == n_args, (name, len(params), len(argtypes))
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p)
            else:
                assert p.split()[0] == kinds[t], (name, p, t)
    assert set(protos) <= set(_lib.SIGNATURES)
    assert lib.advhip_abi_version() == 2


def test_new_entry_points_refuse_before_any_launch():
    """d = 0, s = fpc * d + 1, an F that is not whole windows, a range past the end: ADVHIP_EINVAL (-1) with a message, from each
    new entry point (every call below fails validation: nothing is launched, the pointers are never dereferenced)."""
    _lib, lib = _lib_built()
    p = C.c_void_p(4096)  # stands for a device pointer
    f = C.c_float
    m, sd = f(114.75), f(57.375)
    ten = 0x9876543210
    dense = lambda F, s, d: lib.advhip_tencrop_normalize_u8_sampled(p, p, F, 256, 340, 3, 16, s, d, 224, 10, ten, m, sd, None)
    planes = lambda F, s, d, first, count: lib.advhip_tencrop_normalize_planes_u8_sampled(p, p, F, 256, 340, 3, 16, s, d, 224, 10, ten, first, count, m, sd, None)
    assert dense(70, 32, 0) == -1 and b"frame step 0" in lib.advhip_last_error()
    assert dense(70, 33, 2) == -1 and b"clip stride 33 outside [1, 32]" in lib.advhip_last_error()
    assert dense(70, 0, 2) == -1 and b"clip stride 0 outside [1, 32]" in lib.advhip_last_error()
    assert planes(70, 32, 0, 0, 10) == -1 and b"frame step 0" in lib.advhip_last_error()
    assert planes(70, 33, 2, 0, 10) == -1 and b"clip stride 33 outside [1, 32]" in lib.advhip_last_error()
    assert planes(70, 32, 2, 25, 6) == -1 and b"outside the video's 30" in lib.advhip_last_error()  # 70 frames, spans of 32: 3 windows
    assert planes(70, 24, 2, 30, 1) == -1 and b"outside the video's 30" in lib.advhip_last_error()
    assert planes(70, 5, 2, 89, 2) == -1 and b"outside the video's 90" in lib.advhip_last_error()   # 1 + ceil(38 / 5) = 9 windows
    assert planes(70, 32, 2, -1, 2) == -1

    stem = _lib.ConvDesc(8, 3, 16, 224, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    FH, FW = 256, 340
    taps = lambda F, s, d, first: lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_sampled_f32(
        C.byref(stem), p, F, FH, FW, s, d, 10, ten, F * FH * FW * 3 + 4, first, p, p, p, p, p, sd, p, 0, p, 1 << 40, None)
    byts = lambda F, s, d, first: lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32(
        C.byref(stem), p, F, FH, FW, s, d, 10, ten, first, p, p, p, p, p, sd, p, 0, p, 1 << 40, None)
    for fn in (taps, byts):
        # whole windows at d = 2, s = 24: F = 31 + 24 k
        assert fn(79, 24, 0, 0) == -1 and b"frame step 0" in lib.advhip_last_error()
        assert fn(79, 33, 2, 0) == -1 and b"clip stride 33 outside [1, 32]" in lib.advhip_last_error()
        assert fn(79, 0, 2, 0) == -1 and b"clip stride 0 outside [1, 32]" in lib.advhip_last_error()
        assert fn(80, 24, 2, 0) == -1 and b"not whole clips of 16, one frame in 2, at stride 24" in lib.advhip_last_error()
        assert fn(30, 24, 2, 0) == -1 and b"not whole clips" in lib.advhip_last_error()  # shorter than one window's reach
        assert fn(96, 32, 2, 0) == -1 and b"not whole clips" in lib.advhip_last_error()  # whole SPANS are not whole windows
        assert fn(79, 24, 2, 23) == -1 and b"outside the 3 clips x 10 crops" in lib.advhip_last_error()  # 23 + 8 > 30
        assert fn(79, 24, 2, -1) == -1
    tabs = lambda d: lib.advhip_conv3d_u8_build_tables_sampled(C.byref(stem), FH, FW, d, p, m, p, p, None)
    ttabs = lambda d: lib.advhip_conv3d_u8_taps_build_tables_sampled(C.byref(stem), FH, FW, d, p, m, p, p, p, None)
    for fn in (tabs, ttabs):
        assert fn(0) == -1 and b"frame step 0" in lib.advhip_last_error()
        assert fn(-3) == -1
        assert fn(1 << 20) == -1  # the temporal pitch would leave the 2 GiB the gather addresses
    small = _lib.ConvDesc(8, 3, 16, 300, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    assert lib.advhip_conv3d_u8_build_tables_sampled(C.byref(small), FH, FW, 2, p, m, p, p, None) == -1
    assert b"smaller than the 300 x 224 crop" in lib.advhip_last_error()

    rs = lambda F, d, **kw: lib.advhip_resize_u8_sampled(kw.get("src", p), p, p, F, d, 240, 320, 3, 256, 341, p, p, 3, p, p, 3, 0, 240, None)
    assert rs(7, 0) == -1 and b"frame step 0" in lib.advhip_last_error()
    assert rs(7, -1) == -1
    assert rs(0, 2) == -1 and b"sizes must be >= 1" in lib.advhip_last_error()
    assert rs(7, 2, src=None) == -1 and b"null frames" in lib.advhip_last_error()


def test_old_entry_points_answer_as_before():
    """The arguments tests/test_capi_and_host.py and tests/test_clip_stride_host.py hand the old entry points: the same codes and
    messages now that those forward to the `_sampled` ones with frame_step = 1."""
    _lib, lib = _lib_built()
    p = C.c_void_p(4096)
    f = C.c_float
    stem = _lib.ConvDesc(8, 3, 16, 224, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    nk, nf, nw = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.advhip_conv3d_u8_table_sizes(C.byref(stem), C.byref(nk), C.byref(nf)) == 0
    assert (nk.value, nf.value) == (4 * 736, 9 * 16 * 16 * 64)
    assert lib.advhip_conv3d_u8_taps_table_sizes(C.byref(stem), C.byref(nk), C.byref(nf), C.byref(nw)) == 0
    assert (nk.value, nw.value) == (4 * 248, 248 * 3 * 64)
    F, FH, FW = 32, 256, 340
    nbytes = F * FH * FW * 3
    args = lambda d, frames_F, readable, first: (C.byref(d), p, frames_F, FH, FW, readable, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    old_taps = lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_f32
    assert old_taps(*args(stem, F, nbytes, 0)) == -1 and b"one byte past the last pixel" in lib.advhip_last_error()
    assert old_taps(*args(stem, F, nbytes + 4, 13)) == -1 and b"outside the 2 clips x 10 crops" in lib.advhip_last_error()
    assert old_taps(*args(stem, F - 1, nbytes + 4, 0)) == -1 and b"not whole clips of 16 at stride 16" in lib.advhip_last_error()
    wide = _lib.ConvDesc(8, 4, 16, 224, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    assert old_taps(*args(wide, F, nbytes + 4, 0)) == -1 and b"3-channel pixels" in lib.advhip_last_error()
    big = _lib.ConvDesc(8, 3, 16, 300, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    assert lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_f32(C.byref(big), p, F, FH, FW, 0, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None) == -1
    assert b"smaller than the 300 x 224 crop" in lib.advhip_last_error()
    m, sd = f(114.75), f(57.375)
    assert lib.advhip_tencrop_normalize_u8_strided(p, p, 40, 256, 340, 3, 16, 17, 224, m, sd, None) == -1
    assert b"clip stride 17 outside [1, 16]" in lib.advhip_last_error()
    assert lib.advhip_tencrop_normalize_planes_u8_strided(p, p, 40, 256, 340, 3, 16, 8, 224, 35, 6, m, sd, None) == -1
    assert b"outside the video's 40" in lib.advhip_last_error()
    assert lib.advhip_tencrop_normalize_u8_crops(p, p, 40, 256, 340, 3, 16, 8, 224, 2, 0x49, m, sd, None) == -1  # descending set
    assert b"crop set" in lib.advhip_last_error()
    taps = lambda F, s, first: (C.byref(stem), p, F, FH, FW, s, F * FH * FW * 3 + 4, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    byts = lambda F, s, first: (C.byref(stem), p, F, FH, FW, s, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    for fn, a in ((lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_strided_f32, taps), (lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32, byts)):
        assert fn(*a(41, 8, 0)) == -1 and b"not whole clips of 16 at stride 8" in lib.advhip_last_error()
        assert fn(*a(40, 8, 33)) == -1 and b"outside the 4 clips x 10 crops" in lib.advhip_last_error()
        assert fn(*a(40, 0, 0)) == -1 and b"clip stride 0 outside [1, 16]" in lib.advhip_last_error()
        assert fn(*a(40, 17, 0)) == -1 and b"clip stride 17" in lib.advhip_last_error()
        assert fn(*a(8, 8, 0)) == -1 and b"not whole clips" in lib.advhip_last_error()
    assert lib.advhip_resize_u8(p, p, p, 0, 240, 320, 3, 256, 341, p, p, 3, p, p, 3, 0, 240, None) == -1
    assert b"sizes must be >= 1" in lib.advhip_last_error()
