"""Frame-level ROC-AUC / PR-AUC of `on_validation_epoch_end` (/root/reference/src/runner.py:62-79)
restated in numpy (sklearn is optional; pinned against sklearn known-answers in the tests)."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np


def _ranked(labels, preds):
    y = np.asarray(labels, dtype=np.float64).ravel() > 0.5
    s = np.asarray(preds, dtype=np.float64).ravel()
    order = np.argsort(-s, kind="stable")
    y, s = y[order], s[order]
    cut = np.flatnonzero(np.diff(s))
    idx = np.concatenate([cut, [y.size - 1]])
    tps = np.cumsum(y)[idx].astype(np.float64)
    fps = 1.0 + idx - tps
    return tps, fps


def _area(x: np.ndarray, y: np.ndarray) -> float:
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def roc_auc(labels: Sequence[float], preds: Sequence[float]) -> float:
    tps, fps = _ranked(labels, preds)
    tpr = np.concatenate([[0.0], tps]) / tps[-1]
    fpr = np.concatenate([[0.0], fps]) / fps[-1]
    return _area(fpr, tpr)


def pr_auc(labels: Sequence[float], preds: Sequence[float]) -> float:
    tps, fps = _ranked(labels, preds)
    precision = np.concatenate([(tps / (tps + fps))[::-1], [1.0]])
    recall = np.concatenate([(tps / tps[-1])[::-1], [0.0]])
    return -_area(recall, precision)


def _frame_step(frame_step) -> int:
    d = 1 if frame_step is None else int(frame_step)
    if d < 1:
        raise ValueError(f"frame_step {frame_step!r}: an integer >= 1")
    return d


def frame_scores(scores, frames_per_clip: int = 16, clip_stride: Optional[int] = None, n_frames: Optional[int] = None,
                 frame_step: Optional[int] = None) -> np.ndarray:
    """Per-window scores (n,) -> per-frame scores, fp32 (what mil_ops.frame_scores computes on the device).  Window w covers
    frames [w * clip_stride, w * clip_stride + frames_per_clip); a frame's score is the mean of the scores of the windows
    covering it: added in ascending window order, one division by the count.  Length n_frames, default (n - 1) * clip_stride +
    frames_per_clip; clip_stride = frames_per_clip (the default) is np.repeat(scores, frames_per_clip) bit for bit.
    `frame_step` d (temporal sampling: a window's frames_per_clip sampled frames stand for a span of frames_per_clip * d frames):
    the same rule on spans -- window w covers [w * clip_stride, w * clip_stride + frames_per_clip * d), clip_stride defaults to
    the span and may be up to it; the default stride is np.repeat(scores, frames_per_clip * d)."""
    d = _frame_step(frame_step)
    if d != 1:
        return frame_scores(scores, frames_per_clip * d, frames_per_clip * d if clip_stride is None else clip_stride, n_frames)
    s = frames_per_clip if clip_stride is None else int(clip_stride)
    if not 1 <= s <= frames_per_clip:
        raise ValueError(f"clip_stride {clip_stride} outside [1, frames_per_clip = {frames_per_clip}]")
    x = np.asarray(scores, dtype=np.float32).ravel()
    if x.size == 0:
        raise ValueError("frame_scores: no window scores")
    n = x.size
    covered = (n - 1) * s + frames_per_clip
    nf = covered if n_frames is None else int(n_frames)
    if not 0 < nf <= covered:
        raise ValueError(f"frame_scores: {nf} frames, but {n} windows of {frames_per_clip} at stride {s} cover {covered}")
    f = np.arange(nf)
    lo = np.where(f < frames_per_clip, 0, (f - frames_per_clip) // s + 1)  # first window that reaches frame f
    hi = np.minimum(n - 1, f // s)                                        # last window that starts at or before it
    acc = x[lo].copy()
    for k in range(1, -(-frames_per_clip // s)):  # the k-th further window of every frame that has one
        more = lo + k <= hi
        acc[more] += x[(lo + k)[more]]
    return acc / (hi - lo + 1).astype(np.float32)


def frame_level_auc(preds_per_video, labels_per_video, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                    frame_step: Optional[int] = None) -> Tuple[float, float]:
    """np.repeat(clip scores, 16) vs the frame-level ground truth (runner.py:66-76).  With `clip_stride` < frames_per_clip the
    predictions are scores of overlapping windows, assembled per video by frame_scores; a video whose labels end inside its last
    window (the video's own length rather than the padded one) is cut there.  With `frame_step` d the windows are spans of
    frames_per_clip * d frames (frame_scores): the same, at that span."""
    frames_per_clip = frames_per_clip * _frame_step(frame_step)
    if clip_stride is None or int(clip_stride) == frames_per_clip:
        preds = np.repeat(np.concatenate([np.asarray(p).ravel() for p in preds_per_video]), frames_per_clip)
    else:
        per_video = []
        for p, l in zip(preds_per_video, labels_per_video):
            n, nl = np.asarray(p).size, np.asarray(l).size
            inside = n > 0 and (n - 1) * int(clip_stride) < nl <= (n - 1) * int(clip_stride) + frames_per_clip
            per_video.append(frame_scores(p, frames_per_clip, clip_stride, nl if inside else None))
        preds = np.concatenate(per_video)
    labels = np.concatenate([np.asarray(l).ravel() for l in labels_per_video])
    if preds.shape != labels.shape:
        raise ValueError(f"{preds.shape[0]} repeated predictions vs {labels.shape[0]} frame labels")
    return roc_auc(labels, preds), pr_auc(labels, preds)
