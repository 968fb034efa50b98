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


def roc_auc_from_counts(tps, fps) -> float:
    """The ROC area from the curve's counts: tps[g] / fps[g] positive / negative frames scored at or above the g-th distinct score
    in descending order (what `_ranked` returns, or mil_ops.roc_counts as integers: below 2^53 they are the same float64s, so
    the area has the same bits)."""
    tps, fps = np.asarray(tps, dtype=np.float64), np.asarray(fps, dtype=np.float64)
    tpr = np.concatenate([[0.0], tps]) / tps[-1]
    fpr = np.concatenate([[0.0], fps]) / fps[-1]
    return _area(fpr, tpr)


def pr_auc_from_counts(tps, fps) -> float:
    """The precision-recall area from the same counts."""
    tps, fps = np.asarray(tps, dtype=np.float64), np.asarray(fps, dtype=np.float64)
    precision = np.concatenate([(tps / (tps + fps))[::-1], [1.0]])
    recall = np.concatenate([(tps / tps[-1])[::-1], [0.0]])
    return -_area(recall, precision)


def roc_auc(labels: Sequence[float], preds: Sequence[float]) -> float:
    return roc_auc_from_counts(*_ranked(labels, preds))


def pr_auc(labels: Sequence[float], preds: Sequence[float]) -> float:
    return pr_auc_from_counts(*_ranked(labels, preds))


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


class FrameAucItems:
    """The items of a frame-level curve, host arithmetic only (FrameAucPlan puts them on the device).  Default stride (clip_stride
    None or the span frames_per_clip * frame_step): one item per window, `pos` / `neg` = how many of the window's span frames
    have label > 0.5 / not; video i must have exactly windows * span labels.  clip_stride below the span: one item per frame,
    pos = label > 0.5, neg = 1 - pos, and video i has (windows - 1) * clip_stride + span frames, or as many as it has labels when
    they end inside its last window (frame_level_auc's cut).  A video whose label count fits neither: ValueError with its index."""

    def __init__(self, labels_per_video, windows_per_video, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                 frame_step: Optional[int] = None):
        self.span = int(frames_per_clip) * _frame_step(frame_step)
        self.stride = self.span if clip_stride is None else int(clip_stride)
        if not 1 <= self.stride <= self.span:
            raise ValueError(f"clip_stride {clip_stride} outside [1, {self.span}]")
        self.per_frame = self.stride < self.span
        labels_per_video, self.windows = list(labels_per_video), [int(n) for n in windows_per_video]
        if len(labels_per_video) != len(self.windows) or not self.windows:
            raise ValueError(f"{len(labels_per_video)} label arrays for {len(self.windows)} videos (at least one)")
        pos, self.frames = [], []
        for i, (l, n) in enumerate(zip(labels_per_video, self.windows)):
            y = np.asarray(l, dtype=np.float64).ravel() > 0.5
            if n < 1:
                raise ValueError(f"video {i}: {n} windows")
            covered = (n - 1) * self.stride + self.span
            if not self.per_frame:
                if y.size != covered:
                    raise ValueError(f"video {i}: {y.size} frame labels, but its {n} windows of {self.span} frames cover {covered}")
                pos.append(y.reshape(n, self.span).sum(axis=1))
            else:
                if not (n - 1) * self.stride < y.size <= covered:
                    raise ValueError(f"video {i}: {y.size} frame labels, but its {n} windows of {self.span} frames at stride "
                                     f"{self.stride} cover {covered} (the labels may end inside the last window only)")
                pos.append(y.astype(np.int64))
            self.frames.append(int(y.size))
        self.pos = np.concatenate(pos).astype(np.int32)
        self.neg = ((1 if self.per_frame else self.span) - self.pos).astype(np.int32)
        self.window_offsets = np.concatenate([[0], np.cumsum(self.windows)]).astype(np.int64)
        self.frame_offsets = np.concatenate([[0], np.cumsum(self.frames)]).astype(np.int64)


class FrameAucPlan:
    """frame_level_auc of one fixed test set with the sort and the counting on the device (mil_ops.roc_counts).  Built once:
    labels and geometry do not change between epochs.  Holds a device score buffer of one fp32 per window (`slot(i)`: video i's
    view of it, to be written with the video's window scores), the items' pos / neg counts (FrameAucItems) and the workspace.
    `compute()` -> (rec_auc, pr_auc), equal to metrics.frame_level_auc on the same scores as Python floats: the device returns
    integer counts, the two areas are the host's float64 arithmetic on them.  One synchronisation (roc_counts' read-back) and
    one copy of the compact curve per call.  With clip_stride below the span, compute() first assembles the per-frame scores
    video by video on the device (mil_ops.frame_scores; nothing synchronises).  ValueError: a video whose label count does not
    fit its windows (by index), and NaN / inf scores at compute().  `events(spec)`: the anomaly events of the same scores."""

    def __init__(self, labels_per_video, windows_per_video, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                 frame_step: Optional[int] = None, device="cuda"):
        import torch

        from . import mil_ops

        self.items = it = FrameAucItems(labels_per_video, windows_per_video, frames_per_clip, clip_stride, frame_step)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"FrameAucPlan: device {device!r}: the counts are a HIP kernel (metrics.frame_level_auc is the host path)")
        self.scores = torch.zeros((int(it.window_offsets[-1]),), device=self.device, dtype=torch.float32)
        self.frame_buffer = torch.zeros((int(it.frame_offsets[-1]),), device=self.device, dtype=torch.float32) if it.per_frame else None
        self.pos = torch.from_numpy(it.pos).to(self.device)
        self.neg = torch.from_numpy(it.neg).to(self.device)
        self.workspace = mil_ops.roc_counts_workspace(it.pos.size, self.device)
        self._event_state = None  # events(): (frame scores, smoothed scores, frame offsets, workspace), made on the first call

    def __len__(self) -> int:
        return len(self.items.windows)

    def slot(self, i: int):
        """Video i's window scores: a (windows_i,) view of the score buffer."""
        if not 0 <= i < len(self):
            raise IndexError(f"video {i} of {len(self)}")
        o = self.items.window_offsets
        return self.scores[int(o[i]):int(o[i + 1])]

    def _counts(self):
        from . import mil_ops

        it = self.items
        scores = self.scores
        if it.per_frame:
            scores, fo = self.frame_buffer, it.frame_offsets
            for i in range(len(self)):
                mil_ops.frame_scores(self.slot(i), it.span, it.stride, it.frames[i], out=scores[int(fo[i]):int(fo[i + 1])])
        return mil_ops.roc_counts(scores, self.pos, self.neg, workspace=self.workspace)

    def curve(self):
        """(thresholds fp32, tps int64, fps int64) as numpy: the distinct scores in descending order and the positive / negative
        frames scored at or above each -- the points of the ROC chart, (fps / fps[-1], tps / tps[-1])."""
        return tuple(t.cpu().numpy() for t in self._counts())

    def compute(self) -> Tuple[float, float]:
        import torch

        _, tps, fps = self._counts()
        tps, fps = torch.stack((tps, fps)).cpu().numpy()  # (one copy of the compact curve)
        return roc_auc_from_counts(tps, fps), pr_auc_from_counts(tps, fps)

    def events(self, spec):
        """The anomaly events of the whole test set from the scores in the plan's buffer (events.find_events: moving average,
        two thresholds, gap merge, minimum length) -> events.Events of device tensors, in FRAMES local to each video, equal to
        events.find_events_host on metrics.frame_scores of the same scores.  The per-frame scores are assembled as for the
        AUCs (default stride: np.repeat of all the window scores, one launch; clip_stride below the span: mil_ops.frame_scores
        video by video); the buffers are allocated on the first call.  One synchronisation: the read-back of the number of
        events."""
        import torch

        from . import events, mil_ops

        spec = events.resolve_event_spec(spec)
        if spec is None:
            raise ValueError("FrameAucPlan.events: no event spec")
        it = self.items
        n = int(it.frame_offsets[-1])
        if self._event_state is None:
            frames = self.frame_buffer if it.per_frame else torch.empty((n,), device=self.device, dtype=torch.float32)
            self._event_state = (frames, torch.empty((n,), device=self.device, dtype=torch.float32),
                                 torch.from_numpy(it.frame_offsets).to(self.device), mil_ops.score_events_workspace(n, len(self), self.device))
        frames, smoothed, offsets, workspace = self._event_state
        if it.per_frame:
            fo = it.frame_offsets
            for i in range(len(self)):
                mil_ops.frame_scores(self.slot(i), it.span, it.stride, it.frames[i], out=frames[int(fo[i]):int(fo[i + 1])])
        else:  # every video has windows * span frames: the repeat of the whole buffer is the videos' repeats back to back
            mil_ops.frame_scores(self.scores, it.span, it.span, out=frames)
        return events._find_events_device(frames, offsets, it.frame_offsets, spec, workspace, smoothed)


def frame_level_auc_device(preds_per_video, labels_per_video, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                           frame_step: Optional[int] = None) -> Tuple[float, float]:
    """metrics.frame_level_auc for device score tensors (one fp32 (windows,) CUDA tensor per video) through a throw-away
    FrameAucPlan: == frame_level_auc on the same numbers.  Stricter on the geometry: every video's own label count must fit its
    windows (the host function compares totals only)."""
    preds = [p.reshape(-1) for p in preds_per_video]
    if not preds:
        raise ValueError("frame_level_auc_device: no videos")
    plan = FrameAucPlan(labels_per_video, [p.numel() for p in preds], frames_per_clip, clip_stride, frame_step, device=preds[0].device)
    for i, p in enumerate(preds):
        if not p.is_cuda or p.dtype != plan.scores.dtype:
            raise ValueError(f"frame_level_auc_device: video {i}: expected an fp32 CUDA tensor, got {p.dtype} on {p.device}")
        plan.slot(i).copy_(p)
    return plan.compute()
