"""Anomaly events from per-frame scores: moving average, two thresholds with hysteresis, gap merge, minimum length.

The rule (this package's definition; include/advhip.h restates it for the kernels).  For one video's scores x of L frames:

1. smooth    window w odd in [1, 1023], h = (w - 1) / 2: y[t] = sum(x[max(0, t - h) .. min(L - 1, t + h)]) / count, the sum in fp32
             in ascending order from +0.0, one fp32 division by the count.
2. flags     active = y >= low, strong = y >= high (thresholds rounded to fp32; a NaN is neither).
3. candidates  maximal runs of active frames; runs at most merge_gap inactive frames apart are one candidate, as a chain.
4. keep      a candidate with at least one strong frame and end - start >= min_len.
5. record    video, start, end (exclusive), peak (largest y, NaN ignored), peak_frame (its first frame), mean (float64 sum of
             y[start:end] / length, rounded to fp32; gap frames included).

`find_events` runs it on the device for a ragged batch (mil_ops.smooth_scores + mil_ops.score_events: one read-back),
`find_events_host` is the same rule in vectorised numpy: the stated host definition, as metrics.frame_level_auc is for the AUCs.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

MAX_SMOOTH = 1023


@dataclass(frozen=True)
class EventSpec:
    low: float
    high: float
    smooth: int = 1
    merge_gap: int = 0
    min_len: int = 1


_FIELDS = ("low", "high", "smooth", "merge_gap", "min_len")


def _integer(name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"events: {name}={v!r} is not an integer")
    return int(v)


def resolve_event_spec(spec) -> Optional[EventSpec]:
    """None -> None (the feature is off); an EventSpec, a mapping with the keys low, high[, smooth, merge_gap, min_len] or a
    tuple in that order -> a checked EventSpec.  Refuses, naming the field, whatever the kernels' entry points refuse: a
    threshold that is not finite, low > high, an even smooth or one outside [1, 1023], merge_gap < 0, min_len < 1."""
    if spec is None:
        return None
    if isinstance(spec, EventSpec):
        kw = {k: getattr(spec, k) for k in _FIELDS}
    elif hasattr(spec, "keys"):
        kw = {k: spec[k] for k in spec.keys()}
        unknown = sorted(set(kw) - set(_FIELDS))
        if unknown:
            raise ValueError(f"events: unknown key(s) {unknown}; the keys are {list(_FIELDS)}")
    elif isinstance(spec, (tuple, list)):
        if not 2 <= len(spec) <= len(_FIELDS):
            raise ValueError(f"events: a tuple holds (low, high[, smooth, merge_gap, min_len]), got {len(spec)} values")
        kw = dict(zip(_FIELDS, spec))
    else:
        raise ValueError(f"events: expected a mapping, a tuple or an EventSpec, got {type(spec).__name__}")
    for name in ("low", "high"):
        if name not in kw:
            raise ValueError(f"events: {name} is missing")
        v = kw[name]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"events: {name}={v!r} is not a finite number")
        if abs(float(v)) > float(np.finfo(np.float32).max):
            raise ValueError(f"events: {name}={v!r} is not finite in fp32")
    low, high = float(kw["low"]), float(kw["high"])
    if low > high:
        raise ValueError(f"events: low={low} is above high={high}")
    smooth = _integer("smooth", kw.get("smooth", 1))
    if not 1 <= smooth <= MAX_SMOOTH or smooth % 2 == 0:
        raise ValueError(f"events: smooth={smooth} is not an odd window in [1, {MAX_SMOOTH}]")
    merge_gap = _integer("merge_gap", kw.get("merge_gap", 0))
    if not 0 <= merge_gap < 1 << 31:
        raise ValueError(f"events: merge_gap={merge_gap} outside [0, 2^31)")
    min_len = _integer("min_len", kw.get("min_len", 1))
    if not 1 <= min_len < 1 << 31:
        raise ValueError(f"events: min_len={min_len} outside [1, 2^31)")
    return EventSpec(low, high, smooth, merge_gap, min_len)


class Events:
    """The events of a ragged batch, E rows in (video, start) order: `video`, `start`, `end` (exclusive), `peak_frame` int32 and
    `peak`, `mean` fp32, all (E,), frames local to the video; `counts` int32 (V,) events per video.  The fields are device
    tensors (find_events) or numpy arrays (find_events_host, .numpy()); len() is E."""

    FIELDS = ("video", "start", "end", "peak_frame", "peak", "mean")

    def __init__(self, ev_int, ev_f, counts):
        self.ev_int, self.ev_f, self.counts = ev_int, ev_f, counts  # (E, 4), (E, 2), (V,)

    video = property(lambda self: self.ev_int[:, 0])
    start = property(lambda self: self.ev_int[:, 1])
    end = property(lambda self: self.ev_int[:, 2])
    peak_frame = property(lambda self: self.ev_int[:, 3])
    peak = property(lambda self: self.ev_f[:, 0])
    mean = property(lambda self: self.ev_f[:, 1])

    def __len__(self) -> int:
        return int(self.ev_int.shape[0])

    @property
    def on_host(self) -> bool:
        return isinstance(self.ev_int, np.ndarray)

    def numpy(self) -> "Events":
        """The same events as numpy arrays (three device-to-host copies; self when they already are)."""
        if self.on_host:
            return self
        return Events(self.ev_int.cpu().numpy(), self.ev_f.cpu().numpy(), self.counts.cpu().numpy())

    def per_video(self, i: int) -> "Events":
        """Video i's events (views of the rows; on device tensors the row range is read from `counts`: one read-back)."""
        v = int(self.counts.shape[0])
        if not 0 <= i < v:
            raise IndexError(f"video {i} of {v}")
        first = int(self.counts[:i].sum())
        n = int(self.counts[i])
        return Events(self.ev_int[first:first + n], self.ev_f[first:first + n], self.counts[i:i + 1])

    def to_seconds(self, fps: float) -> dict:
        """Host arithmetic: {video, start, end, peak_time (float64 seconds = frame / fps), peak, mean} as numpy arrays."""
        fps = float(fps)
        if not fps > 0 or not math.isfinite(fps):
            raise ValueError(f"to_seconds: fps={fps!r} is not a positive number")
        h = self.numpy()
        return {"video": h.video.copy(), "start": h.start / fps, "end": h.end / fps, "peak_time": h.peak_frame / fps,
                "peak": h.peak.copy(), "mean": h.mean.copy()}


def _host_offsets(lengths, n: int) -> np.ndarray:
    lengths = np.asarray(lengths)
    if lengths.ndim != 1 or lengths.size < 1 or lengths.dtype.kind not in "iu":
        raise ValueError(f"events: lengths must be a non-empty 1-D sequence of integers, got {lengths.dtype} {lengths.shape}")
    lengths = lengths.astype(np.int64)
    if (lengths < 0).any() or int(lengths.sum()) != n:
        raise ValueError(f"events: {lengths.size} lengths that sum to {int(lengths.sum())} for {n} scores (none negative)")
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def smooth_host(x: np.ndarray, offsets: np.ndarray, window: int) -> np.ndarray:
    """Step 1 of the rule on a flat fp32 array: one vector add per window offset, in ascending order."""
    n, h = x.size, (window - 1) // 2
    lengths = np.diff(offsets)
    start = np.repeat(offsets[:-1], lengths)
    end = np.repeat(offsets[1:], lengths)
    t = np.arange(n, dtype=np.int64)
    acc = np.zeros(n, dtype=np.float32)
    count = np.zeros(n, dtype=np.int64)
    for k in range(-h, h + 1):
        ok = (t + k >= start) & (t + k < end)
        acc[ok] += x[t[ok] + k]
        count += ok
    return acc / count.astype(np.float32)


def find_events_host(scores, lengths, spec) -> Events:
    """The rule in vectorised numpy for a ragged batch: `scores` (N,) holds the videos back to back, `lengths` their frame
    counts (0 allowed).  -> Events of numpy arrays.  What find_events computes on the device: integers, peaks and counts equal,
    means equal up to the order of the float64 sum (at most one fp32 ulp on non-negative scores)."""
    spec = resolve_event_spec(spec)
    if spec is None:
        raise ValueError("find_events_host: no event spec")
    x = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).ravel())
    n = x.size
    offsets = _host_offsets(lengths, n)
    v = offsets.size - 1
    empty = Events(np.zeros((0, 4), np.int32), np.zeros((0, 2), np.float32), np.zeros(v, np.int32))
    if n == 0:
        return empty
    with np.errstate(invalid="ignore", over="ignore"):
        y = smooth_host(x, offsets, spec.smooth)
        active = y >= np.float32(spec.low)
        strong = y >= np.float32(spec.high)
    lens = np.diff(offsets)
    vstart = np.repeat(offsets[:-1], lens)
    vend = np.repeat(offsets[1:], lens)
    t = np.arange(n, dtype=np.int64)
    # the nearest active frame strictly before / after every frame (-1 / n: none); videos are contiguous, so "inside my
    # video" is a comparison with its bounds
    last = np.maximum.accumulate(np.where(active, t, -1))
    prev = np.concatenate([[-1], last[:-1]])
    nxt_incl = np.minimum.accumulate(np.where(active, t, n)[::-1])[::-1]
    nxt = np.concatenate([nxt_incl[1:], [n]])
    g = spec.merge_gap
    starts = np.flatnonzero(active & (prev < np.maximum(vstart, t - g - 1)))
    ends = np.flatnonzero(active & (nxt > np.minimum(vend - 1, t + g + 1))) + 1
    if starts.size == 0:
        return empty
    # candidate k = [starts[k], ends[k]); s0 < e0 < s1 < e1 ...: reduceat over the interleaved bounds, every other segment
    # (one pad element so that an end at N is an index)
    bounds = np.stack([starts, ends], axis=1).ravel()
    pad = lambda a, fill: np.concatenate([a, np.array([fill], dtype=a.dtype)])
    y_max = np.where(np.isnan(y), np.float32(-np.inf), y)
    peak = np.maximum.reduceat(pad(y_max, np.float32(-np.inf)), bounds)[::2]
    any_strong = np.maximum.reduceat(pad(strong.astype(np.int8), 0), bounds)[::2] > 0
    with np.errstate(invalid="ignore"):
        total = np.add.reduceat(pad(y.astype(np.float64), 0.0), bounds)[::2]
        mean = (total / (ends - starts)).astype(np.float32)
    # the first frame of each candidate that holds its peak
    clen = ends - starts
    first = np.concatenate([[0], np.cumsum(clen)[:-1]])
    cid = np.repeat(np.arange(starts.size), clen)
    pos = np.arange(int(clen.sum()), dtype=np.int64) - np.repeat(first, clen) + np.repeat(starts, clen)
    peak_at = np.minimum.reduceat(np.where(y_max[pos] == peak[cid], pos, n), first)
    peak = y[peak_at]  # (the copied float: of -0.0 and +0.0, the one that comes first)
    keep = any_strong & (clen >= spec.min_len)
    video = np.searchsorted(offsets, starts, side="right") - 1  # (steps over videos of length 0)
    base = offsets[video]
    ev_int = np.stack([video, starts - base, ends - base, peak_at - base], axis=1)[keep].astype(np.int32)
    ev_f = np.stack([peak, mean], axis=1)[keep].astype(np.float32)
    counts = np.bincount(video[keep], minlength=v).astype(np.int32)
    return Events(ev_int.reshape(-1, 4), ev_f.reshape(-1, 2), counts)


def find_events(scores, lengths_or_offsets, spec, workspace=None, smoothed=None) -> Events:
    """The rule on the device for a ragged batch: `scores` a contiguous fp32 CUDA (N,) tensor holding the videos back to back.
    `lengths_or_offsets`: the videos' frame counts as a host sequence of V integers (0 allowed), or their offsets as an int64
    CUDA (V + 1,) tensor (read back once to check them and to size the event list).  -> Events of device tensors.  Two kernels'
    worth of launches (mil_ops.smooth_scores, mil_ops.score_events) and ONE read-back, of the number of events.
    `workspace`: mil_ops.score_events_workspace(N, V, device) to reuse; `smoothed`: an fp32 (N,) buffer for the smoothed curve."""
    import torch

    spec = resolve_event_spec(spec)
    if spec is None:
        raise ValueError("find_events: no event spec")
    if not torch.is_tensor(scores) or scores.dim() != 1:
        raise ValueError("find_events: scores must be a 1-D fp32 CUDA tensor")
    n = int(scores.shape[0])
    if torch.is_tensor(lengths_or_offsets) and lengths_or_offsets.is_cuda:
        offsets, host = lengths_or_offsets, None
    else:
        lengths = lengths_or_offsets.numpy() if torch.is_tensor(lengths_or_offsets) else lengths_or_offsets
        host = _host_offsets(lengths, n)
        if n == 0:
            return _empty_device(scores.device, host.size - 1)
        offsets = torch.from_numpy(host).to(scores.device)
    return _find_events_device(scores, offsets, host, spec, workspace, smoothed)


def _empty_device(device, v: int) -> Events:
    import torch

    return Events(torch.zeros((0, 4), device=device, dtype=torch.int32), torch.zeros((0, 2), device=device, dtype=torch.float32),
                  torch.zeros((v,), device=device, dtype=torch.int32))


def _find_events_device(scores, offsets, offsets_host, spec: EventSpec, workspace=None, smoothed=None) -> Events:
    from . import mil_ops

    y = mil_ops.smooth_scores(scores, offsets, spec.smooth, out=smoothed)
    return Events(*mil_ops.score_events(y, offsets, spec.low, spec.high, spec.merge_gap, spec.min_len, workspace=workspace,
                                        offsets_host=offsets_host))


def live_emission_count(end: int, spec) -> int:
    """The sample count at which a live camera emits the event that ends (exclusive) at `end`: end + merge_gap + h + 1 with
    h = (smooth - 1) / 2.  The candidate closes at the first final y more than merge_gap behind its last active sample, position
    end + merge_gap, and y[t] is final once sample t + h has been fed.  An event still open at `finish` is emitted there."""
    spec = resolve_event_spec(spec)
    if spec is None:
        raise ValueError("live_emission_count: no event spec")
    end = _integer("end", end)
    if end < 1:
        raise ValueError(f"events: end={end} below 1 (an event holds a sample)")
    return end + spec.merge_gap + (spec.smooth - 1) // 2 + 1


MAX_LIVE_SAMPLES = (1 << 31) - 1  # positions are int32: a camera is finished or reset before it has fed this many samples


class LiveDrain(NamedTuple):
    events: Events          # the events emitted since the previous drain, per camera and in emission order; video = the camera id
    generation: object      # int32 (E,): the camera's generation when each event was emitted (finish and reset add one)
    lost: np.ndarray        # int64 (n_cameras,): events of each camera overwritten in its log before they were drained


class LiveEventTracker:
    """The event rule, streaming, for `n_cameras` independent score series on the device (include/advhip.h: live events; one
    launch of mil_ops.live_events_update per call).  The events a camera emits while it runs plus what `finish` closes are
    `find_events_host`'s events of its whole series, and the event [s, e) is emitted by the update that brings the camera's sample
    count to `live_emission_count(e, spec)`.  `log`: the events kept per camera between two drains.

    `alert` (1 iff a candidate is open, strong and at least min_len long), `open_start` (its start, or -1), `emitted` and
    `samples` are device tensors; `samples_host` is the host's mirror of the last.  `cams` are checked and their id
    tensors cached by `self.cameras`, a live.CameraSet: a repeated camera set uploads nothing.  `cameras`: the CameraSet of the same
    cameras whose id cache to share (LiveScorer passes its own; the sample counts stay the tracker's).  CUDA only; no fallback."""

    def __init__(self, spec, n_cameras: int, log: int = 64, device="cuda:0", cameras=None):
        from . import mil_ops
        from ._lib import HipExtensionError
        from .live import CameraSet, host_int

        try:
            self.spec = resolve_event_spec(spec)
        except ValueError as e:
            raise HipExtensionError(f"LiveEventTracker: {e}") from None
        if self.spec is None:
            raise HipExtensionError("LiveEventTracker: no event spec")
        for name, v in (("n_cameras", n_cameras), ("log", log)):
            if (k := host_int(v, floats=False)) is None or not 1 <= k < 1 << 31:
                raise HipExtensionError(f"LiveEventTracker: {name} = {v!r} is not an integer in [1, 2^31)")
        self.n_cameras, self.log = int(n_cameras), int(log)
        self.cameras = CameraSet(self.n_cameras, device, "sample", share=cameras)
        self.device = self.cameras.device
        if self.device.type != "cuda":
            raise HipExtensionError(f"LiveEventTracker: device '{self.device}': the state lives on the GPU (there is no CPU fallback)")
        self.state = mil_ops.live_events_state(self.n_cameras, self.spec.smooth, self.log, self.device)
        self._drained = np.zeros(self.n_cameras, dtype=np.int64)

    alert = property(lambda self: self.state["alert"])
    open_start = property(lambda self: self.state["open_start"])
    emitted = property(lambda self: self.state["emitted"])
    samples = property(lambda self: self.state["samples"])

    @property
    def samples_host(self) -> tuple:
        """Samples fed per camera since its last finish / reset, kept by update / finish / reset: nothing is read back."""
        return tuple(self.cameras.host)

    def _launch(self, ids, scores, by_camera: bool, mode: int) -> None:
        from . import mil_ops

        s = self.spec
        mil_ops.live_events_update(scores, ids, self.state, s.low, s.high, s.smooth, s.merge_gap, s.min_len, by_camera, mode)

    def update(self, cams, scores, by_camera: bool = False) -> None:
        """One new sample for each camera of `cams` (distinct host ints): scores fp32 on the device, (len(cams),) in `cams` order,
        or with by_camera (n_cameras,) indexed by camera id (LiveScorer.latest as it is)."""
        from ._lib import LIVE_EVENTS_UPDATE, HipExtensionError

        cams = self.cameras.check(cams, "LiveEventTracker.update")
        full = [c for c in cams if self.cameras.host[c] >= MAX_LIVE_SAMPLES]
        if full:
            raise HipExtensionError(f"LiveEventTracker.update: cameras {full} have fed 2^31 - 1 samples (positions are int32): finish or reset them")
        self._launch(self.cameras.ids(cams), scores, bool(by_camera), LIVE_EVENTS_UPDATE)
        self.cameras.bump(cams)

    def finish(self, cams) -> None:
        """The listed cameras' series end here: their pending (smooth - 1) / 2 samples are finalised as at a video's end, an open
        event is closed and emitted if it qualifies, then the cameras start over (samples 0, generation + 1)."""
        from ._lib import LIVE_EVENTS_FINISH

        self._clear(cams, "LiveEventTracker.finish", LIVE_EVENTS_FINISH)

    def reset(self, cams) -> None:
        """The listed cameras start over without emitting: samples 0, generation + 1, an open candidate is dropped."""
        from ._lib import LIVE_EVENTS_RESET

        self._clear(cams, "LiveEventTracker.reset", LIVE_EVENTS_RESET)

    def _clear(self, cams, what: str, mode: int) -> None:
        cams = self.cameras.check(cams, what)
        self._launch(self.cameras.ids(cams), None, False, mode)
        self.cameras.clear(cams)

    def drain(self) -> LiveDrain:
        """The events emitted since the previous drain: ONE read-back (of `emitted`), then one gather of their log rows on the
        device.  -> LiveDrain(events, generation, lost): `events` an Events of device tensors, camera by camera in emission
        order, video = the camera id, counts int32 (n_cameras,); `generation` int32 (E,) on the device; `lost` int64
        (n_cameras,) on the host: how many of a camera's events were overwritten in its log (more than `log` since the
        previous drain) and are not among `events`."""
        import torch

        emitted = self.state["emitted"].cpu().numpy()
        new = emitted - self._drained
        lost = np.maximum(new - self.log, 0)
        kept = (new - lost).astype(np.int64)
        cam = np.repeat(np.arange(self.n_cameras, dtype=np.int64), kept)
        first = np.repeat(emitted - kept, kept)                                    # the number of each camera's oldest kept event
        within = np.arange(int(kept.sum()), dtype=np.int64) - np.repeat(np.cumsum(kept) - kept, kept)
        rows = cam * self.log + (first + within) % self.log
        self._drained = emitted.copy()
        counts = torch.from_numpy(kept.astype(np.int32)).to(self.device)
        idx = torch.from_numpy(np.stack([rows, cam])).to(self.device)
        ev_int = self.state["log_int"].view(-1, 4).index_select(0, idx[0])
        ev_f = self.state["log_f"].view(-1, 2).index_select(0, idx[0])
        generation = ev_int[:, 0].clone()
        ev_int[:, 0] = idx[1].to(torch.int32)
        return LiveDrain(Events(ev_int, ev_f, counts), generation, lost)


def video_events(window_scores, spec, frames_per_clip: int = 16, clip_stride: Optional[int] = None, frame_step: Optional[int] = None,
                 n_frames: Optional[int] = None) -> Events:
    """One video's events from its window scores (fp32 CUDA (n_windows,)): mil_ops.frame_scores, then find_events on the frames."""
    from . import mil_ops

    frames = mil_ops.frame_scores(window_scores.reshape(-1), frames_per_clip, clip_stride, n_frames, frame_step)
    return find_events(frames, [int(frames.shape[0])], spec)
