"""Live scoring: per-camera feature rings on the device, their sliding windows scored in one padded pass.

    live = LiveScorer(scorer, n_cameras, window=32, ncrops=10, channels=2048, device="cuda:0")
    live.push(cams, feats)      # one new clip (ncrops, channels) for each listed camera
    s = live.score()            # every camera that has a clip: its window's clip scores and its newest clip's score

Every camera keeps its last `window` clips of features, magnitude channel included, in a ring (n_cameras, ncrops, window,
channels + 1); the clip pushed when its camera's count is k lies in slot k % window (`LiveScorer.window_order`).  `push` is
mil_ops.ring_push; `score` is mil_ops.ring_windows into one preallocated padded batch, the scorer's padded pass
(MGFNForVideoAnomalyDetection._score_padded_rows), mil_ops.crop_mean_scatter and mil_ops.crop_mean_last.  A host mirror of the
counts supplies the lengths, and the device vectors of camera ids and lengths are cached by their tuples: once every listed
camera has `window` clips and the calls repeat a camera set, a push + score uploads nothing, synchronises nothing and dispatches
no torch arithmetic.  CUDA tensors only; no fallback.

    live = LiveScorer(scorer, n_cameras, events=EventSpec(low=0.5, high=0.8, smooth=9, merge_gap=2, min_len=4))
    live.score(); live.events.alert; live.events.drain()

With `events=` every score also feeds each listed camera's newest clip score to an events.LiveEventTracker (`live.events`: the
streaming form of events.find_events' rule, one more small launch on `latest` as it is); the steady step still uploads nothing,
synchronises nothing and dispatches no torch arithmetic."""
from __future__ import annotations

from collections import OrderedDict
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import mil_ops
from ._lib import HipExtensionError
from .val_batch import DEFAULT_MAX_ROWS

CACHE_ENTRIES = 64  # camera sets / length tuples kept on the device (least recently used out first)


class LiveScores(NamedTuple):
    cams: Tuple[int, ...]    # the listed cameras
    lens: Tuple[int, ...]    # clips in each one's window, min(count, window)
    scores: torch.Tensor     # (nb, Tmax) fp32: [v, :lens[v]] the window's clip scores, oldest first, 0 behind
    latest: torch.Tensor     # (nb,) fp32: the newest clip's score, scores[v, lens[v] - 1] (a view of `scores` when all lengths agree)


class _Lru:
    def __init__(self, make, entries: int = CACHE_ENTRIES):
        self.make, self.entries, self.items = make, entries, OrderedDict()

    def __call__(self, key):
        if key in self.items:
            self.items.move_to_end(key)
            return self.items[key]
        val = self.items[key] = self.make(key)
        if len(self.items) > self.entries:
            self.items.popitem(last=False)
        return val


class LiveScorer:
    """`scorer`: an MGFNForVideoAnomalyDetection in eval mode on `device`.  `window`: the clips a camera's score looks back over
    (default 32, the T the scorer is trained at).  `max_rows`: the scorer's row limit (val_batch.DEFAULT_MAX_ROWS), which the
    whole state -- n_cameras * ncrops * window rows, one pass when every camera is listed -- has to fit.  `events`: None (nothing
    is built or launched for events), or an event spec (events.resolve_event_spec) for `self.events`, an events.LiveEventTracker
    with a log of `event_log` events per camera: `score` feeds it the newest clip score of every listed camera that has exactly
    one clip more than the tracker has samples of it (a camera scored again without a push is not fed again; one that was pushed
    twice between two scores is refused, its series would miss a sample)."""

    def __init__(self, scorer, n_cameras: int, window: int = 32, ncrops: int = 10, channels: int = 2048, device="cuda:0",
                 max_rows: int = DEFAULT_MAX_ROWS, events=None, event_log: int = 64):
        for name, v in (("n_cameras", n_cameras), ("window", window), ("ncrops", ncrops), ("channels", channels)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise HipExtensionError(f"LiveScorer: {name} = {v!r} is not an integer >= 1 (window < 1 holds no clip)")
        from .events import resolve_event_spec

        try:
            spec = resolve_event_spec(events)
        except ValueError as e:
            raise HipExtensionError(f"LiveScorer: {e}") from None
        if spec is not None and (isinstance(event_log, bool) or not isinstance(event_log, int) or event_log < 1):
            raise HipExtensionError(f"LiveScorer: event_log = {event_log!r} is not an integer >= 1")
        self.scorer = scorer
        self.n_cameras, self.window, self.ncrops, self.channels = int(n_cameras), int(window), int(ncrops), int(channels)
        if self.channels > mil_ops.ADD_MAGNITUDE_NP_MAX_C:
            raise HipExtensionError(f"LiveScorer: channels = {self.channels} above {mil_ops.ADD_MAGNITUDE_NP_MAX_C}: the magnitude channel has numpy's bits up to there")
        rows = self.n_cameras * self.ncrops * self.window
        if rows > int(max_rows):
            raise HipExtensionError(f"LiveScorer: {self.n_cameras} cameras x {self.ncrops} crops x {self.window} clips = {rows} rows is above the "
                                    f"scorer's row limit of {int(max_rows)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HipExtensionError(f"LiveScorer: device '{self.device}': the rings live on the GPU (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        shape = (self.n_cameras, self.ncrops, self.window, self.channels + 1)
        self.ring = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self._counts = torch.zeros((self.n_cameras,), dtype=torch.int64, device=self.device)
        self._host = [0] * self.n_cameras
        self.latest = torch.full((self.n_cameras,), float("nan"), dtype=torch.float32, device=self.device)
        # (never initialised: the rows behind a window hold what an earlier call left there, which the padded pass never reads as values)
        self._batch = torch.empty(shape, dtype=torch.float32, device=self.device).view(-1)
        self._iota = torch.arange(self.n_cameras, dtype=torch.int32).to(self.device)
        self._ids = _Lru(lambda cams: torch.tensor(cams, dtype=torch.int32).to(self.device))  # keyed by checked tuples only
        self._lens = _Lru(self._make_lens)
        self.events = None
        if spec is not None:
            from .events import LiveEventTracker

            self.events = LiveEventTracker(spec, self.n_cameras, log=event_log, device=self.device)

    def _make_lens(self, key):
        from .models.mgfn.modeling_mgfn import PaddedLens

        lens, tmax = key
        return PaddedLens(lens, self.ncrops, tmax, self.device)

    @staticmethod
    def window_order(count: int, W: int) -> Tuple[int, ...]:
        """The slots of a camera's window after `count` pushes into a ring of W, oldest clip first: the clip pushed at count k lies
        in slot k % W, so the last len = min(count, W) clips lie in slots (count - len + t) % W, t = 0 .. len - 1."""
        count, W = int(count), int(W)
        if count < 0 or W < 1:
            raise ValueError(f"window_order: count {count}, W {W}")
        n = min(count, W)
        return tuple((count - n + t) % W for t in range(n))

    @property
    def counts(self) -> torch.Tensor:
        """Clips pushed so far per camera: int64 (n_cameras,) on the device."""
        return self._counts

    @property
    def counts_host(self) -> Tuple[int, ...]:
        """The same numbers on the host, kept by push / reset: nothing is read back."""
        return tuple(self._host)

    def _check_cams(self, cams, what: str) -> Tuple[int, ...]:
        if type(cams) is tuple and all(type(c) is int for c in cams) and cams in self._ids.items:
            return cams  # (a camera set seen before was checked then)
        try:
            cams = tuple(cams)
        except TypeError:
            raise HipExtensionError(f"{what}: cams must be a sequence of camera ids, got {type(cams).__name__}") from None
        if not cams:
            raise HipExtensionError(f"{what}: an empty list of cameras")
        for c in cams:
            if isinstance(c, bool) or torch.is_tensor(c) or int(c) != c:
                raise HipExtensionError(f"{what}: camera id {c!r} is not a host integer")
            if not 0 <= int(c) < self.n_cameras:
                raise HipExtensionError(f"{what}: camera id {int(c)} is out of range [0, {self.n_cameras})")
        cams = tuple(int(c) for c in cams)
        if len(set(cams)) != len(cams):
            dup = sorted(c for c in set(cams) if cams.count(c) > 1)
            raise HipExtensionError(f"{what}: duplicate camera ids {dup}: one clip per camera and call")
        return cams

    def push(self, cams: Sequence[int], feats: torch.Tensor) -> None:
        """One new clip for each camera of `cams` (distinct host ints): feats (len(cams), ncrops, channels) fp32 on the device."""
        cams = self._check_cams(cams, "LiveScorer.push")
        want = (len(cams), self.ncrops, self.channels)
        if not torch.is_tensor(feats) or tuple(feats.shape) != want:
            raise HipExtensionError(f"LiveScorer.push: feats must be {want} (cameras, crops, channels), got {tuple(getattr(feats, 'shape', ()))}")
        mil_ops.ring_push(feats, self._ids(cams), self.ring, self._counts)
        for c in cams:
            self._host[c] += 1

    def score(self, cams: Optional[Sequence[int]] = None) -> LiveScores:
        """The windows of the listed cameras (None: every camera with at least one clip, ascending) scored in one padded pass."""
        if cams is None:
            cams = tuple(c for c, k in enumerate(self._host) if k > 0)
            if not cams:
                raise HipExtensionError("LiveScorer.score: no camera has a clip yet")
        else:
            cams = self._check_cams(cams, "LiveScorer.score")
            empty = [c for c in cams if self._host[c] == 0]
            if empty:
                raise HipExtensionError(f"LiveScorer.score: cameras {empty} have no clip yet")
        feed = None
        if self.events is not None:  # which of the listed cameras have a new clip for the tracker: decided before anything is launched
            fed = self.events._host
            ahead = [c for c in cams if self._host[c] > fed[c] + 1]
            if ahead:
                raise HipExtensionError(f"LiveScorer.score: cameras {ahead} are more than one clip ahead of their event series (pushed twice, scored "
                                        f"once): every clip's score is a sample; score after every push, or reset the cameras")
            feed = tuple(c for c in cams if self._host[c] == fed[c] + 1)
        lens = tuple(min(self._host[c], self.window) for c in cams)
        nb, tmax = len(cams), max(lens)
        ids, pl = self._ids(cams), self._lens((lens, tmax))
        video = self._batch[: nb * self.ncrops * tmax * (self.channels + 1)].view(nb, self.ncrops, tmax, self.channels + 1)
        mil_ops.ring_windows(self.ring, self._counts, ids, video)
        rows, _ = self.scorer._score_padded_rows(video, pl)
        scores = torch.zeros((nb, tmax), dtype=torch.float32, device=self.device)
        mil_ops.crop_mean_scatter(rows, pl.video_lens, pl.dense_offsets, scores, nb, self.ncrops)
        mil_ops.crop_mean_last(rows, pl.video_lens, ids, self.latest, self.ncrops)
        if feed:
            self.events.update(feed, self.latest, by_camera=True)
        if min(lens) == tmax:  # the newest clips are one column of the scores (the same sum, the same bits): a view of it
            latest = scores[:, tmax - 1]
        else:
            latest = mil_ops.crop_mean_last(rows, pl.video_lens, self._iota[:nb], torch.empty((nb,), dtype=torch.float32, device=self.device), self.ncrops)
        return LiveScores(cams, lens, scores, latest)

    def reset(self, cams: Sequence[int]) -> None:
        """The listed cameras start over: count 0, latest NaN (their rings' old clips can no longer be reached).  With `events`
        their event series start over too, an open event is dropped: call `self.events.finish(cams)` first to keep it."""
        cams = self._check_cams(cams, "LiveScorer.reset")
        if self.events is not None:
            self.events.reset(cams)
        idx = self._ids(cams).long()
        self._counts[idx] = 0
        self.latest[idx] = float("nan")
        for c in cams:
            self._host[c] = 0

    def step_frames(self, backbone, frames_u8: torch.Tensor, cams: Sequence[int], **sampling) -> LiveScores:
        """One clip per camera straight from resized uint8 frames: `frames_u8` (len(cams) * span, FH, FW, 3) on the device holds
        the cameras' clips back to back in `cams` order (span = frames_per_clip * frame_step frames each); `sampling` are
        I3Res50.forward_frames' arguments (frames_per_clip, crop, crops, frame_step, normalize), with len(crops) = ncrops.
        -> backbone.forward_frames, `push`, `score(cams)`."""
        from . import ops

        cams = self._check_cams(cams, "LiveScorer.step_frames")
        fpc = sampling.get("frames_per_clip", 16)
        s, crops, d = ops.resolve_sampling(fpc, sampling.get("clip_stride"), sampling.get("crops"), sampling.get("frame_step"))
        if s != fpc * d:
            raise HipExtensionError(f"LiveScorer.step_frames: clip_stride {s} is not the clip's span {fpc * d}: the cameras' clips lie back to back")
        if len(crops) != self.ncrops:
            raise HipExtensionError(f"LiveScorer.step_frames: {len(crops)} crops, the rings hold {self.ncrops}")
        if not torch.is_tensor(frames_u8) or frames_u8.dim() != 4 or frames_u8.shape[0] != len(cams) * fpc * d:
            raise HipExtensionError(f"LiveScorer.step_frames: frames_u8 must be ({len(cams) * fpc * d}, FH, FW, 3): {fpc * d} frames for each of "
                                    f"{len(cams)} cameras, got {tuple(getattr(frames_u8, 'shape', ()))}")
        feats = backbone.forward_frames(frames_u8, 0, len(cams) * self.ncrops, **sampling)
        if feats.numel() != len(cams) * self.ncrops * self.channels:
            raise HipExtensionError(f"LiveScorer.step_frames: the backbone's features are {tuple(feats.shape)}, the rings hold {self.channels} channels")
        self.push(cams, feats.reshape(len(cams), self.ncrops, self.channels))
        return self.score(cams)
