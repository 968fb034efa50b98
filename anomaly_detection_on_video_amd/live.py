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
synchronises nothing and dispatches no torch arithmetic.

    lf = LiveFrames(n_cameras, frame_hw=(256, 340), frames_per_clip=16, clip_stride=8)
    live.step_camera_frames(backbone, lf, cams, frames, resize=256, crops="center_flip")   # None until a clip is due

`LiveFrames` is the front end: per-camera rings of the last `span` resized uint8 frames, one decoded frame per camera and push,
and the clips that are due gathered in one launch into the buffer I3Res50.forward_frames reads -- each one window w of the
camera's frames as an offline video, byte for byte.

    lf = LiveFrames(n_cameras, ..., motion=MotionGate(pixel_delta=6, max_changed=0.002))   # (numbers for illustration only)

`motion=` adds a per-camera motion gate on the device (include/advhip.h: "live frames: motion gate"); the default, None,
allocates and launches nothing.  THE RULE: every camera has an anchor frame and a row {still, epoch, changed, peak}, at first
{-1, 0, -1, 0}.  For a pushed frame f (at ring size), n = the byte positions with |f[i] - anchor[i]| > pixel_delta, compared as
integers (both signs count, |d| == pixel_delta is not changed).  Without an anchor (still == -1) or with n > limit the frame
MOVES: anchor := f, still := 0, epoch += 1, peak := 0, changed := n (-1 without an anchor).  Otherwise it is STILL: still :=
min(still + 1, 2^30), changed := n, peak := max(peak, n), the anchor stays.  A due window is QUIET iff still + 1 >= span: all its
frames lie within the tolerance of one anchor frame.  `gate_decision`, on the host, from the one read-back of {still, epoch}: a
quiet window is HELD iff ref_epoch[c] == epoch and (max_hold is None or holds[c] < max_hold), and then holds[c] += 1; an
extracted quiet window does ref_epoch[c] := epoch, holds[c] := 0; an extracted window that is not quiet does ref_epoch[c] :=
None, holds[c] := 0.  So the first quiet window after any motion is always extracted (the reference of the still scene), only
later quiet windows under the same anchor repeat it (`LiveScorer.hold`: the camera's newest clip row again, bit for bit), a
clip that contains motion is never repeated, and slow drift, measured against the fixed anchor, eventually moves.  `reset` does
still := -1, epoch += 1 and clears ref_epoch[c] and holds[c].

All three classes (and events.LiveEventTracker) keep their cameras in one `CameraSet`: the rule for `cams`, the cached id vectors,
the host mirror of the counts."""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
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


def host_int(v, floats: bool = True) -> Optional[int]:
    """`v` as an int where it is an integer-valued host number -- never a bool, a tensor or a string; floats=False: of an integer
    type -- else None.  The bounds and the message are the caller's."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer) + ((float, np.floating) if floats else ())):
        return None
    return int(v) if isinstance(v, (int, np.integer)) or float(v).is_integer() else None


def _resolve_device(device) -> torch.device:
    """A bare "cuda" means the current device.  Whether anything but a GPU will do is the caller's to say."""
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


class CameraSet:
    """The cameras of one live object: how many and on which device, the one rule for the `cams` of a call (`check`), the device
    vectors of checked id tuples (`ids`, an LRU cache of CACHE_ENTRIES) and the host mirror of a per-camera count (`host`, moved by
    `bump` and `clear` only).  `unit` names what a call brings each listed camera: a frame, a clip, a sample.  `share`: a
    CameraSet of the same cameras whose id cache this one uses -- a tuple is then uploaded once for both; the counts stay apart."""

    def __init__(self, n_cameras: int, device, unit: str, share: Optional["CameraSet"] = None):
        self.n_cameras, self.device, self.unit = n_cameras, _resolve_device(device), unit
        if share is not None and (share.n_cameras, share.device) != (self.n_cameras, self.device):
            raise HipExtensionError(f"CameraSet: {share.n_cameras} cameras on {share.device} share no ids with {self.n_cameras} on {self.device}")
        self.host = [0] * n_cameras
        # (keyed by checked tuples only)
        self.ids = share.ids if share is not None else _Lru(lambda cams: torch.tensor(cams, dtype=torch.int32).to(self.device))

    def check(self, cams, what: str) -> Tuple[int, ...]:
        """`cams` as a tuple of distinct host ints in [0, n_cameras), or a refusal that starts with `what`."""
        if type(cams) is tuple and all(type(c) is int for c in cams) and cams in self.ids.items:
            return cams  # (a camera set seen before was checked then)
        if torch.is_tensor(cams) or isinstance(cams, np.ndarray):
            raise HipExtensionError(f"{what}: cams must be a sequence of host integers, got a {type(cams).__name__} (the ids are checked on the host)")
        try:
            cams = tuple(cams)
        except TypeError:
            raise HipExtensionError(f"{what}: cams must be a sequence of camera ids, got {type(cams).__name__}") from None
        if not cams:
            raise HipExtensionError(f"{what}: an empty list of cameras")
        for c in cams:
            if host_int(c) is None:
                raise HipExtensionError(f"{what}: camera id {c!r} is not a host integer")
            if not 0 <= int(c) < self.n_cameras:
                raise HipExtensionError(f"{what}: camera id {int(c)} is out of range [0, {self.n_cameras})")
        cams = tuple(int(c) for c in cams)
        if len(set(cams)) != len(cams):
            dup = sorted(c for c in set(cams) if cams.count(c) > 1)
            raise HipExtensionError(f"{what}: duplicate camera ids {dup}: one {self.unit} per camera and call")
        return cams

    def bump(self, cams) -> None:
        for c in cams:
            self.host[c] += 1

    def clear(self, cams) -> None:
        for c in cams:
            self.host[c] = 0


@dataclass(frozen=True)
class MotionGate:
    """The motion gate's numbers (the module docstring has the rule).  `pixel_delta`: how far a byte may lie from the anchor's and
    still count as unchanged, an int in [0, 255].  `max_changed`: how many changed bytes a still frame may have -- an int >= 0
    (bytes) or a float in [0, 1] (a share of frame_bytes; `limit` floors it once).  `max_hold`: None, or how many windows in a
    row may repeat one reference before the next quiet window is extracted again, an int >= 1.  pixel_delta and max_changed have
    NO defaults: what suits a real camera (sensor noise, compression, auto-exposure) has not been measured by anybody."""
    pixel_delta: int
    max_changed: Union[int, float]
    max_hold: Optional[int] = None

    def __post_init__(self):
        tau, mc, mh = self.pixel_delta, self.max_changed, self.max_hold
        if host_int(tau, floats=False) is None:
            raise ValueError(f"motion: pixel_delta={tau!r} is not an integer")
        if not 0 <= int(tau) <= 255:
            raise ValueError(f"motion: pixel_delta={int(tau)} outside [0, 255]")
        if isinstance(mc, bool) or not isinstance(mc, (int, float, np.integer, np.floating)):
            raise ValueError(f"motion: max_changed={mc!r} is neither an integer (bytes) nor a float (a share of the frame)")
        if isinstance(mc, (float, np.floating)):
            if not math.isfinite(float(mc)):
                raise ValueError(f"motion: max_changed={mc!r} is not finite")
            if float(mc) < 0:
                raise ValueError(f"motion: max_changed={mc!r} is negative")
            if float(mc) > 1:
                raise ValueError(f"motion: max_changed={mc!r} is a share above 1 (an integer counts bytes)")
            mc = float(mc)
        else:
            if int(mc) < 0:
                raise ValueError(f"motion: max_changed={int(mc)} is negative")
            mc = int(mc)
        if mh is not None:
            if host_int(mh, floats=False) is None:
                raise ValueError(f"motion: max_hold={mh!r} is neither None nor an integer")
            if int(mh) < 1:
                raise ValueError(f"motion: max_hold={int(mh)} is below 1")
            mh = int(mh)
        for name, v in (("pixel_delta", int(tau)), ("max_changed", mc), ("max_hold", mh)):
            object.__setattr__(self, name, v)

    def limit(self, frame_bytes: int) -> int:
        """The changed bytes a still frame may have: max_changed itself (at most frame_bytes), or floor(share * frame_bytes)."""
        if isinstance(self.max_changed, float):
            return min(int(math.floor(self.max_changed * frame_bytes)), frame_bytes)
        return min(self.max_changed, frame_bytes)


_GATE_FIELDS = ("pixel_delta", "max_changed", "max_hold")


def resolve_motion_gate(spec) -> Optional[MotionGate]:
    """None -> None (the gate is off); a MotionGate, a mapping with the keys pixel_delta, max_changed[, max_hold] or a tuple in
    that order -> a checked MotionGate.  Refuses with a ValueError that names the field."""
    if spec is None:
        return None
    if isinstance(spec, MotionGate):
        return spec
    if hasattr(spec, "keys"):
        kw = {k: spec[k] for k in spec.keys()}
        unknown = sorted(set(kw) - set(_GATE_FIELDS))
        if unknown:
            raise ValueError(f"motion: unknown key(s) {unknown}; the keys are {list(_GATE_FIELDS)}")
    elif isinstance(spec, (tuple, list)):
        if not 2 <= len(spec) <= 3:
            raise ValueError(f"motion: a tuple holds (pixel_delta, max_changed[, max_hold]), got {len(spec)} values")
        kw = dict(zip(_GATE_FIELDS, spec))
    else:
        raise ValueError(f"motion: expected a mapping, a tuple or a MotionGate, got {type(spec).__name__}")
    for name in _GATE_FIELDS[:2]:
        if name not in kw:
            raise ValueError(f"motion: {name} is missing (it has no default: nobody has measured what suits a real camera)")
    return MotionGate(kw["pixel_delta"], kw["max_changed"], kw.get("max_hold"))


def gate_decision(still: int, epoch: int, span: int, ref_epoch: Optional[int], holds: int, max_hold: Optional[int]):
    """The motion gate's decision for one due window (the module docstring has the rule): the camera's {still, epoch} as read
    back, the window's span, and the host's ref_epoch (None: no reference) and holds for it -> (held, ref_epoch, holds) with the
    bookkeeping as it stands after the decision.  held: the window repeats the previous clip; else it is extracted."""
    quiet = still + 1 >= span
    if quiet and ref_epoch is not None and ref_epoch == epoch and (max_hold is None or holds < max_hold):
        return True, ref_epoch, holds + 1
    return False, (epoch if quiet else None), 0


class LiveFrames:
    """The front end of live scoring: per-camera rings of the last `span` resized uint8 frames on the device, and the clips that
    are due gathered from them in one launch (include/advhip.h: "live frames").

        lf = LiveFrames(n_cameras, frame_hw=(256, 340), frames_per_clip=16, frame_step=None, clip_stride=None, device="cuda:0")
        due = lf.push(cams, frames, resize=256)   # one new decoded frame per listed camera -> the cameras whose clip is now due
        clips = lf.windows(due)                   # (len(due) * frames_per_clip, FH, FW, 3) uint8: what forward_frames reads

    span = frames_per_clip * frame_step; the frame pushed when a camera's count is k lies in slot k % span.  A clip is due after
    the push that brings a camera's count to k iff k >= span and (k - span) % clip_stride == 0, and it is window (k - span) /
    clip_stride of the camera's frames taken as an offline video (frames[w * s : w * s + span : d]) byte for byte, so features and
    scores are the offline ones.  No LoopPad runs live: a camera below `span` frames has no clip.  `frame_step` and `clip_stride`
    are ops.resolve_sampling's (None: 1 and the span).  The state is the ring (n_cameras, span, FH, FW, 3), the counts with a
    mirror on the host, one clip buffer (n_cameras * frames_per_clip, FH, FW, 3) -- the ring's size at frame_step 1 -- and one
    staging buffer (n_cameras, FH, FW, 3) the resize writes to.  Device id vectors are cached by their checked tuples: a push of
    device frames at ring size + windows on a repeated camera set uploads nothing, synchronises nothing and dispatches no torch
    arithmetic.  CUDA tensors only; no fallback.

        lf = LiveFrames(n_cameras, ..., motion=MotionGate(pixel_delta, max_changed, max_hold=None))
        due = lf.push(cams, frames)               # the gate's update runs on the frames on their way into the ring; every due camera
        extract, held = lf.decide(due)            # the one read-back: whose window goes through the backbone, whose repeats

    `motion` (resolve_motion_gate; None, the default: nothing is allocated or launched, `push` is launch for launch what it is
    without the argument) adds the motion gate of the module docstring: `anchor` (n_cameras, FH, FW, 3) uint8, `gate_state`
    (n_cameras, 4) int32 = {still, epoch, changed, peak}, a scratch for the counts and a pinned host buffer.  `push` then runs
    mil_ops.frame_gate_update in front of the ring push, and a step on which nothing is due still uploads nothing, synchronises
    nothing and dispatches no torch arithmetic; `decide`, called on due steps only, copies gate_state to the host and
    synchronises the stream once.  `last_decision` = (extract, held) of the last decide, `extracted_total` and `held_total`
    count windows; all three are host values.

        lf = LiveFrames(n_cameras, frame_hw=(256, 340), ..., rois=resize.RoiSpec((1080, 1920), {0: (0, 0, 960, 540), 3: (200.5, 100, 1400, 900)}))
        due = lf.push(cams, frames, pixel_format="nv12")        # each camera's box of its decoded frame -> its ring
        due = lf.push((4, 5, 6), frames, source_of=(0, 0, 1))   # cameras 4 and 5 are two regions of frames[0], camera 6 one of frames[1]

    `rois` (a resize.RoiSpec; None, the default: nothing is built and `push` is launch for launch what it is without the argument)
    gives every camera a region of interest of its decoded (H, W) frames -- a (left, top, right, bottom) box as PIL's
    `Image.resize(box=)` takes it, floats allowed; a camera without one sees the whole frame -- resized to frame_hw.  The tables of
    all cameras are built and uploaded once, here (resize.roi_tables); `push` then takes decoded frames in any form resize_u8 takes
    and resizes them into the staging buffer in one pair of launches, camera c with table c (resize.resize_rois_u8 with table_of =
    the cached id vector), so a steady push still uploads nothing and dispatches no torch arithmetic.  `source_of` (host ints, one
    per listed camera, cached on the device per tuple like the ids) names the row of `frames` each camera reads: one wide frame
    in, several virtual cameras' frames out.  The motion gate, the rings and everything behind them see the resized frames."""

    MAX_ROWS = 65535  # frame rows of one launch (the grid's second dimension)

    def __init__(self, n_cameras: int, frame_hw=(256, 340), frames_per_clip: int = 16, frame_step: Optional[int] = None,
                 clip_stride: Optional[int] = None, device="cuda:0", motion=None, rois=None):
        from . import ops
        from . import resize as rz

        try:
            fh, fw = frame_hw
        except (TypeError, ValueError):
            raise HipExtensionError(f"LiveFrames: frame_hw = {frame_hw!r} is not a pair (FH, FW)") from None
        for name, v in (("n_cameras", n_cameras), ("frame_hw[0]", fh), ("frame_hw[1]", fw), ("frames_per_clip", frames_per_clip)):
            if (k := host_int(v)) is None or k < 1:
                raise HipExtensionError(f"LiveFrames: {name} = {v!r} is not an integer >= 1")
        self.n_cameras, self.frame_hw, self.frames_per_clip = int(n_cameras), (int(fh), int(fw)), int(frames_per_clip)
        self.clip_stride, _, self.frame_step = ops.resolve_sampling(self.frames_per_clip, clip_stride, None, frame_step)
        self.span = self.frames_per_clip * self.frame_step
        if self.n_cameras * self.frames_per_clip > self.MAX_ROWS:
            raise HipExtensionError(f"LiveFrames: {self.n_cameras} cameras x {self.frames_per_clip} frames per clip is above the {self.MAX_ROWS} frame "
                                    f"rows one gather launch takes")
        try:
            self.motion = resolve_motion_gate(motion)
        except ValueError as e:
            raise HipExtensionError(f"LiveFrames: {e}") from None
        fb = self.frame_hw[0] * self.frame_hw[1] * 3
        if self.motion is not None and fb >= 1 << 31:
            raise HipExtensionError(f"LiveFrames: frames of {fb} bytes: the motion gate counts changed bytes in int32 (frame_bytes < 2^31)")
        self.cameras = CameraSet(self.n_cameras, device, "frame")
        self.device = self.cameras.device
        if self.device.type != "cuda":
            raise HipExtensionError(f"LiveFrames: device '{self.device}': the rings live on the GPU (there is no CPU fallback)")
        frame = self.frame_hw + (3,)
        self.ring = torch.zeros((self.n_cameras, self.span) + frame, dtype=torch.uint8, device=self.device)
        self._counts = torch.zeros((self.n_cameras,), dtype=torch.int64, device=self.device)
        self._clips = torch.empty((self.n_cameras * self.frames_per_clip,) + frame, dtype=torch.uint8, device=self.device)
        self._staging = torch.empty((self.n_cameras,) + frame, dtype=torch.uint8, device=self.device)
        self.last_decision, self.extracted_total, self.held_total = None, 0, 0
        self.rois = None
        if rois is not None:
            self.rois = self._resolve_rois(rois)
            with torch.cuda.device(self.device):
                self._roi_tables = rz.roi_tables(*self.rois.source_hw, self.frame_hw, self.rois.boxes, self.rois.resample, self.device)
            self._roi_ws = torch.empty((self.n_cameras * self._roi_tables.ws_rows * self.frame_hw[1] * 3,), dtype=torch.uint8, device=self.device)
            self._sources = _Lru(lambda rows: torch.tensor(rows, dtype=torch.int32).to(self.device))  # (keyed by checked tuples only)
        if self.motion is not None:
            self.gate_limit = self.motion.limit(fb)
            self.anchor = torch.zeros((self.n_cameras,) + frame, dtype=torch.uint8, device=self.device)
            self.gate_state = torch.tensor([mil_ops.GATE_STATE_INIT] * self.n_cameras, dtype=torch.int32).to(self.device)
            self._gate_scratch = torch.zeros((mil_ops.frame_gate_scratch(self.n_cameras, fb),), dtype=torch.int32, device=self.device)
            self._gate_host = torch.empty((self.n_cameras, 4), dtype=torch.int32, pin_memory=True)
            self._gate_rows = self._gate_host.numpy()  # (the same memory: what `decide` reads behind its synchronisation)
            self._ref_epoch, self._holds = [None] * self.n_cameras, [0] * self.n_cameras
            self._decided_at = [0] * self.n_cameras  # the count at which a camera's window was last decided

    def _resolve_rois(self, rois):
        """`rois` -> a resize.RoiSpec with (H, W) ints and a list of n_cameras boxes (None: the whole frame); the boxes themselves
        are checked by resize.roi_tables."""
        from . import resize as rz

        what = "LiveFrames: rois"
        if not isinstance(rois, rz.RoiSpec):
            if not isinstance(rois, (tuple, list)) or not 2 <= len(rois) <= 3:
                raise HipExtensionError(f"{what} = {rois!r} is not a resize.RoiSpec(source_hw, boxes, resample='bilinear')")
            rois = rz.RoiSpec(*rois)
        try:
            h, w = rois.source_hw
        except (TypeError, ValueError):
            raise HipExtensionError(f"{what}: source_hw = {rois.source_hw!r} is not a pair (H, W)") from None
        if (hh := host_int(h)) is None or (ww := host_int(w)) is None or hh < 1 or ww < 1:
            raise HipExtensionError(f"{what}: source_hw = {rois.source_hw!r} is not a pair of integers >= 1")
        boxes = rois.boxes
        if hasattr(boxes, "keys"):
            bad = [c for c in boxes.keys() if host_int(c, floats=False) is None or not 0 <= int(c) < self.n_cameras]
            if bad:
                raise HipExtensionError(f"{what}: boxes name cameras {bad} outside [0, {self.n_cameras})")
            by_cam = {int(c): boxes[c] for c in boxes.keys()}
            boxes = [by_cam.get(c) for c in range(self.n_cameras)]
        elif isinstance(boxes, (tuple, list)) and len(boxes) == self.n_cameras:
            boxes = list(boxes)
        else:
            raise HipExtensionError(f"{what}: boxes must be a sequence of {self.n_cameras} boxes (one per camera, None: the whole frame) or a "
                                    f"{{camera: box}} dict, got {boxes!r}")
        try:
            for bx in boxes:
                rz.resolve_box(what, bx, hh, ww)
            return rz.RoiSpec((hh, ww), boxes, rz.filter_name(rois.resample))
        except ValueError as e:
            raise HipExtensionError(str(e)) from None

    @property
    def counts(self) -> torch.Tensor:
        """Frames pushed so far per camera: int64 (n_cameras,) on the device."""
        return self._counts

    @property
    def counts_host(self) -> Tuple[int, ...]:
        """The same numbers on the host, kept by push / reset: nothing is read back."""
        return tuple(self.cameras.host)

    def is_due(self, count: int) -> bool:
        """The due rule: a clip is due at a camera's count k iff k >= span and (k - span) % clip_stride == 0."""
        return count >= self.span and (count - self.span) % self.clip_stride == 0

    def _source_hw(self, frames: torch.Tensor, pixel_format, surface) -> Optional[Tuple[int, int]]:
        """(H, W) of the frames resize_u8 is about to read, or None where their form is not one it takes (it says so itself)."""
        from . import resize as rz

        pf = rz.resolve_pixel_format(pixel_format)
        if pf is None:
            return tuple(frames.shape[1:3]) if surface is None and frames.dim() == 4 else None
        if surface is not None:
            if frames.dim() != 2:
                return None
            sf = rz.resolve_surface(surface, pf, frames.shape[1])
            return sf.height, sf.width
        return rz.frame_hw(frames.shape) if frames.dim() == 3 else None

    def push(self, cams: Sequence[int], frames: torch.Tensor, resize=None, resample="bilinear", pixel_format=None, surface=None,
             source_of=None) -> Tuple[int, ...]:
        """One new decoded frame for each camera of `cams` (distinct host ints); `frames` uint8 with len(cams) leading rows, on the
        host (copied non-blocking on the current stream) or on the device.  Without `resize`: (n, FH, FW, 3), already at ring
        size.  With `resize` (resize_u8's `size`): whatever resize_u8 takes -- packed RGB (n, H, W, 3), 4:2:0 (n, 3H/2, W) with
        `pixel_format`, (n, frame_bytes) with `surface` -- resized into the staging buffer; a result of another size than frame_hw
        is refused before anything is launched.  All frames of one call share a geometry.  -> the listed cameras whose clip
        became due with this push, in `cams` order, decided on the host mirror of the counts.
        With `rois` (the class docstring): `frames` are decoded frames of the RoiSpec's geometry in any of those forms, `resize` is
        refused (the boxes and frame_hw say what is resized to what), and `source_of` -- host ints, one per listed camera, each a
        row of `frames` -- lets several cameras read the same row; without it `frames` has one row per camera."""
        from . import resize as rz

        what = "LiveFrames.push"
        cams = self.cameras.check(cams, what)
        n = len(cams)
        if source_of is not None and self.rois is None:
            raise HipExtensionError(f"{what}: source_of names the decoded frame each camera's region is cut from: this LiveFrames has no rois")
        if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or frames.dim() < 2 or (frames.shape[0] != n and source_of is None):
            raise HipExtensionError(f"{what}: frames must be a torch.uint8 tensor with {n} leading rows, one frame per listed camera, got "
                                    f"{getattr(frames, 'dtype', type(frames).__name__)} {tuple(getattr(frames, 'shape', ()))}")
        if self.rois is not None:
            if resize is not None:
                raise HipExtensionError(f"{what}: resize= together with rois: the cameras' boxes are resized to the rings' {self.frame_hw} already")
            hw = self._source_hw(frames, pixel_format, surface)
            if hw is not None and tuple(hw) != self.rois.source_hw:
                raise HipExtensionError(f"{what}: the rois are boxes of {self.rois.source_hw[0]} x {self.rois.source_hw[1]} frames, these are "
                                        f"{hw[0]} x {hw[1]}")
            if source_of is not None:
                source_of = self._check_sources(what, source_of, n, frames.shape[0])
        elif resize is None:
            if pixel_format is not None or surface is not None:
                raise HipExtensionError(f"{what}: pixel_format / surface describe frames to be converted: give resize= (the ring's size {self.frame_hw} "
                                        f"for frames already that large)")
            want = (n,) + self.frame_hw + (3,)
            if tuple(frames.shape) != want:
                raise HipExtensionError(f"{what}: frames must be {want} (frames at ring size; resize= takes decoded frames), got {tuple(frames.shape)}")
        else:
            hw = self._source_hw(frames, pixel_format, surface)
            if hw is not None and rz.output_size(hw[0], hw[1], resize) != self.frame_hw:
                raise HipExtensionError(f"{what}: resize={resize!r} of {hw[0]} x {hw[1]} frames gives {rz.output_size(hw[0], hw[1], resize)}, the rings "
                                        f"hold {self.frame_hw} frames")
        if not frames.is_cuda:
            frames = frames.to(self.device, non_blocking=True)
        if self.rois is not None:  # camera c's box with table c: the id vector is the table vector
            frames = rz.resize_rois_u8(frames, self._roi_tables, table_of=self.cameras.ids(cams), src_of=None if source_of is None else self._sources(source_of),
                                       out=self._staging[:n], pixel_format=pixel_format, surface=surface, ws=self._roi_ws)
        elif resize is not None:
            frames = rz.resize_u8(frames, resize, resample, out=self._staging[:n], pixel_format=pixel_format, surface=surface)
        if self.motion is not None:  # on the frames as they enter the ring (its checks of `frames` are the ring push's: refused here, nothing has moved)
            mil_ops.frame_gate_update(frames, self.cameras.ids(cams), self.anchor, self.gate_state, self._gate_scratch, self.motion.pixel_delta,
                                      self.gate_limit)
        mil_ops.frame_ring_push(frames, self.cameras.ids(cams), self.ring, self._counts)
        self.cameras.bump(cams)
        return tuple(c for c in cams if self.is_due(self.cameras.host[c]))

    def _check_sources(self, what: str, source_of, n: int, n_frames: int) -> Tuple[int, ...]:
        """`source_of` as a tuple of n host ints in [0, n_frames), or a refusal."""
        if type(source_of) is tuple and len(source_of) == n and all(type(r) is int and 0 <= r < n_frames for r in source_of):
            return source_of
        if torch.is_tensor(source_of) or isinstance(source_of, (np.ndarray, str, bytes)) or not hasattr(source_of, "__len__"):
            raise HipExtensionError(f"{what}: source_of must be a sequence of host integers, got a {type(source_of).__name__}")
        if len(source_of) != n:
            raise HipExtensionError(f"{what}: source_of has {len(source_of)} entries for {n} listed cameras")
        for r in source_of:
            if host_int(r) is None or not 0 <= int(r) < n_frames:
                raise HipExtensionError(f"{what}: source_of entry {r!r} is not a row of the {n_frames} frames")
        return tuple(int(r) for r in source_of)

    def decide(self, due: Sequence[int]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        """The motion gate's decision for the cameras whose clip the last push made due -> (extract, held), both in `due` order:
        the windows of `extract` go through the backbone, the cameras of `held` repeat their previous clip (LiveScorer.hold).
        One copy of gate_state into the pinned host buffer and one synchronisation of the current stream, then `gate_decision`
        per camera; the bookkeeping (ref_epoch, holds, the totals, last_decision) is committed here, so a window is decided once."""
        what = "LiveFrames.decide"
        if self.motion is None:
            raise HipExtensionError(f"{what}: this LiveFrames has no motion gate (motion=None): every due window is extracted")
        due = self.cameras.check(due, what)
        host = self.cameras.host
        early = [c for c in due if not self.is_due(host[c])]
        if early:
            raise HipExtensionError(f"{what}: cameras {early} have no clip due at their counts {[host[c] for c in early]} (decide takes what push returned)")
        again = [c for c in due if self._decided_at[c] == host[c]]
        if again:
            raise HipExtensionError(f"{what}: the windows of cameras {again} are decided already: one decision per due window")
        self._gate_host.copy_(self.gate_state, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        extract, held = [], []
        for c in due:
            still, epoch = int(self._gate_rows[c, 0]), int(self._gate_rows[c, 1])
            is_held, self._ref_epoch[c], self._holds[c] = gate_decision(still, epoch, self.span, self._ref_epoch[c], self._holds[c], self.motion.max_hold)
            (held if is_held else extract).append(c)
            self._decided_at[c] = host[c]
        self.last_decision = (tuple(extract), tuple(held))
        self.extracted_total += len(extract)
        self.held_total += len(held)
        return self.last_decision

    def windows(self, cams: Sequence[int]) -> torch.Tensor:
        """The newest windows of the listed cameras, back to back in `cams` order: (len(cams) * frames_per_clip, FH, FW, 3) uint8,
        every frame_step-th frame of each camera's last `span`, oldest first -- one launch into the owned clip buffer, of which
        the result is a view (the next call overwrites it).  Every listed camera must have `span` frames."""
        cams = self.cameras.check(cams, "LiveFrames.windows")
        short = [c for c in cams if self.cameras.host[c] < self.span]
        if short:
            raise HipExtensionError(f"LiveFrames.windows: cameras {short} have fewer than span = {self.span} frames: no clip yet (no LoopPad runs live)")
        dst = self._clips[: len(cams) * self.frames_per_clip]
        return mil_ops.frame_ring_windows(self.ring, self._counts, self.cameras.ids(cams), dst, self.frames_per_clip, self.frame_step)

    def reset(self, cams: Sequence[int]) -> None:
        """The listed cameras start over at count 0: their rings' old frames can no longer reach a window.  With a motion gate
        they lose their anchor too (still := -1, epoch += 1) and the host forgets their reference and their holds."""
        cams = self.cameras.check(cams, "LiveFrames.reset")
        idx = self.cameras.ids(cams).long()
        self._counts[idx] = 0
        self.cameras.clear(cams)
        if self.motion is not None:
            self.gate_state[idx, 0] = -1
            self.gate_state[idx, 1] += 1
            for c in cams:
                self._ref_epoch[c], self._holds[c], self._decided_at[c] = None, 0, 0


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
            if (k := host_int(v)) is None or k < 1:
                raise HipExtensionError(f"LiveScorer: {name} = {v!r} is not an integer >= 1 (window < 1 holds no clip)")
        from .events import resolve_event_spec

        try:
            spec = resolve_event_spec(events)
        except ValueError as e:
            raise HipExtensionError(f"LiveScorer: {e}") from None
        if spec is not None and ((k := host_int(event_log, floats=False)) is None or k < 1):
            raise HipExtensionError(f"LiveScorer: event_log = {event_log!r} is not an integer >= 1")
        self.scorer = scorer
        self.n_cameras, self.window, self.ncrops, self.channels = int(n_cameras), int(window), int(ncrops), int(channels)
        if self.channels > mil_ops.ADD_MAGNITUDE_NP_MAX_C:
            raise HipExtensionError(f"LiveScorer: channels = {self.channels} above {mil_ops.ADD_MAGNITUDE_NP_MAX_C}: the magnitude channel has numpy's bits up to there")
        rows = self.n_cameras * self.ncrops * self.window
        if rows > int(max_rows):
            raise HipExtensionError(f"LiveScorer: {self.n_cameras} cameras x {self.ncrops} crops x {self.window} clips = {rows} rows is above the "
                                    f"scorer's row limit of {int(max_rows)}")
        self.cameras = CameraSet(self.n_cameras, device, "clip")
        self.device = self.cameras.device
        if self.device.type != "cuda":
            raise HipExtensionError(f"LiveScorer: device '{self.device}': the rings live on the GPU (there is no CPU fallback)")
        shape = (self.n_cameras, self.ncrops, self.window, self.channels + 1)
        self.ring = torch.zeros(shape, dtype=torch.float32, device=self.device)
        self._counts = torch.zeros((self.n_cameras,), dtype=torch.int64, device=self.device)
        self.latest = torch.full((self.n_cameras,), float("nan"), dtype=torch.float32, device=self.device)
        # (never initialised: the rows behind a window hold what an earlier call left there, which the padded pass never reads as values)
        self._batch = torch.empty(shape, dtype=torch.float32, device=self.device).view(-1)
        self._iota = torch.arange(self.n_cameras, dtype=torch.int32).to(self.device)
        self._lens = _Lru(self._make_lens)
        self.events = None
        if spec is not None:
            from .events import LiveEventTracker

            self.events = LiveEventTracker(spec, self.n_cameras, log=event_log, device=self.device, cameras=self.cameras)

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
        return tuple(self.cameras.host)

    def push(self, cams: Sequence[int], feats: torch.Tensor) -> None:
        """One new clip for each camera of `cams` (distinct host ints): feats (len(cams), ncrops, channels) fp32 on the device."""
        cams = self.cameras.check(cams, "LiveScorer.push")
        want = (len(cams), self.ncrops, self.channels)
        if not torch.is_tensor(feats) or tuple(feats.shape) != want:
            raise HipExtensionError(f"LiveScorer.push: feats must be {want} (cameras, crops, channels), got {tuple(getattr(feats, 'shape', ()))}")
        mil_ops.ring_push(feats, self.cameras.ids(cams), self.ring, self._counts)
        self.cameras.bump(cams)

    def hold(self, cams: Sequence[int]) -> None:
        """The newest clip of each listed camera again (mil_ops.ring_repeat): every crop's row, magnitude channel included, bit
        for bit from slot (k - 1) % window to slot k % window at the camera's count k, and the count goes up by one -- what the
        motion gate does for a still camera instead of the backbone.  The repeated clip is a clip like any other: it is scored,
        and with `events=` it is a sample of the camera's series.  A camera without a clip is refused."""
        cams = self.cameras.check(cams, "LiveScorer.hold")
        empty = [c for c in cams if self.cameras.host[c] == 0]
        if empty:
            raise HipExtensionError(f"LiveScorer.hold: cameras {empty} have no clip to repeat (their count is 0)")
        mil_ops.ring_repeat(self.cameras.ids(cams), self.ring, self._counts)
        self.cameras.bump(cams)

    def score(self, cams: Optional[Sequence[int]] = None) -> LiveScores:
        """The windows of the listed cameras (None: every camera with at least one clip, ascending) scored in one padded pass."""
        if cams is None:
            cams = tuple(c for c, k in enumerate(self.cameras.host) if k > 0)
            if not cams:
                raise HipExtensionError("LiveScorer.score: no camera has a clip yet")
        else:
            cams = self.cameras.check(cams, "LiveScorer.score")
            empty = [c for c in cams if self.cameras.host[c] == 0]
            if empty:
                raise HipExtensionError(f"LiveScorer.score: cameras {empty} have no clip yet")
        feed = None
        if self.events is not None:  # which of the listed cameras have a new clip for the tracker: decided before anything is launched
            fed = self.events.cameras.host
            ahead = [c for c in cams if self.cameras.host[c] > fed[c] + 1]
            if ahead:
                raise HipExtensionError(f"LiveScorer.score: cameras {ahead} are more than one clip ahead of their event series (pushed twice, scored "
                                        f"once): every clip's score is a sample; score after every push, or reset the cameras")
            feed = tuple(c for c in cams if self.cameras.host[c] == fed[c] + 1)
        lens = tuple(min(self.cameras.host[c], self.window) for c in cams)
        nb, tmax = len(cams), max(lens)
        ids, pl = self.cameras.ids(cams), self._lens((lens, tmax))
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
        cams = self.cameras.check(cams, "LiveScorer.reset")
        if self.events is not None:
            self.events.reset(cams)
        idx = self.cameras.ids(cams).long()
        self._counts[idx] = 0
        self.latest[idx] = float("nan")
        self.cameras.clear(cams)

    def step_frames(self, backbone, frames_u8: torch.Tensor, cams: Sequence[int], **sampling) -> LiveScores:
        """One clip per camera straight from resized uint8 frames: `frames_u8` (len(cams) * span, FH, FW, 3) on the device holds
        the cameras' clips back to back in `cams` order (span = frames_per_clip * frame_step frames each); `sampling` are
        I3Res50.forward_frames' arguments (frames_per_clip, crop, crops, frame_step, normalize), with len(crops) = ncrops.
        -> backbone.forward_frames, `push`, `score(cams)`."""
        from . import ops

        cams = self.cameras.check(cams, "LiveScorer.step_frames")
        fpc = sampling.get("frames_per_clip", 16)
        s, crops, d = ops.resolve_sampling(fpc, sampling.get("clip_stride"), sampling.get("crops"), sampling.get("frame_step"))
        if s != fpc * d:
            raise HipExtensionError(f"LiveScorer.step_frames: clip_stride {s} is not the clip's span {fpc * d}: the cameras' clips lie back to back")
        if len(crops) != self.ncrops:
            raise HipExtensionError(f"LiveScorer.step_frames: {len(crops)} crops, the rings hold {self.ncrops}")
        if not torch.is_tensor(frames_u8) or frames_u8.dim() != 4 or frames_u8.shape[0] != len(cams) * fpc * d:
            raise HipExtensionError(f"LiveScorer.step_frames: frames_u8 must be ({len(cams) * fpc * d}, FH, FW, 3): {fpc * d} frames for each of "
                                    f"{len(cams)} cameras, got {tuple(getattr(frames_u8, 'shape', ()))}")
        return self._step_clips("LiveScorer.step_frames", backbone, frames_u8, cams, sampling)

    def _step_clips(self, what: str, backbone, clips: torch.Tensor, cams: Tuple[int, ...], forward_kw: dict) -> LiveScores:
        """The tail of both step methods: backbone.forward_frames on the back-to-back clips of `cams`, `push`, `score(cams)`."""
        self._extract_clips(what, backbone, clips, cams, forward_kw)
        return self.score(cams)

    def _extract_clips(self, what: str, backbone, clips: torch.Tensor, cams: Tuple[int, ...], forward_kw: dict) -> None:
        """backbone.forward_frames on the back-to-back clips of `cams`, then `push`."""
        feats = backbone.forward_frames(clips, 0, len(cams) * self.ncrops, **forward_kw)
        if feats.numel() != len(cams) * self.ncrops * self.channels:
            raise HipExtensionError(f"{what}: the backbone's features are {tuple(feats.shape)}, the rings hold {self.channels} channels")
        self.push(cams, feats.reshape(len(cams), self.ncrops, self.channels))

    _PUSH_KW, _FORWARD_KW = ("resize", "resample", "pixel_format", "surface", "source_of"), ("crop", "crops", "normalize")

    def step_camera_frames(self, backbone, live_frames: LiveFrames, cams: Sequence[int], frames: torch.Tensor, **kw) -> Optional[LiveScores]:
        """One new decoded frame per listed camera, through to the scores: `live_frames.push(cams, frames, ...)`; when no clip
        became due, None, with nothing else launched; else `live_frames.windows(due)`, backbone.forward_frames on those
        back-to-back clips (the gather has applied clip_stride and frame_step already), `push(due, feats)` and `score(due)`.
        `kw`: push's resize / resample / pixel_format / surface / source_of and forward_frames' crop / crops / normalize, with len(crops) =
        ncrops; frames_per_clip, frame_step and clip_stride are the LiveFrames' own and refused here.  The features and scores of
        a camera are those of its frames as an offline video, window by window.  With `events=` every due window is one sample
        of the camera's series: a sample is then clip_stride frames, not span frames, and EventSpec's lengths (smooth, merge_gap,
        min_len) count such samples.  A LiveFrames with a motion gate: push, `live_frames.decide(due)` -> (extract, held), then
        windows / forward_frames / push for `extract` only (skipped when it is empty), `hold(held)`, and `score(due)` in one
        padded pass; a held clip is a sample like any other.  A camera that starts over is reset in both objects: the gate's
        reference is a clip in this object's ring, and `hold` refuses a camera whose ring is empty."""
        from . import ops

        what = "LiveScorer.step_camera_frames"
        if not isinstance(live_frames, LiveFrames):
            raise HipExtensionError(f"{what}: live_frames must be a LiveFrames, got {type(live_frames).__name__}")
        own = [k for k in ("frames_per_clip", "frame_step", "clip_stride") if k in kw]
        if own:
            raise HipExtensionError(f"{what}: {', '.join(own)} belong to the LiveFrames (frames_per_clip {live_frames.frames_per_clip}, frame_step "
                                    f"{live_frames.frame_step}, clip_stride {live_frames.clip_stride}): they are set where the rings are built")
        unknown = [k for k in kw if k not in self._PUSH_KW + self._FORWARD_KW]
        if unknown:
            raise HipExtensionError(f"{what}: unknown arguments {unknown}: push takes {list(self._PUSH_KW)}, forward_frames {list(self._FORWARD_KW)}")
        if live_frames.n_cameras != self.n_cameras or live_frames.device != self.device:
            raise HipExtensionError(f"{what}: the LiveFrames holds {live_frames.n_cameras} cameras on {live_frames.device}, the LiveScorer "
                                    f"{self.n_cameras} on {self.device}")
        crops = ops.resolve_crops(kw.get("crops"))
        if len(crops) != self.ncrops:
            raise HipExtensionError(f"{what}: {len(crops)} crops, the rings hold {self.ncrops}")
        due = live_frames.push(cams, frames, **{k: kw[k] for k in self._PUSH_KW if k in kw})
        if not due:
            return None
        forward_kw = {"frames_per_clip": live_frames.frames_per_clip, **{k: kw[k] for k in self._FORWARD_KW if k in kw}}
        if live_frames.motion is None:
            return self._step_clips(what, backbone, live_frames.windows(due), due, forward_kw)
        # the motion gate: the backbone sees the windows that moved (and every still scene's first), a still camera repeats its clip
        extract, held = live_frames.decide(due)
        if extract:
            self._extract_clips(what, backbone, live_frames.windows(extract), extract, forward_kw)
        if held:
            self.hold(held)
        return self.score(due)
