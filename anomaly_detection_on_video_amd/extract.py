"""Feature-extraction driver: the hot loops of `/root/reference/extract_features.py`.

Kept from the reference: `load_feature_extraction_model`, the `(n_clips, 10, 2048)` output layout
of `_extract` (:77-102), `.npy` per video with skip-if-exists resume (:104-110, :156) and
`segment()` (:159-185).  Changed on purpose: the ten crops are folded into
the batch dimension (one backbone forward over (10*B) crop-clips instead of ten forwards of B),
nothing builds an autograd graph, features stay on the GPU until a whole video is done, and the
bucket means of `segment()` run on the device.  Video decoding / TenCrop (decord, torchvision)
are out of scope: sources here are tensors already shaped like `TenCropVideoFrameDataset` items,
(n_clips, 10, 16, 3, 224, 224) fp32 normalised frames (src/dataset.py:192-195).
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import dist as adist
from . import mil_ops
from . import resize as resize_mod
from .i3d import build_i3d_feature_extractor
from .ops import crop_minmax_u8, crop_stats_pitch, crops_tag, n_windows, normalize_is_default, normalize_tag, resolve_normalize, pad_windows_u8, resolve_clip_stride, resolve_frame_step, resolve_sampling  # noqa: F401  (n_windows is part of this module's interface)

FRAMES_PER_CLIP = 16
NCROPS = 10


PINNED_MODEL = "tushar-n-baseline"  # the in-repo I3Res50: parity pinned by reference-made goldens


def load_feature_extraction_model(model_name: str = "i3d_8x8_r50", **factory_kwargs):
    """(model.eval() on the GPU, device) -- extract_features.py:34-40, same default name as the reference.

    `i3d_8x8_r50` is the third-party pytorchvideo ResNet (src/i3d.py:339-350): it is built here on the same HIP kernels
    from its published topology, but pytorchvideo is not available to check it against -- PARITY UNPINNED, and a warning says
    so.  `tushar-n-baseline` (the in-repo I3Res50, what the shipped training features `revision: tushar-n` come from) is
    the variant pinned by the reference-made goldens and the one bench.py times."""
    if model_name == "i3d_8x8_r50":
        import warnings

        warnings.warn("load_feature_extraction_model: 'i3d_8x8_r50' (the reference's default, pytorchvideo topology) is parity-unpinned "
                      f"here; pass model_name={PINNED_MODEL!r} for the I3Res50 pinned against the reference", stacklevel=2)
    model = build_i3d_feature_extractor(model_name=model_name, **factory_kwargs)
    model.eval()
    if not torch.cuda.is_available():
        raise RuntimeError("no AMD GPU visible: the extraction path runs only as HIP kernels (no CPU fallback)")
    model.cuda()
    device = next(model.parameters()).device
    return model, device


_LANES: Dict[torch.device, list] = {}


@torch.no_grad()
def run_chunks_on_lanes(model, chunks, lanes: Optional[int] = None, fn=None, prepare=None) -> torch.Tensor:
    """Backbone forwards of independent chunks of crop-clips -> (sum of rows, 2048), in order.  One chunk: a plain
    `model(chunk)` (which splits its batch over two streams itself).  Several: chunk i runs on HIP stream lane
    i % lanes as whole-batch launches, so up to `lanes` forwards are in flight and one chunk's kernel tails and
    memory-bound launches overlap another's MFMA-bound ones (same kernels, bit-identical rows; pipeline.py has the
    measurements).  The caller's stream waits for every lane before the rows are concatenated."""
    lanes = int(os.environ.get("ADV_PIPELINE_LANES", "3")) if lanes is None else lanes
    if fn is not None:  # chunks are descriptors (e.g. crop-clip ranges of a frames tensor), fn(chunk) runs one; prepare() builds lazy state
        if len(chunks) <= 1 or lanes <= 1:
            return torch.cat([fn(c).reshape(-1, 2048) for c in chunks], dim=0)
        dev = next(model.parameters()).device
    elif len(chunks) <= 1 or lanes <= 1 or not chunks[0].is_cuda:  # (CPU tensors: host-logic tests with a stand-in model)
        return torch.cat([model(c.contiguous()).reshape(-1, 2048) for c in chunks], dim=0)
    else:
        dev = chunks[0].device
    pool = _LANES.setdefault(dev, [])
    while len(pool) < lanes:
        pool.append(torch.cuda.Stream(device=dev))
    cur = torch.cuda.current_stream(dev)
    if prepare is not None:
        prepare()
    elif hasattr(model, "ensure_tables"):
        model.ensure_tables(tuple(chunks[0].shape[2:]))  # lazily built state: before the lanes fork
    ready = torch.cuda.Event()
    ready.record(cur)
    outs, inner = [], getattr(model, "streams", 1)
    try:
        model.streams = 1
        for i, c in enumerate(chunks):
            lane = pool[i % lanes]
            with torch.cuda.stream(lane):
                lane.wait_event(ready)
                if fn is not None:
                    out = fn(c).reshape(-1, 2048)
                else:
                    c = c.contiguous()
                    c.record_stream(lane)
                    out = model(c).reshape(-1, 2048)
                done = torch.cuda.Event()
                done.record(lane)
            cur.wait_event(done)
            out.record_stream(cur)
            outs.append(out)
    finally:
        model.streams = inner
    return torch.cat(outs, dim=0)


@torch.no_grad()
def extract_clip_batch(model, clips: torch.Tensor, max_crop_clips: int = 32, sharded: bool = False) -> torch.Tensor:
    """(B, ncrops, 16, 3, H, W) TenCrop'd clips -> (B, ncrops, 2048) features on the device.

    `max_crop_clips` bounds the folded batch per backbone launch (activation memory; 32 is the batch
    the tile table in tuned/gfx950.json was measured at).  With
    `sharded=True` the folded crop-clips are split over the ranks of the default process group
    and the rows all-gathered (dist.sharded_map_rows)."""
    if clips.dim() != 6:
        raise ValueError(f"expected (B, ncrops, T, 3, H, W), got {tuple(clips.shape)}")
    B, ncrops = clips.shape[:2]
    dev = next(model.parameters()).device
    if clips.dtype == torch.uint8:
        # raw TenCrop'd pixels: only uint8 crosses PCIe; float conversion, (x-114.75)/57.375 and the
        # (T,C)->(C,T) permute happen in one HIP pass (dataset.py:175-183 + extract_features.py:83)
        folded = mil_ops.normalize_permute_u8(clips.to(dev, non_blocking=True).reshape(B * ncrops, *clips.shape[2:]))
    else:
        # (B, ncrops, T, C, H, W) -> (B*ncrops, C, T, H, W): the reference's permute (:83) + crop fold
        folded = clips.to(dev, non_blocking=True).permute(0, 1, 3, 2, 4, 5).reshape(B * ncrops, clips.shape[3], clips.shape[2], *clips.shape[4:])

    def run(units: torch.Tensor) -> torch.Tensor:
        return run_chunks_on_lanes(model, [units[i : i + max_crop_clips] for i in range(0, units.shape[0], max_crop_clips)])

    rows = adist.sharded_map_rows(run, folded) if sharded else run(folded)
    return rows.reshape(B, ncrops, 2048)


@torch.no_grad()
def extract_video(model, video_clips: torch.Tensor, batch_size: int = 16, **kw) -> np.ndarray:
    """The reference's `_extract`: all clips of one video -> np.float32 (n_clips, 10, 2048)."""
    outs = [extract_clip_batch(model, video_clips[i : i + batch_size], **kw) for i in range(0, video_clips.shape[0], batch_size)]
    out = torch.cat(outs, dim=0).cpu().numpy()
    return np.squeeze(out)  # np.squeeze as the reference does (:100): a 1-clip video loses its first axis


@torch.no_grad()
def extract_video_frames(model, frames: torch.Tensor, frames_per_clip: int = FRAMES_PER_CLIP, crop: int = 224,
                         clips_per_step: Optional[int] = None, resize=None, resample="bilinear", clip_stride: Optional[int] = None,
                         crops=None, frame_step: Optional[int] = None, normalize=None, pixel_format=None, surface=None,
                         box=None, **kw) -> np.ndarray:
    """One video as resized uint8 frames (F, H, W, 3) -- what the decoder + GroupResize(256) hand over -- to np.float32
    (n_clips, 10, 2048): TenCrop, float conversion, normalisation, LoopPad and both permutes run on the device
    (mil_ops.tencrop_normalize_u8), so only the resized uint8 frames cross PCIe (1/23 of the fp32 ten-crop tensor the
    reference's DataLoader ships per clip, src/dataset.py:175-195, extract_features.py:79-86).  `clips_per_step` clips
    (x 10 crops) are pre-processed and run per step.

    With `resize` (e.g. 256), `frames` are the decoded frames at their native size, on the host or the device, and each
    step's frames are resized on the device first: `GroupResize(resize, resample)` of src/gtransforms.py:9-18, PIL's bytes
    (resize.resize_u8).  Only the decoded uint8 frames cross PCIe then.

    `clip_stride` (default frames_per_clip, the reference's back-to-back clips): clip w is the window of frames_per_clip
    frames that starts at frame w * clip_stride, n_clips = n_windows(F, frames_per_clip, clip_stride), only the last window is
    LoopPad-ed.  The windows are addressed in place by the kernels: a step reads frames [w0 * s, (w0 + clips_per_step - 1) * s +
    frames_per_clip), host frames are copied per step with that overlap (with `resize`, the overlap is resized again: PIL's
    bytes either way), frames already on the device are not copied at all.

    `crops` (ops.resolve_crops: "ten", "five", "center" / "centre", "center_flip" or a strictly ascending tuple of TenCrop
    indices; default None = all ten): only those crops are extracted, (n_clips, len(crops), 2048) -- a subset is never squeezed -- and row
    [q, j] is bit for bit row [q, crops[j]] of the ten-crop features at the same step cuts: 10 / len(crops) times less backbone
    work per clip.  `clips_per_step` defaults to 3; with a crop subset and no explicit value to max(1, 30 // len(crops)), so a
    step still launches about 30 crop-clips.

    `frame_step` d (default None = 1): temporal sampling -- sampled frame t of clip w is frames[w * clip_stride + t * d], a clip spans
    frames_per_clip * d frames, clip_stride defaults to that span (1 <= clip_stride <= span) and n_clips = n_windows(F,
    frames_per_clip, clip_stride, d); a short last clip LoopPads its ceil((F - w * s) / d) sampled frames.  Nothing is decimated
    on the host into a second tensor.  Where d divides clip_stride a step's sampled frames form one lattice: of host frames only
    that lattice is copied (and resized); decoded frames already on the device are resized straight from the lattice
    (resize_u8(frame_step=d)), and the step then runs at (clip_stride // d, 1) -- the result is extract_video_frames(frames[::d],
    clip_stride=clip_stride // d) bit for bit.  Resized frames already on the device, and any stride d does not divide, are
    addressed in place by the kernels with d as a launch argument.

    `normalize` (ops.resolve_normalize; default None = the reference's (x - 114.75) / 57.375): ("standardize", mean, std) with
    per-channel lists, "pixel_minmax" / ("pixel_minmax", lo, hi) or "channel_minmax" / ("channel_minmax", lo, hi) -- the reference's
    GroupStandardizationTenCrop, GroupPixelMinmaxTenCrop and GroupRGBChannelMinmaxTenCrop (src/gtransforms.py:57-112), bit for
    bit on the normalised pixels, NaN for a constant crop / channel included.  The min-max kinds take each (frame, crop)'s minimum
    and maximum first: one statistics launch per step on the caller's stream (ops.crop_minmax_u8), shared by the step's ranges.  A
    frame's statistics are its own: the normalised pixels do not depend on how the video is cut into steps.

    `pixel_format` (resize.resolve_pixel_format; default None = packed RGB): "nv12", "i420" / "yuv420p", (layout, "bt709"),
    (layout, matrix, "full") -- `frames` are the decoder's own 8-bit 4:2:0 frames, uint8 (F, 3H/2, W), on the host or the device.
    Host frames cross PCIe as they are (1.5 bytes per pixel), the colour conversion runs on the device: inside the resize's
    horizontal pass with `resize` (the full-size RGB frames never exist), as one launch of its own without (a decoder that scaled
    already).  The features are those of the converted frames, extract_video_frames(yuv420_to_rgb_u8(frames), ...), bit for bit.
    The conversion is resize.yuv_coefficients' integer formula with nearest chroma, not swscale's bytes: packed RGB frames
    remain the reference-parity input.  Like `resize` it describes the source, so file names carry no tag for it.

    `surface` (a resize.Surface, e.g. from resize.surface; with `pixel_format`; default None = the compact frames above): `frames`
    are the decoder's surfaces as they are, uint8 (F, frame_bytes) -- a row pitch above W, aligned rows, plane offsets, NV21 / YV12
    order, 10-bit P010 / yuv420p10le -- and the conversion or the fused resize reads them in place by that geometry.  Host frames
    cross PCIe as they are, padding included.  The features are again those of the converted frames, bit for bit; no file-name tag.

    `box` (left, top, right, bottom) in source pixels, floats allowed (with `resize`; default None = the whole frame): a region of
    interest -- every decoded frame is resized from that box, PIL's `Image.resize(size, resample, box=box)` (resize_u8(box=)), so
    the features are those of the box-resized frames bit for bit, from any source form.  An int `resize` is the box's short side."""
    if box is not None and resize is None:
        raise ValueError("box= names a part of the decoded frames: it needs resize= (the size the box is resized to)")
    s, crops, fstep = resolve_sampling(frames_per_clip, clip_stride, crops, frame_step)
    norm = resolve_normalize(normalize)
    plain = normalize_is_default(norm)
    nc = len(crops)
    subset = nc != 10  # ("ten" and (0, ..., 9) are None in every respect, the squeeze included)
    if clips_per_step is None:
        clips_per_step = max(1, 30 // nc) if subset else 3
    pf = resize_mod.resolve_pixel_format(pixel_format)
    if surface is not None:  # (refuses a missing pixel format and an impossible geometry before anything is copied)
        if frames.dtype != torch.uint8 or frames.dim() != 2:
            raise ValueError(f"expected uint8 (F, frame_bytes) surfaces, got {frames.dtype} {tuple(frames.shape)}")
        surface = resize_mod.resolve_surface(surface, pf, frames.shape[1])
    elif pf is not None:
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise ValueError(f"expected uint8 (F, 3H/2, W) {pf.layout} frames, got {frames.dtype} {tuple(frames.shape)}")
        resize_mod.frame_hw(frames.shape)  # (refuses an impossible geometry before anything is copied)
    elif frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"expected uint8 (F,H,W,C) frames, got {frames.dtype} {tuple(frames.shape)}")
    convert = resize is not None or pf is not None  # a device pass writes the RGB frames the step reads
    dev = next(model.parameters()).device
    rows = []
    n_total = n_windows(frames.shape[0], frames_per_clip, s, fstep)
    lattice = fstep != 1 and s % fstep == 0  # the sampled frames of a step: frames w0 * s + k * fstep, one arithmetic progression
    max_cc = kw.get("max_crop_clips", 32)
    direct = hasattr(model, "forward_frames") and hasattr(model, "frames_fused") and model.frames_fused()
    for w0 in range(0, n_total, clips_per_step):
        w1 = min(w0 + clips_per_step, n_total)
        fr = frames[w0 * s : (w1 - 1) * s + frames_per_clip * fstep]  # (the slice ends with the video: a short last window)
        ss, dd, rstep = s, fstep, None  # how the kernels address `fr`; the step of the resize
        if lattice:
            if fr.is_cuda and not convert:
                pass  # resized frames on the device: read in place, every fstep-th frame
            else:
                ss, dd = s // fstep, 1  # downstream sees the lattice as a video of its own
                if fr.is_cuda:
                    rstep = fstep  # decoded frames on the device: the resize reads the lattice in place
                else:
                    fr = fr[::fstep]  # host frames: only the lattice crosses PCIe
        if convert:  # decoded frames -> (colour conversion +) GroupResize on the device, into a buffer with the stem's spare bytes
            fr = fr.to(dev, non_blocking=True).contiguous()
            if surface is not None:
                (h, w), c = (surface.height, surface.width), 3
            else:
                (h, w), c = ((fr.shape[1], fr.shape[2]), fr.shape[3]) if pf is None else (resize_mod.frame_hw(fr.shape), 3)
            if box is not None:
                oh, ow = resize_mod.box_output_size(resize_mod.resolve_box("extract_video_frames", box, h, w), resize)
            else:
                oh, ow = (h, w) if resize is None else resize_mod.output_size(h, w, resize)
            nf = fr.shape[0] if rstep is None else -(-fr.shape[0] // rstep)
            n = nf * oh * ow * c
            buf = torch.empty((n + 16,), device=dev, dtype=torch.uint8)
            out = buf[:n].view(nf, oh, ow, c)
            if resize is None:  # 4:2:0 frames a decoder scaled already: the conversion launch alone
                fr = resize_mod.yuv420_to_rgb_u8(fr, pf, out=out, frame_step=rstep, surface=surface)
            elif pf is None:
                fr = resize_mod.resize_u8(fr, resize, resample, out=out, frame_step=rstep, box=box)
            else:
                fr = resize_mod.resize_u8(fr, resize, resample, out=out, frame_step=rstep, pixel_format=pf, surface=surface, box=box)
        elif direct and not fr.is_cuda:  # a device buffer with a few spare bytes behind the pixels (the stem fetches whole 4-byte pieces)
            buf = torch.empty((fr.numel() + 16,), device=dev, dtype=torch.uint8)
            if fr.is_contiguous():
                buf[: fr.numel()].copy_(fr.reshape(-1), non_blocking=True)
            else:  # (the lattice of a sampled step: a strided host view, copied frame by frame into the compact buffer)
                buf[: fr.numel()].view(fr.shape).copy_(fr, non_blocking=True)
            fr = buf[: fr.numel()].view(fr.shape)
        else:
            fr = fr.to(dev, non_blocking=True)
        if not direct:
            x = mil_ops.tencrop_normalize_u8(fr, frames_per_clip, crop, clip_stride=ss, crops=crops, frame_step=dd, normalize=norm)
            rows.append(run_chunks_on_lanes(model, [x[i : i + max_cc] for i in range(0, x.shape[0], max_cc)]))
            continue
        # the stem kernel reads the uint8 pixels itself (TenCrop + float + normalise in its load stage): only LoopPad is left,
        # and only for a last window shorter than frames_per_clip (src/gtransforms.py:119-132) -- a uint8 gather of <= 15 frames
        # (a sampled step whose model runs a TenCrop pass first is left as it is: that pass LoopPads itself)
        # (nor is a step with another normalisation: it always runs a TenCrop pass)
        if plain and (dd == 1 or not hasattr(model, "frames_need_whole_windows") or model.frames_need_whole_windows(crop)):
            fr = pad_windows_u8(fr, frames_per_clip, ss, dd).contiguous()
        n = (w1 - w0) * nc
        ranges = [(i, min(max_cc, n - i)) for i in range(0, n, max_cc)]
        if plain:
            more = {}
        else:  # the step's statistics once, here on the caller's stream, before the lanes fork: every range reads the same table
            fr = fr.contiguous()
            stats = None if norm.kind == "standardize" else crop_minmax_u8(fr, crop, crop_stats_pitch(frames_per_clip, ss, dd))
            more = dict(normalize=norm, crop_stats=stats)

        def run_range(r, fr=fr, ss=ss, dd=dd, more=more):
            for t in (fr, more.get("crop_stats")):  # (read on a lane stream, allocated on the caller's)
                if t is not None:
                    t.record_stream(torch.cuda.current_stream(dev))
            return model.forward_frames(fr, r[0], r[1], frames_per_clip, crop, clip_stride=ss, crops=crops, frame_step=dd, **more)

        def build_tables(fr=fr, dd=dd):
            norm_kw = {} if plain else dict(normalize=norm)
            for b in sorted({r[1] for r in ranges}):
                model.ensure_frame_tables(tuple(fr.shape[1:3]), frames_per_clip, crop, b, frame_step=dd, **norm_kw)

        rows.append(run_chunks_on_lanes(model, ranges, fn=run_range, prepare=build_tables))
    out = torch.cat(rows, dim=0).reshape(-1, nc, 2048).cpu().numpy()
    return out if subset else np.squeeze(out)  # (the reference's np.squeeze quirk belongs to its own ten-crop call only)


SEGMENT_FRAMES = 16 * 188  # 3008: extract_features.py:121


def segment_windows(n_frames: int, seg_len: int = SEGMENT_FRAMES, frames_per_clip: int = FRAMES_PER_CLIP,
                    clip_stride: Optional[int] = None, frame_step: Optional[int] = None):
    """How a long video's windows are shared out between its segments: [(segment, first window, end window, first frame, end
    frame)] over the reference's segments 0 .. n_frames // seg_len (extract_features.py:116-148), those that own no window left out.
    Segment k owns the windows that START in [k * seg_len, (k + 1) * seg_len) and therefore reads frames up to frames_per_clip -
    clip_stride past its end: frames [k * seg_len, min((k + 1) * seg_len + frames_per_clip - clip_stride, n_frames)), which taken
    as a video of their own have exactly the owned windows -- and only the video's last window can be short.  seg_len must be a
    multiple of clip_stride (window starts would drift against the segments otherwise).  With `frame_step` d a window spans
    frames_per_clip * d frames: the same with that span, a segment reads up to frames_per_clip * d - clip_stride past its end."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    if seg_len < 1 or seg_len % s:
        raise ValueError(f"seg_len {seg_len} is not a positive multiple of clip_stride {s}")
    n, per_seg = n_windows(n_frames, frames_per_clip, s, d), seg_len // s
    out = []
    for seg in range(n_frames // seg_len + 1):
        w0, w1 = seg * per_seg, min((seg + 1) * per_seg, n)
        if w0 >= w1:  # nothing starts here: n_frames a multiple of seg_len, or a tail the previous segment's last window covers
            continue
        out.append((seg, w0, w1, seg * seg_len, min((seg + 1) * seg_len + frames_per_clip * d - s, n_frames)))
    return out


def feature_tag(frames_per_clip: int = FRAMES_PER_CLIP, clip_stride: Optional[int] = None, crops=None,
                frame_step: Optional[int] = None, normalize=None) -> str:
    """What a feature file's name says about how it was extracted: "" for the reference's own (back-to-back clips, ten crops),
    "_d<step>" for temporal sampling, "_s<stride>" for a stride other than the window span (frames_per_clip * frame_step), then
    "_c<digits>" for a crop subset ("_s8_c4", "_c01234", "_d2", "_d2_s8_c4"), then the normalisation's tag (ops.normalize_tag: "_npix",
    "_nch-1f3a...", "_d2_s8_c4_nstd-...").  Files made one way are never read another way."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    return ("" if d == 1 else f"_d{d}") + ("" if s == frames_per_clip * d else f"_s{s}") + crops_tag(crops) + normalize_tag(normalize)


def extract_long_video_frames(model, name: str, n_frames: int, read_frames: Callable[[int, int], torch.Tensor], outpath: str,
                              seg_len: int = SEGMENT_FRAMES, **kw) -> np.ndarray:
    """The reference's treatment of videos too large to hold in RAM (extract_features.py:116-148): the video is cut into
    segments of `seg_len` frames (a multiple of 16, so only the last clip of the video is LoopPad-ed), each segment's
    (n_clips, 10, 2048) features are cached as `<outpath>/<name>/<name>_<seg>.npy` and re-used on a later run, and the
    segments are stacked.  `read_frames(start, stop)` returns the resized uint8 frames [start, stop) as (F, H, W, 3) (the decoded
    ones with `resize=...` in `kw`, 4:2:0 frames (F, 3H/2, W) with `pixel_format=...`, see extract_video_frames).  With `clip_stride` in `kw` a segment owns the windows that start
    in it (segment_windows) and its files are `<name>_s<stride>_<seg>.npy`: a cache made at one stride is never read at another.
    With `crops` in `kw` the features are (n_clips, len(crops), 2048) and the files carry the set too, behind the stride:
    `<name>_s8_c4_<seg>.npy`.  With `frame_step` in `kw` the step comes first: `<name>_d2_<seg>.npy`, `<name>_d2_s8_c4_<seg>.npy`.
    With `normalize` in `kw` its tag comes last: `<name>_npix_<seg>.npy`, `<name>_d2_s8_c4_nch-1f3a..._<seg>.npy`."""
    fpc = kw.get("frames_per_clip", FRAMES_PER_CLIP)
    s, crops, d = resolve_sampling(fpc, kw.get("clip_stride"), kw.get("crops"), kw.get("frame_step"))
    nc = len(crops)
    tag = feature_tag(fpc, s, crops, d, kw.get("normalize"))
    seg_folder = os.path.join(outpath, name)
    plan = segment_windows(n_frames, seg_len, fpc, s, d)  # (refuses a seg_len the stride does not divide before anything is written)
    os.makedirs(seg_folder, exist_ok=True)
    segments = []
    for seg, _w0, _w1, lo, hi in plan:
        seg_path = os.path.join(seg_folder, f"{name}{tag}_{seg}.npy")
        if os.path.exists(seg_path):
            out = np.load(seg_path)
        else:
            out = extract_video_frames(model, read_frames(lo, hi), **kw)
            np.save(seg_path, out)
        segments.append(out.reshape(-1, nc, 2048))
    return np.vstack(segments)


def extract_frames(sources: Iterable[Tuple[str, int, Callable[[int, int], torch.Tensor]]], model, outpath: str,
                   long_video_frames: int = SEGMENT_FRAMES, seg_len: int = SEGMENT_FRAMES, **kw) -> Dict[str, str]:
    """Per-video driver for frame sources (name, n_frames, read_frames): `<name>_i3d.npy` per video with the reference's
    skip-if-exists rule (:106-110); videos longer than `long_video_frames` go through the per-segment cache.  With
    `clip_stride` (below frames_per_clip) the files are `<name>_i3d_s<stride>.npy`, with a crop subset
    `<name>_i3d[_s<stride>]_c<digits>.npy`, with `frame_step` `<name>_i3d_d<step>[_s<stride>][_c<digits>].npy`, with `normalize`
    `<name>_i3d[_d<step>][_s<stride>][_c<digits>]_n<kind>[-<hash>].npy` (feature_tag)."""
    os.makedirs(outpath, exist_ok=True)
    fpc = kw.get("frames_per_clip", FRAMES_PER_CLIP)
    d = resolve_frame_step(kw.get("frame_step"))
    s = resolve_clip_stride(fpc, kw.get("clip_stride"), d)
    suffix = "_i3d" + feature_tag(fpc, s, kw.get("crops"), d, kw.get("normalize")) + ".npy"
    written = {}
    for name, n_frames, read_frames in sources:
        savepath = os.path.join(outpath, name + suffix)
        if os.path.exists(savepath):
            continue
        if n_frames > long_video_frames:
            out = extract_long_video_frames(model, name, n_frames, read_frames, outpath, seg_len, **kw)
        else:
            out = extract_video_frames(model, read_frames(0, n_frames), **kw)
        np.save(savepath, out)
        written[name] = savepath
    return written


def extract(sources: Iterable[Tuple[str, Callable[[], torch.Tensor]]], model, outpath: str, **kw) -> Dict[str, str]:
    """Per-video driver with the reference's resume rule: skip a video whose `<name>_i3d.npy`
    exists (:106-110).  `sources` yields (name, loader) where loader() returns the clip tensor."""
    os.makedirs(outpath, exist_ok=True)
    written = {}
    for name, loader in sources:
        savepath = os.path.join(outpath, name + "_i3d.npy")
        if os.path.exists(savepath):
            continue
        np.save(savepath, extract_video(model, loader(), **kw))
        written[name] = savepath
    return written


def segment_array(features: np.ndarray, seg_length: int = 32, device: Optional[torch.device] = None) -> np.ndarray:
    """(n_clips, 10, C) -> (10, seg_length, C) float32, bucket means on the GPU (:171-183)."""
    dev = device or torch.device("cuda")
    f = torch.as_tensor(features, dtype=torch.float32).to(dev)
    return mil_ops.segment_features(f, seg_length).cpu().numpy()


def segment(feature_path: str, seg_outpath: str, seg_length: int = 32) -> None:
    """File driver of extract_features.py:159-185 (same skip-if-exists rule)."""
    os.makedirs(seg_outpath, exist_ok=True)
    for file in sorted(os.listdir(feature_path)):
        if not file.endswith(".npy"):
            continue
        savepath = os.path.join(seg_outpath, file)
        if os.path.exists(savepath):
            continue
        np.save(savepath, segment_array(np.load(os.path.join(feature_path, file)), seg_length))


def two_stream_features(rgb_model, flow_model, rgb_clips: torch.Tensor, flow_clips: torch.Tensor) -> torch.Tensor:
    """(B, 2048) rows of a two-stream I3D (BASELINE config 5): the mean of the RGB backbone's and the flow backbone's
    (`I3Res50(in_channels=2)`) features of the same crop-clips -- late fusion into the 2 048-d row the MGFN scorer expects
    (`segment` / `FeatureDataset.add_magnitude` / the scorer downstream are unchanged).  NOT IN THE REFERENCE, which is RGB-only
    (/root/reference/src/i3d.py:202-209: no flow stem, no fusion rule): unpinned by construction, checked against the oracle's
    generic arithmetic only.  Both forwards are the fused HIP plan; the mean is one elementwise launch."""
    if rgb_clips.shape[0] != flow_clips.shape[0] or rgb_clips.shape[2:] != flow_clips.shape[2:]:
        raise ValueError(f"two_stream_features: RGB clips {tuple(rgb_clips.shape)} and flow clips {tuple(flow_clips.shape)} do not describe the same crop-clips")
    with torch.no_grad():
        fr = rgb_model(rgb_clips).reshape(rgb_clips.shape[0], -1)
        ff = flow_model(flow_clips).reshape(flow_clips.shape[0], -1)
        return (fr + ff) * 0.5
