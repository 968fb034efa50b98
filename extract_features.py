#!/usr/bin/env python3
"""I3D feature extraction entry point (the reference's extract_features.py surface).

    python extract_features.py --outdir OUT [--videos N] [--weights path.pt | --synthetic-weights] [--frame-size HxW [--clip-stride N] [--frame-step N] [--crops SET] [--normalize SPEC] [--pixel-format FMT [--surface GEOMETRY]]]

The reference decodes the UCF-Crime videos with decord + torchvision TenCrop (not available in
the MI355X image, and outside the hot path).  Here the video source is synthetic TenCrop'd clip
tensors of the same layout; plug a real decoder in by passing (name, loader) pairs to
`anomaly_detection_on_video_amd.extract.extract`.  With `--frame-size HxW` the source is synthetic DECODED uint8 frames of
that size instead, resized (GroupResize(256)), ten-cropped and normalised on the device: `extract_frames(..., resize=256)`,
the entry point for a real decoder's (name, n_frames, read_frames) triples.  `--clip-stride N` (with `--frame-size`) extracts a
16-frame window every N frames instead of every 16 (`<name>_i3d_s<N>.npy`); the windows overlap in place on the device.
`--crops ten|five|center|center_flip|0,4,9` (with `--frame-size`) extracts only those of TenCrop's ten crops
(`<name>_i3d[_s<N>]_c<digits>.npy`, features (n_clips, len(SET), 2048)): a tenth to all of the backbone work per clip.
`--frame-step N` (with `--frame-size`) samples every N-th frame: a window is 16 frames out of a span of 16 x N, windows start
every `--clip-stride` frames (1 .. 16 x N, default the span), files are `<name>_i3d_d<N>[_s<stride>][_c<digits>].npy`.
`--normalize SPEC` (with `--frame-size`) replaces the reference's (x - 114.75) / 57.375 by another of its normalisers, on the device:
`standardize:MEAN:STD` (each one number or three, e.g. `standardize:123.675,116.28,103.53:58.395,57.12,57.375`), `pixel_minmax` or
`pixel_minmax:LO,HI` (e.g. `pixel_minmax:-1,1`), `channel_minmax`, `channel_minmax:LO,HI` or `channel_minmax:LO,LO,LO:HI,HI,HI`; the
files carry the normalisation last in their name (`<name>_i3d..._npix-<hash>.npy`).
`--pixel-format nv12|i420[:bt601|bt709][:limited|full]` (with `--frame-size`, both sizes even) makes the source the decoder's own
8-bit 4:2:0 frames, uint8 (F, 3H/2, W): the colour conversion runs on the device inside the resize (file names do not change).
`--surface pitch=2048,rows=1088,bits=10,shift=6,order=vu` (with `--pixel-format`; any subset of the keys, also `chroma_pitch=` and
`y_offset=`) makes the source a decoder's surfaces, uint8 (F, frame_bytes) with that row pitch, allocated rows, sample depth and
chroma order (`resize.surface`), read in place on the device.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from anomaly_detection_on_video_amd.extract import extract, extract_frames, load_feature_extraction_model, segment  # noqa: E402,F401


def synthetic_sources(n_videos: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed)
    for i in range(n_videos):
        n_clips = int(torch.randint(2, 6, (1,), generator=g))
        name = ("Normal_Videos_%03d_x264" if i % 2 == 0 else "Abuse%03d_x264") % i
        yield name, (lambda n=n_clips, s=seed + i: torch.randn((n, 10, 16, 3, 224, 224), generator=torch.Generator().manual_seed(s)))


def synthetic_frame_sources(n_videos: int, frame_size, seed: int = 0, pixel_format=None, surface=None):
    """(name, n_frames, read_frames) of synthetic decoded uint8 (F, H, W, 3) videos of 2-5 clips plus a few frames; with a
    `pixel_format` the frames are seeded random 4:2:0 ones, (F, 3H/2, W); with a `surface` (a resize.Surface) seeded random
    surfaces, (F, surface.frame_bytes_min), with noise in the padding and in the bits a 10-bit sample ignores."""
    g = torch.Generator().manual_seed(seed)
    h, w = frame_size
    shape = (h, w, 3) if pixel_format is None else (h // 2 * 3, w)
    if surface is not None:
        shape = (surface.frame_bytes_min,)
    for i in range(n_videos):
        n_frames = int(torch.randint(2 * 16, 6 * 16, (1,), generator=g))
        name = ("Normal_Videos_%03d_x264" if i % 2 == 0 else "Abuse%03d_x264") % i

        def read_frames(lo, hi, n=n_frames, s=seed + i):  # the same video on every call (a decoder reads a range of it)
            return torch.randint(0, 256, (n, *shape), generator=torch.Generator().manual_seed(s), dtype=torch.uint8)[lo:hi]

        yield name, n_frames, read_frames


def parse_frame_size(text: str):
    try:
        h, w = (int(v) for v in text.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--frame-size wants HxW, e.g. 240x320; got {text!r}")
    if h < 1 or w < 1:
        raise argparse.ArgumentTypeError(f"--frame-size {text!r}: sizes must be >= 1")
    return h, w


def parse_crops(text: str):
    """--crops: a name of ops.CROP_SETS or comma-separated TenCrop indices, e.g. 0,4,9 -> the validated tuple."""
    from anomaly_detection_on_video_amd.ops import CROP_SETS, resolve_crops

    try:
        return resolve_crops(text if text in CROP_SETS else tuple(int(v) for v in text.split(",")))
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--crops {text!r}: {e}")


def parse_normalize(text: str):
    """--normalize: KIND, KIND:A,B (two scalars) or KIND:A:B (each one number or three, comma-separated) -> ops.Normalize."""
    from anomaly_detection_on_video_amd.ops import resolve_normalize

    def numbers(part):
        v = tuple(float(x) for x in part.split(","))
        return v[0] if len(v) == 1 else v

    try:
        kind, *parts = text.split(":")
        if not parts:
            return resolve_normalize(kind)
        if len(parts) == 1:
            pair = numbers(parts[0])
            if not isinstance(pair, tuple) or len(pair) != 2:
                raise ValueError("KIND:A,B takes two numbers; per-channel values go in KIND:A,A,A:B,B,B")
            return resolve_normalize((kind, pair[0], pair[1]))
        if len(parts) == 2:
            return resolve_normalize((kind, numbers(parts[0]), numbers(parts[1])))
        raise ValueError("KIND, KIND:A,B or KIND:A:B")
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--normalize {text!r}: {e}")


def parse_pixel_format(text: str):
    """--pixel-format: LAYOUT[:MATRIX][:RANGE], e.g. nv12, i420:bt709, nv12:bt601:full -> resize.PixelFormat."""
    from anomaly_detection_on_video_amd.resize import resolve_pixel_format

    try:
        return resolve_pixel_format(tuple(text.split(":")))
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--pixel-format {text!r}: {e}")


_SURFACE_KEYS = ("pitch", "rows", "chroma_pitch", "bits", "shift", "y_offset")


def parse_surface(text: str):
    """--surface: comma-separated KEY=VALUE with the keys pitch, rows, chroma_pitch, bits, shift, y_offset (integers) and order
    (uv | vu) -> the keyword arguments of resize.surface."""
    kw = {}
    try:
        for item in text.split(","):
            key, sep, value = item.partition("=")
            if not sep or key in kw or (key == "order" and "chroma_order" in kw):
                raise ValueError(f"{item!r} is not KEY=VALUE, or repeats a key")
            if key == "order":
                if value not in ("uv", "vu"):
                    raise ValueError(f"order {value!r} is neither uv nor vu")
                kw["chroma_order"] = value
            elif key in _SURFACE_KEYS:
                kw[key] = int(value)
            else:
                raise ValueError(f"unknown key {key!r} (pitch, rows, chroma_pitch, bits, shift, y_offset, order)")
    except ValueError as e:
        raise argparse.ArgumentTypeError(f"--surface {text!r}: {e}")
    return kw


def main(outdir: str = "ucf_crime", videos: int = 4, weights: str = None, synthetic_weights: bool = False,
         model_name: str = "i3d_8x8_r50", frame_size=None, clip_stride: int = None, crops=None, frame_step: int = None,
         normalize=None, pixel_format=None, surface=None):
    """`model_name` defaults to the reference's (extract_features.py:34,46); that variant is parity-unpinned here (a warning
    says so) -- `--model-name tushar-n-baseline` is the I3Res50 pinned against the reference."""
    if clip_stride is not None and frame_size is None:
        raise ValueError("--clip-stride needs --frame-size: the clip-tensor source has no frames to stride over")
    if frame_step is not None and frame_size is None:
        raise ValueError("--frame-step needs --frame-size: the clip-tensor source has no frames to sample")
    if frame_step is not None and frame_step < 1:
        raise ValueError(f"--frame-step {frame_step} must be at least 1")
    span = 16 * (frame_step or 1)
    if clip_stride is not None and not 1 <= clip_stride <= span:
        raise ValueError(f"--clip-stride {clip_stride} outside [1, {span}]")
    if crops is not None and frame_size is None:
        raise ValueError("--crops needs --frame-size: the clip-tensor source is already ten-cropped")
    if normalize is not None and frame_size is None:
        raise ValueError("--normalize needs --frame-size: the clip-tensor source is normalised already")
    if pixel_format is not None and frame_size is None:
        raise ValueError("--pixel-format needs --frame-size: the clip-tensor source holds no decoded frames")
    if pixel_format is not None and (frame_size[0] % 2 or frame_size[1] % 2):
        raise ValueError(f"--pixel-format needs an even frame size (4:2:0 chroma), got {frame_size[0]}x{frame_size[1]}")
    if surface is not None:
        if pixel_format is None:
            raise ValueError("--surface needs --pixel-format: the geometry describes 4:2:0 frames")
        from anomaly_detection_on_video_amd import resize as resize_mod

        surface = resize_mod.surface(pixel_format, *frame_size, **surface)
        surface = resize_mod.resolve_surface(surface, pixel_format, surface.frame_bytes_min)
    if synthetic_weights:
        os.environ["ADV_I3D_SYNTHETIC"] = "1"
    model, _device = load_feature_extraction_model(model_name, state_dict_path=weights, check_model_size=True)
    outpath = os.path.join(outdir, "anomaly_features", "train")
    if frame_size is None:
        extract(synthetic_sources(videos), model, outpath)
    else:  # decoded frames: GroupResize(256) + TenCrop + normalise on the device
        extract_frames(synthetic_frame_sources(videos, frame_size, pixel_format=pixel_format, surface=surface), model, outpath, resize=256,
                       clip_stride=clip_stride, crops=crops, frame_step=frame_step, normalize=normalize, pixel_format=pixel_format,
                       **({} if surface is None else {"surface": surface}))
    seg_length = 32
    segment(outpath, os.path.join(outdir, f"segment_features_{seg_length}"), seg_length)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default="ucf_crime")
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--model-name", default="i3d_8x8_r50", choices=["i3d_8x8_r50", "tushar-n-baseline"],
                    help="the reference's default is i3d_8x8_r50 (parity-unpinned here); tushar-n-baseline = the pinned in-repo I3Res50")
    ap.add_argument("--frame-size", type=parse_frame_size, default=None, metavar="HxW",
                    help="feed synthetic decoded uint8 frames of this size, resized to 256 on the device (default: ten-cropped clip tensors)")
    ap.add_argument("--clip-stride", type=int, default=None, metavar="N",
                    help="with --frame-size: a 16-frame window every N frames (1..16 x frame step; default: that span, back-to-back windows)")
    ap.add_argument("--frame-step", type=int, default=None, metavar="N",
                    help="with --frame-size: temporal sampling, a window is every N-th frame of a span of 16 x N frames (default 1)")
    ap.add_argument("--crops", type=parse_crops, default=None, metavar="SET",
                    help="with --frame-size: ten (default), five, center, center_flip, or ascending TenCrop indices such as 0,4,9")
    ap.add_argument("--normalize", type=parse_normalize, default=None, metavar="SPEC",
                    help="with --frame-size: standardize:MEAN:STD, pixel_minmax[:LO,HI] or channel_minmax[:LO,HI | :LO,LO,LO:HI,HI,HI] "
                         "(default: the reference's (x - 114.75) / 57.375)")
    ap.add_argument("--pixel-format", type=parse_pixel_format, default=None, metavar="FMT",
                    help="with --frame-size: the frames are 8-bit 4:2:0, nv12 or i420 (yuv420p), optionally :bt601 (default) or :bt709 and "
                         ":limited (default) or :full; converted on the device (default: packed RGB)")
    ap.add_argument("--surface", type=parse_surface, default=None, metavar="GEOMETRY",
                    help="with --pixel-format: the frames are decoder surfaces, KEY=VALUE pairs such as pitch=2048,rows=1088,bits=10,shift=6,order=vu "
                         "(also chroma_pitch=, y_offset=); default: compact 8-bit frames")
    a = ap.parse_args()
    if a.clip_stride is not None and a.frame_size is None:
        ap.error("--clip-stride needs --frame-size: the clip-tensor source has no frames to stride over")
    if a.frame_step is not None and a.frame_size is None:
        ap.error("--frame-step needs --frame-size: the clip-tensor source has no frames to sample")
    if a.frame_step is not None and a.frame_step < 1:
        ap.error(f"--frame-step {a.frame_step} must be at least 1")
    if a.clip_stride is not None and not 1 <= a.clip_stride <= 16 * (a.frame_step or 1):
        ap.error(f"--clip-stride {a.clip_stride} outside [1, {16 * (a.frame_step or 1)}]")
    if a.crops is not None and a.frame_size is None:
        ap.error("--crops needs --frame-size: the clip-tensor source is already ten-cropped")
    if a.normalize is not None and a.frame_size is None:
        ap.error("--normalize needs --frame-size: the clip-tensor source is normalised already")
    if a.pixel_format is not None and a.frame_size is None:
        ap.error("--pixel-format needs --frame-size: the clip-tensor source holds no decoded frames")
    if a.pixel_format is not None and (a.frame_size[0] % 2 or a.frame_size[1] % 2):
        ap.error(f"--pixel-format needs an even frame size (4:2:0 chroma), got {a.frame_size[0]}x{a.frame_size[1]}")
    if a.surface is not None and a.pixel_format is None:
        ap.error("--surface needs --pixel-format: the geometry describes 4:2:0 frames")
    main(a.outdir, a.videos, a.weights, a.synthetic_weights, a.model_name, a.frame_size, a.clip_stride, a.crops, a.frame_step, a.normalize,
         a.pixel_format, a.surface)
