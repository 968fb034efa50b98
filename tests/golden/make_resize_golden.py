#!/usr/bin/env python3
"""Generate the GroupResize goldens tests/golden/resize_<H>x<W>.npz with Pillow (nothing else: no package resampling code).

    python -B tests/golden/make_resize_golden.py [--out DIR]

Each file holds one input geometry's PIL `Image.resize` outputs for the four supported filters (keys `box`, `bilinear`,
`bicubic`, `lanczos`, uint8 (OH, OW, 3)), the requested `size` (one int = torchvision's `Resize(int)` rule, restated below;
two = (h, w) as given), the output size and the Pillow version.  The input frames are not stored: they are a pure function
of the geometry (weights.hash_uniform), rebuilt by the tests (tests/_pil_resample.golden_input).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from anomaly_detection_on_video_amd.weights import hash_uniform  # noqa: E402

# (in_h, in_w) -> size: an int (short side) or (out_h, out_w)
GEOMETRIES = [
    ((240, 320), 256),         # UCF-Crime native -> 256 x 341
    ((480, 640), 256),         # -> 256 x 341
    ((1080, 1920), 256),       # HD -> 256 x 455
    ((100, 33), (341, 256)),   # up both ways, aspect changed
    ((37, 45), 64),            # -> 64 x 77
    ((64, 64), (64, 20)),      # width only
    ((200, 31), (201, 31)),    # height only
    ((7, 5), (1, 1)),
    ((256, 341), 256),         # already at size: unchanged
]
FILTERS = {"box": 4, "bilinear": 2, "bicubic": 3, "lanczos": 1}  # PIL.Image.Resampling codes


def output_size(h: int, w: int, size):
    """torchvision transforms.Resize(size) on an (h, w) image (what GroupResize applies per frame)."""
    if isinstance(size, tuple):
        return size
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    return oh, ow


def golden_input(h: int, w: int) -> np.ndarray:
    """Blocks of uniform random colour, b x b pixels with b = 8 * max(1, min(h, w) // 256) (sharp edges: the filters' overshoot
    reaches the 0 / 255 clamp); a pure function of (h, w).  Random noise instead would not fit the size limit."""
    b = 8 * max(1, min(h, w) // 256)
    bh, bw = (h + b - 1) // b, (w + b - 1) // b
    blocks = np.floor((hash_uniform(f"resize/blocks/{h}x{w}", bh * bw * 3) + 1.0) * 128.0)
    return blocks.reshape(bh, bw, 3).repeat(b, axis=0).repeat(b, axis=1)[:h, :w].astype(np.uint8)


def main(out: str) -> None:
    import PIL
    from PIL import Image

    for (h, w), size in GEOMETRIES:
        oh, ow = output_size(h, w, size)
        img = Image.fromarray(golden_input(h, w))
        arrays = {name: np.asarray(img.resize((ow, oh), code)) for name, code in FILTERS.items()}
        path = os.path.join(out, f"resize_{h}x{w}.npz")
        np.savez_compressed(path, size=np.array(size if isinstance(size, tuple) else (size,), dtype=np.int64),
                            out_hw=np.array((oh, ow), dtype=np.int64), pillow_version=np.array(PIL.__version__), **arrays)
        print(f"{path}: {h}x{w} -> {oh}x{ow}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    main(ap.parse_args().out)
