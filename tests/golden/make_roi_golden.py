#!/usr/bin/env python3
"""Generate the region-of-interest goldens tests/golden/roi_<H>x<W>.npz with Pillow (nothing else: no package resampling code).

    python -B tests/golden/make_roi_golden.py [--out DIR]

Each file holds one input geometry's PIL `Image.resize((OW, OH), filter, box=box, reducing_gap=None)` outputs for the four
supported filters over a handful of boxes: keys `<filter>/<box name>`, uint8 (OH, OW, 3); `names` and `boxes` (float64 (n, 4) =
left, top, right, bottom, as handed to Pillow), the output size and the Pillow version.  The boxes: integer, fractional, touching
each edge of the frame, under one pixel wide / high, the whole frame on one axis only, an odd left edge.  The input frames are
not stored: they are a pure function of the geometry (weights.hash_uniform), rebuilt by the tests (tests/_roi_ref.roi_input).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from anomaly_detection_on_video_amd.weights import hash_uniform  # noqa: E402

# (in_h, in_w) -> (out_h, out_w)
GEOMETRIES = [
    ((24, 30), (10, 14)),  # down both ways for most boxes, up for the thin ones
    ((13, 11), (17, 9)),   # odd sizes; up vertically
]
FILTERS = {"box": 4, "bilinear": 2, "bicubic": 3, "lanczos": 1}  # PIL.Image.Resampling codes


def boxes(h: int, w: int) -> dict:
    return {
        "integer": (3, 2, w - 5, h - 4),
        "fractional": (1.3, 2.7, w - 3.4, h - 1.15),
        "top_left": (0, 0, w // 2 + 0.5, h // 3),
        "bottom_right": (w / 3.0, h / 2.0, w, h),
        "thin": (w / 2.0 + 0.2, 1, w / 2.0 + 0.9, h - 1),
        "flat": (2, h / 2.0 + 0.1, w - 2, h / 2.0 + 0.6),
        "full_height": (w / 4.0, 0, w - 1.5, h),
        "full_width": (0, 1.25, w, h - 2.5),
        "odd_left": (5, 3, w - 4, h - 3),
    }


def roi_input(h: int, w: int) -> np.ndarray:
    """Seeded noise over the whole range in 2 x 2 blocks: neighbours differ, so a tap beside the box changes bytes."""
    bh, bw = (h + 1) // 2, (w + 1) // 2
    u = hash_uniform(f"roi/1x{h}x{w}", bh * bw * 3)
    blocks = np.minimum((u + 1.0) * 128.0, 255.0).astype(np.uint8).reshape(bh, bw, 3)
    return blocks.repeat(2, axis=0).repeat(2, axis=1)[:h, :w]


def main(out: str) -> None:
    import PIL
    from PIL import Image

    for (h, w), (oh, ow) in GEOMETRIES:
        img = Image.fromarray(roi_input(h, w))
        bx = boxes(h, w)
        arrays = {f"{f}/{name}": np.asarray(img.resize((ow, oh), code, box=box, reducing_gap=None))
                  for f, code in FILTERS.items() for name, box in bx.items()}
        path = os.path.join(out, f"roi_{h}x{w}.npz")
        np.savez_compressed(path, names=np.array(list(bx)), boxes=np.array(list(bx.values()), dtype=np.float64),
                            out_hw=np.array((oh, ow), dtype=np.int64), pillow_version=np.array(PIL.__version__), **arrays)
        print(f"{path}: {h}x{w} -> {oh}x{ow}, {len(arrays)} outputs, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    main(ap.parse_args().out)
