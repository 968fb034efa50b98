#!/usr/bin/env python3
"""What regions of interest cost on the live front end (anomaly_detection_on_video_amd/live.py: LiveFrames(rois=), resize.py:
resize_rois_u8): every one of N cameras delivers one decoded 1080 x 1920 frame, resident on the device, and a push brings each
camera's region to the rings' (256, 340); one JSON record -> argv[1] (default profiles/roi.json).

N = 16 / 64 / 256 cameras, packed RGB and NV12 sources.  The legs, each one push of all N cameras:

  (a)      LiveFrames(rois=).push with a distinct box per camera, each a quarter of the frame (camera c: quarter c % 4);
  (a-none) the same with every camera's box None (the whole frame): what the per-frame lookup costs against (c);
  (b)      what one writes without rois, RGB only (a 4:2:0 frame cannot be sliced): per camera frames[c, t:b, l:r].contiguous() +
           resize_u8(out=) into a staging row, then one push of the staged frames.  NOT the same bytes as (a): taps at the crop's
           edge are clipped where Pillow's box reads the neighbouring pixels;
  (c)      the whole-frame push(resize=(256, 340)) of the same frames;
  (d)      N virtual cameras on N / 4 resident frames through source_of (four quarters of each frame), against (a), which reads N
           resident frames: the same launches on a quarter of the held (and uploaded) bytes.

One process; per (N, source) the legs are run alternately (their order rotates from round to round), `--rounds` rounds after a
warm-up round, each timing `--iters` pushes between two HIP events (the last one synchronised); medians and min-max over the
rounds; `leg_order` keeps which leg ran behind which.  Before timing, (a-none) must leave the rings' bytes of (c).  Also the launch
pair alone (resize_rois_u8 into owned output and workspace, issued from Python) with (a)'s tables, in microseconds and in bytes
read + written per second, the bytes counted from the shapes and the tables: the horizontal pass reads `rows` source rows of the
box's columns (3 bytes a pixel, 1.5 for NV12) and writes rows x OW x 3, the vertical pass reads those and writes OH x OW x 3.

    python tools/time_roi.py [out.json] [--rounds 5] [--iters 20] [--cameras 16 64 256] [--label TEXT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "roi.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--cameras", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--source-hw", type=int, nargs=2, default=[1080, 1920])
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch

from anomaly_detection_on_video_amd import resize
from anomaly_detection_on_video_amd.live import LiveFrames

if not torch.cuda.is_available():
    raise SystemExit("time_roi: no GPU visible")
DEV = torch.device("cuda", 0)
(H, W), (FH, FW), FPC = args.source_hw, (256, 340), 16
QUARTERS = [(0, 0, W // 2, H // 2), (W // 2, 0, W, H // 2), (0, H // 2, W // 2, H), (W // 2, H // 2, W, H)]


def median_range(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def timed(step, iters):
    """ms per call of `step` over `iters` calls between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(legs, rounds, iters):
    """legs: {name: step} -> {name: [ms per step, one per round]}, the legs in turn within every round, the turn moved on by one leg
    from round to round; round -1 warms up."""
    runs = {k: [] for k in legs}
    order, turns = list(legs), []
    for rnd in range(-1, rounds):
        turn = order[rnd % len(order):] + order[:rnd % len(order)]
        for name in turn:
            ms = timed(legs[name], iters)
            if rnd >= 0:
                runs[name].append(ms)
            print(rnd, name, f"{ms:.4f} ms", flush=True)
        if rnd >= 0:
            turns.append([order.index(name) for name in turn])
    return runs, turns


def pair_bytes(t, n, bytes_per_pixel):
    """Bytes the launch pair reads + writes for n frames, frame i with table i % n_tables."""
    total = 0
    for i in range(n):
        k = i % t.n_tables
        rows = int(t.rowspan[k, 1])
        cols = int(t.xbounds[k, -1, 0] + t.xbounds[k, -1, 1] - t.xbounds[k, 0, 0])
        total += rows * cols * bytes_per_pixel + 2 * rows * t.out_w * 3 + t.out_h * t.out_w * 3
    return int(total)


A, AN, B, C, D = "(a) rois, a quarter per camera", "(a-none) rois, every box None", "(b) slice + contiguous + resize_u8 per camera, one push", \
    "(c) push(resize=), whole frames", "(d) source_of, 4 cameras per frame"
rec = {"tool": "tools/time_roi.py", "label": args.label, "rounds": args.rounds, "pushes_per_round": args.iters, "source_hw": [H, W],
       "frame_hw": [FH, FW], "frames_per_clip": FPC, "filter": "bilinear", "device": torch.cuda.get_device_name(0),
       "unit": "ms per push of all N cameras (one decoded frame each, resident on the device, into the rings)", "cameras": {}}
for n in args.cameras:
    entry = rec["cameras"][str(n)] = {}
    cams = tuple(range(n))
    boxes = [QUARTERS[c % 4] for c in cams]
    src4 = tuple(c // 4 for c in cams)
    for form in ("rgb", "nv12"):
        torch.manual_seed(n)
        shape = (n, H, W, 3) if form == "rgb" else (n, H * 3 // 2, W)
        frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV)
        kw = {} if form == "rgb" else {"pixel_format": "nv12"}
        make = lambda **more: LiveFrames(n, frame_hw=(FH, FW), frames_per_clip=FPC, device=DEV, **more)  # noqa: E731
        lf_a, lf_n, lf_c, lf_d = make(rois=resize.RoiSpec((H, W), boxes)), make(rois=resize.RoiSpec((H, W), {})), make(), make(rois=resize.RoiSpec((H, W), boxes))
        legs = {A: lambda: lf_a.push(cams, frames, **kw), AN: lambda: lf_n.push(cams, frames, **kw),
                C: lambda: lf_c.push(cams, frames, resize=(FH, FW), **kw), D: lambda: lf_d.push(cams, frames[: -(-n // 4)], source_of=src4, **kw)}
        if form == "rgb":
            lf_b = make()
            staged = torch.empty((n, FH, FW, 3), dtype=torch.uint8, device=DEV)

            def leg_b():
                for c, (l, t, r, b) in enumerate(boxes):
                    resize.resize_u8(frames[c : c + 1, t:b, l:r].contiguous(), (FH, FW), out=staged[c : c + 1])
                lf_b.push(cams, staged)

            legs[B] = leg_b
        legs[AN]()
        legs[C]()
        same = bool(torch.equal(lf_n.ring, lf_c.ring))
        if not same:
            raise SystemExit(f"time_roi: (a-none) and (c) disagree at {n} cameras, {form}")
        runs, turns = alternate(legs, args.rounds, args.iters)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread_c = max(runs[C]) - min(runs[C])
        e = entry[form] = {"ms_per_push": {k: median_range(v) for k, v in runs.items()}, "ms_per_push_runs": runs, "leg_order": turns,
                           "a_none_over_c": round(med[AN] / med[C], 4), "a_none_minus_c_ms": round(med[AN] - med[C], 4), "c_spread_ms": round(spread_c, 4),
                           "a_none_slower_than_c_beyond_c_spread": bool(med[AN] - med[C] > spread_c), "a_none_and_c_same_bytes": same,
                           "d_over_a": round(med[D] / med[A], 4), "resident_source_bytes": {"(a)": int(frames.numel()), "(d)": int(frames[: -(-n // 4)].numel())}}
        if form == "rgb":
            e["a_over_b"] = round(med[A] / med[B], 4)
            e["every_round_of_a_below_every_round_of_b"] = bool(max(runs[A]) < min(runs[B]))
        # the launch pair alone, with (a)'s tables
        t = lf_a._roi_tables
        out = torch.empty((n, FH, FW, 3), dtype=torch.uint8, device=DEV)
        ws = torch.empty((n * t.ws_rows * FW * 3,), dtype=torch.uint8, device=DEV)
        ids = lf_a.cameras.ids(cams)
        pair, _ = alternate({"resize_rois_u8 (two launches)": lambda: resize.resize_rois_u8(frames, t, table_of=ids, out=out, ws=ws, **kw)}, args.rounds, args.iters)
        v = pair["resize_rois_u8 (two launches)"]
        moved = pair_bytes(t, n, 3 if form == "rgb" else 1.5)
        e["launch_pair_us"] = {k: round(x * 1e3, 2) for k, x in median_range(v).items()}
        e["launch_pair_us_runs"] = [round(x * 1e3, 2) for x in v]
        e["launch_pair_bytes_moved"] = moved
        e["launch_pair_tb_per_s"] = {"median": round(moved / (float(np.median(v)) * 1e-3) / 1e12, 3), "min": round(moved / (max(v) * 1e-3) / 1e12, 3),
                                     "max": round(moved / (min(v) * 1e-3) / 1e12, 3)}
        print(json.dumps({"cameras": n, "form": form, **{k: e[k] for k in ("ms_per_push", "launch_pair_us", "launch_pair_tb_per_s")}}), flush=True)
        del lf_a, lf_n, lf_c, lf_d, legs, frames, out, ws
        if form == "rgb":
            del lf_b, staged
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
