#!/usr/bin/env python3
"""Normalisation modes of the uint8-frame path against the default call of the same build; one JSON record -> argv[1] (default
profiles/normalize_run.json).  A 256x340 video resized beforehand, ten crops, from two places: resident on the device, and in
pinned host memory (the method of tools/time_frame_step.py).

1. the statistics kernel alone (ops.crop_minmax_u8) on 48 frames of 256x340: HIP-event time per launch over `--stat-reps`
   launches, after a warm-up, and the bytes its windows cover (skipped on a tree without it).
2. windows/s of extract_video_frames for the default call ("no argument": runs on any commit, the regression guard between two
   trees) and for each mode -- per-channel standardize, pixel_minmax at (-1, 1), channel_minmax at (0, 1) -- on a tree whose
   extract_video_frames has the `normalize` argument (the signature is inspected).
Every timed call ends in .cpu() (synchronised); the configurations are alternated, `--reps` rounds, every round's value kept;
"ratio_to_default" is median over median within this run.

    python tools/time_normalize.py [out.json] [--frames 384] [--reps 5] [--label TEXT] [--only-default]
"""
import argparse
import inspect
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from anomaly_detection_on_video_amd import ops
from anomaly_detection_on_video_amd.extract import extract_video_frames
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "normalize_run.json"))
ap.add_argument("--frames", type=int, default=384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--stat-reps", type=int, default=200)
ap.add_argument("--label", default="")
ap.add_argument("--only-default", action="store_true", help="time the default call alone (the regression guard between two trees)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_normalize: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
has_modes = "normalize" in inspect.signature(extract_video_frames).parameters
H, W = 256, 340

m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
rec = {"tool": "tools/time_normalize.py", "label": args.label, "device": torch.cuda.get_device_name(0), "video_frames": args.frames,
       "frame_size": [H, W], "rounds": args.reps, "has_normalize": has_modes, "sources": {}}
host = torch.from_numpy(np.random.default_rng(H).integers(0, 256, (args.frames, H, W, 3), dtype=np.uint8)).pin_memory()

if has_modes and not args.only_default:
    from anomaly_detection_on_video_amd import _lib

    fr = host[:48].to(dev)
    stats = torch.empty((48, 6, 3, 2), device=dev, dtype=torch.uint8)
    lib, st = _lib.load(), _lib.stream()

    def launch():  # the entry point itself on a preallocated table: no allocation, no wrapper checks
        _lib.check(lib.advhip_crop_minmax_u8(fr.data_ptr(), stats.data_ptr(), 48, H, W, 3, 224, 1, st), "crop_minmax_u8")

    def event_us(fn, reps):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / reps

    us = event_us(launch, args.stat_reps)
    us_wrapped = event_us(lambda: ops.crop_minmax_u8(fr, 224), args.stat_reps)
    assert torch.equal(stats, ops.crop_minmax_u8(fr, 224))
    window_bytes = 48 * 6 * 224 * 224 * 3
    rec["crop_minmax_u8"] = {"frames": 48, "crop": 224, "launches": args.stat_reps, "us_per_launch": round(us, 2),
                             "us_per_wrapper_call": round(us_wrapped, 2),
                             "how": "HIP events around back-to-back launches on one stream, divided by their number",
                             "window_MB": round(window_bytes / 1e6, 2), "frame_MB": round(48 * H * W * 3 / 1e6, 2),
                             "GB_per_s_of_window_bytes": round(window_bytes / us / 1e3, 1)}
    print("crop_minmax_u8", json.dumps(rec["crop_minmax_u8"]), flush=True)
    del fr

MODES = [] if args.only_default or not has_modes else [
    ("standardize per channel", ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))),
    ("pixel_minmax (-1, 1)", ("pixel_minmax", -1.0, 1.0)),
    ("channel_minmax (0, 1)", "channel_minmax"),
]
n_windows = 1 + max(0, -(-(args.frames - 16) // 16))
for place in ("resident", "pinned host"):
    frames = host.to(dev) if place == "resident" else host
    runs = {"no argument": lambda: extract_video_frames(m, frames)}
    for name, spec in MODES:
        runs[name] = lambda spec=spec: extract_video_frames(m, frames, normalize=spec)
    for fn in runs.values():  # warm-up: every shape of the timed window
        fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()  # ends in .cpu(): synchronised
            rates[k].append(round(n_windows / (time.perf_counter() - t), 2))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    rec["sources"][place] = {"windows": n_windows, "windows_per_s": rates, "median": med,
                             "spread": {k: [min(v), max(v)] for k, v in rates.items()},
                             "ratio_to_default": {k: round(v / med["no argument"], 4) for k, v in med.items() if k != "no argument"}}
    print(place, json.dumps(rec["sources"][place]), flush=True)
    del frames

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
