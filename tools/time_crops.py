#!/usr/bin/env python3
"""Crop subsets (crops=) of extract_video_frames: what the default costs after the change, and what a subset buys; one JSON
record -> argv[1] (default profiles/crops_run.json).

Sources: 256x340 frames resident on the device; the same frames in pinned host memory (copied per step); 240x320 decoded
frames in pinned host memory, resized on the device (resize=256).
Configurations: the call without the argument (runs on any commit: the bar for the default is the PARENT's run of this
tool, alternated with this tree's on one box), and -- on a tree that has the argument -- crops = "ten", "five", "center_flip",
"center" at their default clips_per_step (3, 6, 15, 30: about 30 crop-clips per step).
Every timed call ends in .cpu() (synchronised); the configurations are alternated, `--reps` rounds, every round's value kept.

    python tools/time_crops.py [out.json] [--frames 384] [--reps 5] [--label TEXT]
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

from anomaly_detection_on_video_amd.extract import extract_video_frames
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "crops_run.json"))
ap.add_argument("--frames", type=int, default=384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_crops: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
FPC = 16
has_crops = "crops" in inspect.signature(extract_video_frames).parameters
NAMED = {"ten": 10, "five": 5, "center_flip": 2, "center": 1}

m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
n_clips = -(-args.frames // FPC)
rec = {"tool": "tools/time_crops.py", "label": args.label, "device": torch.cuda.get_device_name(0), "video_frames": args.frames,
       "clips": n_clips, "rounds": args.reps, "has_crops": has_crops, "sources": {}}
SOURCES = {"256x340 resident": ((256, 340), True, {}),
           "256x340 pinned host": ((256, 340), False, {}),
           "240x320 decoded pinned host, resize=256": ((240, 320), False, {"resize": 256})}
for name, ((h, w), resident, kw) in SOURCES.items():
    host = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (args.frames, h, w, 3), dtype=np.uint8))
    frames = host.to(dev) if resident else host.pin_memory()
    runs, nc, per_step = {}, {}, {}
    runs["no argument"] = lambda: extract_video_frames(m, frames, **kw)
    nc["no argument"], per_step["no argument"] = 10, 3
    same = {}
    if has_crops:
        for c, k in NAMED.items():
            runs[c] = lambda c=c: extract_video_frames(m, frames, crops=c, **kw)
            nc[c], per_step[c] = k, max(1, 30 // k)
        ten = runs["no argument"]()
        same["ten == no argument"] = bool(np.array_equal(runs["ten"](), ten))
        # (a subset's rows are the ten-crop rows bit for bit at equal launch positions -- the tests; across the different step
        # cuts used here they agree to fp32 rounding: the largest relative difference is recorded)
        for c, idx in (("five", [0, 1, 2, 3, 4]), ("center_flip", [4, 9]), ("center", [4])):
            got = runs[c]()
            same[f"{c} vs ten: max rel diff"] = float(np.max(np.abs(got - ten[:, idx])) / np.max(np.abs(ten)))
    for fn in runs.values():  # warm-up: every shape of the timed window
        fn()
    torch.cuda.synchronize()
    secs = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()  # ends in .cpu(): synchronised
            secs[k].append(time.perf_counter() - t)
    clips_s = {k: [round(n_clips / s, 1) for s in v] for k, v in secs.items()}
    step_mb = {k: round(((per_step[k] - 1) * FPC + FPC) * h * w * 3 / 1e6, 1) for k in runs}
    rec["sources"][name] = {"crops_per_clip": nc, "clips_per_step": per_step, "frame_MB_per_step": step_mb, "checks": same,
                            "clips_per_s": clips_s,
                            "median_clips_per_s": {k: float(np.median(v)) for k, v in clips_s.items()},
                            "median_crop_clips_per_s": {k: round(float(np.median(v)) * nc[k], 1) for k, v in clips_s.items()}}
    print(name, json.dumps(rec["sources"][name]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
