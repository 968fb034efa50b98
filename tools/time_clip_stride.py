#!/usr/bin/env python3
"""Dense extraction (clip_stride) against what a user had before it; one JSON record -> argv[1] (default
profiles/clip_stride_run.json).  Frames resident on the device; two sources: 240x320 decoded frames resized on the device
(resize=256) and 256x340 frames resized beforehand.

1. windows/s of extract_video_frames(clip_stride=s) at s = 16, 8, 4 (skipped on a tree that has no clip_stride argument).
2. the baseline: the overlapping windows gathered into a new uint8 tensor on the device (the gather inside the timed
   window, last window LoopPad-ed by index), then extract_video_frames without the argument -- runs on any commit, as does
   the plain back-to-back call ("no argument").
Every timed call ends in .cpu() (synchronised); the configurations are alternated, `--reps` rounds, every round's value kept.
peak_MiB: torch's peak allocated device memory over one untimed call of each configuration, above what was allocated before it.

    python tools/time_clip_stride.py [out.json] [--frames 384] [--reps 5] [--label TEXT]
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
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "clip_stride_run.json"))
ap.add_argument("--frames", type=int, default=384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_clip_stride: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
FPC = 16
has_stride = "clip_stride" in inspect.signature(extract_video_frames).parameters


def window_index(F, s):
    n = 1 + max(0, -(-(F - FPC) // s))
    idx = []
    for w in range(n):
        length = min(FPC, F - w * s)
        idx += [w * s + t % length for t in range(FPC)]
    return n, torch.tensor(idx, device=dev)


m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
rec = {"tool": "tools/time_clip_stride.py", "label": args.label, "device": torch.cuda.get_device_name(0), "video_frames": args.frames,
       "frames_per_clip": FPC, "rounds": args.reps, "has_clip_stride": has_stride, "sources": {}}
SOURCES = {"240x320 decoded, resize=256 on the device": ((240, 320), {"resize": 256}),
           "256x340 resized beforehand": ((256, 340), {})}
for name, ((h, w), kw) in SOURCES.items():
    frames = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (args.frames, h, w, 3), dtype=np.uint8)).to(dev)
    runs, windows = {}, {}
    runs["no argument"] = lambda: extract_video_frames(m, frames, **kw)
    windows["no argument"] = window_index(args.frames, FPC)[0]
    for s in (16, 8, 4):
        n, idx = window_index(args.frames, s)
        if has_stride:
            runs[f"clip_stride={s}"] = lambda s=s: extract_video_frames(m, frames, clip_stride=s, **kw)
            windows[f"clip_stride={s}"] = n
        if s < FPC:
            runs[f"gather+extract s={s}"] = lambda idx=idx: extract_video_frames(m, frames[idx], **kw)
            windows[f"gather+extract s={s}"] = n
    same = {}
    if has_stride:  # faster and different is not faster: the two ways give the same features
        for s in (8, 4):
            same[f"s={s}"] = bool(np.array_equal(runs[f"clip_stride={s}"](), runs[f"gather+extract s={s}"]()))
    for fn in runs.values():  # warm-up: every shape of the timed window
        fn()
    torch.cuda.synchronize()
    peak = {}
    for k, fn in runs.items():
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        peak[k] = round((torch.cuda.max_memory_allocated(dev) - before) / 2**20, 1)
    rates = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()  # ends in .cpu(): synchronised
            rates[k].append(round(windows[k] / (time.perf_counter() - t), 1))
    rec["sources"][name] = {"windows": windows, "same_features": same, "peak_MiB": peak, "windows_per_s": rates,
                            "median": {k: float(np.median(v)) for k, v in rates.items()}}
    print(name, json.dumps(rec["sources"][name]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
