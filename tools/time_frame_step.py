#!/usr/bin/env python3
"""Temporal sampling (frame_step) against what a user had before it; one JSON record -> argv[1] (default
profiles/frame_step_run.json).  A 256x340 video resized beforehand, ten crops, from two places: resident on the device, and in
pinned host memory.

1. windows/s of extract_video_frames(frame_step=2), (frame_step=2, clip_stride=5) and (frames_per_clip=8, frame_step=8)
   (skipped on a tree whose extract_video_frames has no frame_step argument: the signature is inspected).
2. the baseline of each: what a user does without the argument -- the sampled frames gathered into a new uint8 tensor
   (frames[::d], or every window's frames for a stride d does not divide; on the device for resident frames, on the host for
   host frames), the gather INSIDE the timed region, then the existing call.  Runs on any commit, as does the plain default
   call ("no argument"), which is the regression guard between two trees.
Every timed call ends in .cpu() (synchronised); the configurations are alternated, `--reps` rounds, every round's value kept.
peak_MiB: torch's peak allocated device memory over one untimed call of each configuration, above what was allocated before it.
h2d_MiB: the uint8 bytes a call moves to the device (host frames), by the arithmetic of what each configuration copies.

    python tools/time_frame_step.py [out.json] [--frames 384] [--reps 5] [--label TEXT] [--only-default]
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
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "frame_step_run.json"))
ap.add_argument("--frames", type=int, default=384)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--label", default="")
ap.add_argument("--only-default", action="store_true", help="time the default call alone (the regression guard between two trees)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_frame_step: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
has_step = "frame_step" in inspect.signature(extract_video_frames).parameters
H, W = 256, 340


def window_index(F, fpc, s, d):
    """(windows, the frames of every window one after the other) by the rule: window w samples frames w s + (t % L) d."""
    n = 1 + max(0, -(-(F - fpc * d) // s))
    idx = []
    for w in range(n):
        length = min(fpc, -(-(F - w * s) // d))
        idx += [w * s + (t % length) * d for t in range(fpc)]
    return n, torch.tensor(idx)


m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
rec = {"tool": "tools/time_frame_step.py", "label": args.label, "device": torch.cuda.get_device_name(0), "video_frames": args.frames,
       "frame_size": [H, W], "rounds": args.reps, "has_frame_step": has_step, "sources": {}}
host = torch.from_numpy(np.random.default_rng(H).integers(0, 256, (args.frames, H, W, 3), dtype=np.uint8)).pin_memory()
FRAME_MIB = H * W * 3 / 2**20
# (name, frames_per_clip, frame_step, clip_stride or None)
CASES = [] if args.only_default else [("frame_step=2", 16, 2, None), ("frame_step=2, clip_stride=5", 16, 2, 5), ("fpc=8, frame_step=8", 8, 8, None)]
for place in ("resident", "pinned host"):
    frames = host.to(dev) if place == "resident" else host
    on_host = place != "resident"
    runs, windows, h2d = {}, {}, {}
    runs["no argument"] = lambda: extract_video_frames(m, frames)
    windows["no argument"] = 1 + max(0, -(-(args.frames - 16) // 16))
    h2d["no argument"] = round(args.frames * FRAME_MIB, 1) if on_host else 0.0
    pairs = []
    for name, fpc, d, s in CASES:
        ss = fpc * d if s is None else s
        n, idx = window_index(args.frames, fpc, ss, d)
        kw = {} if fpc == 16 else {"frames_per_clip": fpc}
        if ss % d == 0:  # the user's way: decimate, then the existing call at stride s / d
            base = f"gather [::{d}] + extract ({name})"
            skw = {} if s is None else {"clip_stride": ss // d}
            runs[base] = lambda d=d, kw=kw, skw=skw: extract_video_frames(m, frames[::d].contiguous(), **kw, **skw)
            h2d[base] = round(-(-args.frames // d) * FRAME_MIB, 1) if on_host else 0.0
        else:  # ... or every window's frames, one after the other
            base = f"gather windows + extract ({name})"
            idx = idx if on_host else idx.to(dev)
            runs[base] = lambda idx=idx, kw=kw: extract_video_frames(m, frames[idx], **kw)
            h2d[base] = round(n * fpc * FRAME_MIB, 1) if on_host else 0.0
        windows[base] = n
        if has_step:
            skw = {} if s is None else {"clip_stride": s}
            runs[name] = lambda d=d, kw=kw, skw=skw: extract_video_frames(m, frames, frame_step=d, **kw, **skw)
            windows[name] = n
            if on_host:  # a lattice when d divides the stride; else each step's span, the overlap between steps twice
                h2d[name] = round(-(-args.frames // d) * FRAME_MIB, 1) if ss % d == 0 else None
            else:
                h2d[name] = 0.0
            pairs.append((name, base))
    errors = {}
    for k in list(runs):  # warm-up, every shape of the timed window; a configuration the tree cannot run is recorded, not timed
        try:
            runs[k]()
        except Exception as e:  # noqa: BLE001
            errors[k] = f"{type(e).__name__}: {e}"[:300]
            del runs[k]
    same = {name: bool(np.array_equal(runs[name](), runs[base]())) for name, base in pairs if name in runs and base in runs}
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
            rates[k].append(round(windows[k] / (time.perf_counter() - t), 2))
    rec["sources"][place] = {"windows": {k: windows[k] for k in runs}, "same_features": same, "peak_MiB": peak,
                             "h2d_MiB": {k: h2d[k] for k in runs}, "windows_per_s": rates,
                             "median": {k: float(np.median(v)) for k, v in rates.items()},
                             "spread": {k: [min(v), max(v)] for k, v in rates.items()}, "errors": errors}
    print(place, json.dumps(rec["sources"][place]), flush=True)
    del frames

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
