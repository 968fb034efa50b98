#!/usr/bin/env python3
"""GroupResize on the device against what it replaces; one JSON record -> profiles/resize.json (or argv[1]).

1. resize_u8 per 48 frames (device events over >= 200 calls after warm-up): 240x320 -> 256x341 and 1080x1920 -> 256x455.
2. extract_video_frames crop-clips/s from decoded 240x320 host frames with resize=256 (A) against the same frames resized
   beforehand (B): one model, one process, A and B alternated three times.
3. PIL Image.resize (BILINEAR) ms per frame on this host's CPU, one thread, for the same geometries (what the kernel replaces).
"""
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from anomaly_detection_on_video_amd import resize
from anomaly_detection_on_video_amd.extract import extract_video_frames
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

GEOMS = [((240, 320), (256, 341)), ((1080, 1920), (256, 455))]
if not torch.cuda.is_available():
    raise SystemExit("time_resize: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
rec = {"tool": "tools/time_resize.py", "device": torch.cuda.get_device_name(0), "resize_u8": [], "pil": []}


def frames(n, h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


# 1. kernel time per 48 frames
for (h, w), (oh, ow) in GEOMS:
    x = frames(48, h, w, 1).to(dev)
    out = torch.empty((48, oh, ow, 3), device=dev, dtype=torch.uint8)
    for _ in range(20):
        resize.resize_u8(x, 256, out=out)
    torch.cuda.synchronize()
    n = 300
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        resize.resize_u8(x, 256, out=out)
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / n * 1e3
    p = resize.plan(h, w, oh, ow)
    moved = 48 * (h * w * 3 + 2 * p.rows * ow * 3 + oh * ow * 3)  # read frames, write + read the workspace, write the output
    rec["resize_u8"].append({"geometry": f"{h}x{w}->{oh}x{ow}", "frames": 48, "calls": n, "us_per_call": round(us, 2),
                             "us_per_frame": round(us / 48, 3), "min_bytes": moved, "GB_per_s": round(moved / us / 1e3, 1)})
    print(rec["resize_u8"][-1], flush=True)

# 2. crop-clips/s: decoded frames resized inside the driver (A) vs frames resized beforehand (B)
m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
F = 96  # 6 clips = 60 crop-clips per video
decoded = frames(F, 240, 320, 2)
pre = resize.resize_u8(decoded.to(dev), 256).cpu()
runs = {"A_resize_on_device": lambda: extract_video_frames(m, decoded, resize=256),
        "B_preresized": lambda: extract_video_frames(m, pre)}
same = np.array_equal(runs["A_resize_on_device"](), runs["B_preresized"]())
for fn in runs.values():
    fn()
torch.cuda.synchronize()
rates = {k: [] for k in runs}
reps = 6
for _ in range(3):
    for k, fn in runs.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()  # ends in .cpu(): synchronised
        rates[k].append(reps * F // 16 * 10 / (time.perf_counter() - t))
rec["extract"] = {"frames": "240x320 decoded, host uint8", "video_frames": F, "crop_clips_per_video": F // 16 * 10, "videos_per_window": reps,
                  "same_features": bool(same), "crop_clips_per_s": {k: [round(v, 1) for v in r] for k, r in rates.items()},
                  "ratio_A_over_B_median": round(float(np.median(rates["A_resize_on_device"]) / np.median(rates["B_preresized"])), 4)}
print(rec["extract"], flush=True)

# 3. PIL on the host, one thread
try:
    import PIL
    from PIL import Image

    for (h, w), (oh, ow) in GEOMS:
        imgs = [Image.fromarray(f) for f in frames(16, h, w, 3).numpy()]
        for im in imgs[:2]:
            im.resize((ow, oh), Image.BILINEAR)
        t = time.perf_counter()
        for _ in range(3):
            for im in imgs:
                im.resize((ow, oh), Image.BILINEAR)
        ms = (time.perf_counter() - t) / (3 * len(imgs)) * 1e3
        rec["pil"].append({"geometry": f"{h}x{w}->{oh}x{ow}", "ms_per_frame": round(ms, 3)})
    rec["pil_version"] = PIL.__version__
    rec["pil_host"] = platform.processor() or platform.machine()
except ImportError:
    rec["pil"] = "PIL not importable on this host: not measured"
print(rec["pil"], flush=True)

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resize.json")
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", path)
