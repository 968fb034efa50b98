#!/usr/bin/env python3
"""What listing the test set's anomaly events costs on the device (metrics.FrameAucPlan.events: frame scores, smoothing, the
event kernels, one read-back) against the host path a user writes without it: `plan.scores.cpu()`, np.repeat to frames and
events.find_events_host.  One JSON record -> argv[1] (default profiles/events.json).

Corpus: UCF-Crime's test set in size, as tools/time_validation.py's -- `--videos` (290) videos of T ~ U[50, 500] clips of 16
frames, resident as window scores in a FrameAucPlan (smoothed noise in [0, 1]; the scores do not come from a model: what they
are changes how many events there are, not what a pass costs per frame).  The two legs run alternately, `--rounds` rounds after
one warm-up each, in one process: the device leg between two HIP events (and its wall time beside it), the host leg as wall
time; medians and ranges.  Every round's two event lists must agree (integers, peaks and counts equal, means within one fp32 ulp).

The driver starts no GPU work itself: the measurement is a child process under its own `timeout`.

    python tools/time_events.py [out.json] [--rounds 5] [--videos 290] [--label TEXT]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "events.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--videos", type=int, default=290)
ap.add_argument("--label", default="")
ap.add_argument("--step", choices=["measure"], help="(internal) run the measurement in this process")
ap.add_argument("--dir", help="(internal) where the step leaves its record")
args = ap.parse_args()

SPECS = {"smooth=9, merge_gap=32, min_len=16": (0.6, 0.75, 9, 32, 16), "smooth=1, merge_gap=0, min_len=1": (0.6, 0.75, 1, 0, 1),
         "smooth=255, merge_gap=160, min_len=64": (0.55, 0.65, 255, 160, 64)}


def median_range(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def agree(a, b):
    if not (np.array_equal(a.ev_int, b.ev_int) and np.array_equal(a.counts, b.counts) and np.array_equal(a.peak, b.peak)):
        return False
    near = (a.mean == b.mean) | (np.nextafter(a.mean, np.float32(np.inf)) == b.mean) | (np.nextafter(a.mean, np.float32(-np.inf)) == b.mean)
    return bool((near | (np.isnan(a.mean) & np.isnan(b.mean))).all())


def measure():
    import torch

    from anomaly_detection_on_video_amd import events, metrics

    if not torch.cuda.is_available():
        raise SystemExit("time_events: no GPU visible")
    rng = np.random.default_rng(0)
    windows = [int(rng.integers(50, 501)) for _ in range(args.videos)]
    plan = metrics.FrameAucPlan([np.zeros(16 * t, np.float32) for t in windows], windows, 16, device="cuda")
    z = np.convolve(rng.standard_normal(sum(windows) + 30), np.ones(31) / 31, mode="valid")
    plan.scores.copy_(torch.from_numpy(((z - z.min()) / (z.max() - z.min())).astype(np.float32)))
    frames = plan.items.frames
    out = {"corpus": {"test_videos": args.videos, "clips": int(sum(windows)), "frames": int(sum(frames)), "clips_per_video": [min(windows), max(windows)]},
           "device": torch.cuda.get_device_name(0), "specs": {}}
    for name, spec in SPECS.items():
        spec = events.resolve_event_spec(spec)
        dev_ms, dev_wall_ms, host_ms, host_copy_ms = [], [], [], []
        n_events = None
        for rnd in range(-1, args.rounds):  # round -1: the warm-up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = time.perf_counter()
            e0.record()
            ev = plan.events(spec)
            e1.record()
            e1.synchronize()
            wall = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            scores = plan.scores.cpu().numpy()
            copied = (time.perf_counter() - t) * 1e3
            want = events.find_events_host(np.repeat(scores, 16), frames, spec)
            host = (time.perf_counter() - t) * 1e3
            if not agree(ev.numpy(), want):
                raise SystemExit(f"time_events: the device and the host event lists differ ({name})")
            n_events = len(want)
            if rnd >= 0:
                dev_ms.append(e0.elapsed_time(e1))
                dev_wall_ms.append(wall)
                host_ms.append(host)
                host_copy_ms.append(copied)
            print(rnd, name, f"device {e0.elapsed_time(e1):.3f} ms (wall {wall:.3f}), host {host:.3f} ms, {n_events} events", flush=True)
        out["specs"][name] = {"spec": {k: getattr(spec, k) for k in ("low", "high", "smooth", "merge_gap", "min_len")}, "events": n_events,
                              "device_ms_hip_events": median_range(dev_ms), "device_ms_wall": median_range(dev_wall_ms),
                              "host_ms_wall": median_range(host_ms), "of_which_scores_cpu_ms": median_range(host_copy_ms),
                              "host_over_device": round(float(np.median(host_ms)) / float(np.median(dev_ms)), 2)}
    return out


if args.step:
    with open(os.path.join(args.dir, "measure.json"), "w") as f:
        json.dump(measure(), f)
    sys.exit(0)

rec = {"tool": "tools/time_events.py", "label": args.label, "rounds": args.rounds}
with tempfile.TemporaryDirectory() as tmp:
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "measure", "--dir", tmp, "--rounds", str(args.rounds),
           "--videos", str(args.videos)]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
        raise SystemExit(f"time_events: the measurement ended with {rc}")
    with open(os.path.join(tmp, "measure.json")) as f:
        rec.update(json.load(f))
print(json.dumps(rec["specs"]), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
