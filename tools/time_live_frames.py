#!/usr/bin/env python3
"""What the live front end costs (anomaly_detection_on_video_amd/live.py: LiveFrames, LiveScorer.step_camera_frames): every one of
N cameras delivers one decoded frame per step, and every clip_stride steps every camera has a clip due, which goes through the
backbone, the feature rings and the scorer; one JSON record -> argv[1] (default profiles/live_frames.json).

N = 16 / 64 / 256 cameras, frames 256 x 340 already at ring size on the device, frames_per_clip 16, crops "center", a scorer
window of 32 clips (full from the start: the feature rings are pre-filled), clip_stride 16 and 8.  Two legs do the same steps on
the same frames:

  (a) LiveScorer.step_camera_frames: the frames go into LiveFrames' rings, due windows are gathered in one launch;
  (b) what one writes without LiveFrames: a (16, FH, FW, 3) tensor per camera rolled forward with torch.cat((h[1:], frame)) at
      every step, and, when the clips are due, torch.stack of the cameras' tensors + LiveScorer.step_frames.

The unit is one CYCLE of clip_stride steps (clip_stride frames per camera, one due clip per camera at its end), in ms.  One
process; per (N, clip_stride) the legs are run alternately (their order rotates from round to round), `--rounds` rounds after a
warm-up round, each timing `--cycles` cycles between two HIP events (the last one synchronised); medians and min-max over the
rounds; `leg_order` keeps which leg ran behind which.  Before timing, both legs are fed the same frames for two cycles and must
give the same score bits.  Also the two new launches alone at each N -- frame_ring_push of N frames, frame_ring_windows of N
windows (16-byte accesses: every operand is 16-byte aligned and a frame is 261 120 bytes) -- next to mil_ops.gather_rows and
mil_ops.ring_windows moving the same byte count as frame_ring_windows, timed the same way, in ms and bytes (read + written) per
second.  Backbone and scorer at synthetic weights (the time does not depend on them).

    python tools/time_live_frames.py [out.json] [--rounds 5] [--cameras 16 64 256] [--strides 16 8] [--label TEXT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "live_frames.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cycles", type=int, default=2)
ap.add_argument("--cameras", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--strides", type=int, nargs="+", default=[16, 8])
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch

from anomaly_detection_on_video_amd import mil_ops
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.live import LiveFrames, LiveScorer
from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_module_state_dict

if not torch.cuda.is_available():
    raise SystemExit("time_live_frames: no GPU visible")
DEV = torch.device("cuda", 0)
FH, FW, FPC, C, W = 256, 340, 16, 2048, args.window
FRAME = FH * FW * 3


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


def alternate(legs, rounds):
    """legs: {name: (step, iters)} -> {name: [ms per step, one per round]}, the legs in turn within every round, the turn moved on by
    one leg from round to round; round -1 warms up."""
    runs = {k: [] for k in legs}
    order, turns = list(legs), []
    for rnd in range(-1, rounds):
        turn = order[rnd % len(order):] + order[:rnd % len(order)]
        for name in turn:
            step, iters = legs[name]
            ms = timed(step, iters)
            if rnd >= 0:
                runs[name].append(ms)
            print(rnd, name, f"{ms:.4f} ms", flush=True)
        if rnd >= 0:
            turns.append([order.index(name) for name in turn])
    return runs, turns


scorer = MGFNForVideoAnomalyDetection(MGFNConfig())
scorer.load_state_dict(synth_module_state_dict(scorer), strict=True)
scorer = scorer.eval().to(DEV)
backbone = I3Res50()
backbone.load_state_dict(synth_i3d_state_dict())
backbone = backbone.eval().to(DEV)

A, B = "(a) step_camera_frames", "(b) per-camera torch.cat roll + torch.stack + step_frames"
rec = {"tool": "tools/time_live_frames.py", "label": args.label, "rounds": args.rounds, "cycles_per_round": args.cycles, "frame_hw": [FH, FW],
       "frames_per_clip": FPC, "crops": "center", "window": W, "device": torch.cuda.get_device_name(0),
       "unit": "ms per cycle of clip_stride steps (every camera delivers clip_stride frames; one clip per camera comes due, is extracted, pushed and scored)",
       "cameras": {}}
with torch.no_grad():
    for n in args.cameras:
        g = torch.Generator().manual_seed(n)
        pool = [torch.randint(0, 256, (n, FH, FW, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(4)]
        fill = [torch.rand((n, 1, C), generator=g).to(DEV) for _ in range(W)]
        cams = tuple(range(n))
        entry = rec["cameras"][str(n)] = {"strides": {}}
        for s in args.strides:
            lf = LiveFrames(n, frame_hw=(FH, FW), frames_per_clip=FPC, clip_stride=s, device=DEV)
            live_a = LiveScorer(scorer, n, window=W, ncrops=1, channels=C, device=DEV)
            live_b = LiveScorer(scorer, n, window=W, ncrops=1, channels=C, device=DEV)
            for f in fill:  # full scorer windows from the start: the padded pass has its steady shape
                live_a.push(cams, f)
                live_b.push(cams, f)
            state = {"hist": [torch.zeros((FPC, FH, FW, 3), dtype=torch.uint8, device=DEV) for _ in range(n)], "k": 0, "ia": 0, "ib": 0,
                     "a": None, "b": None}

            def cycle_a():
                for _ in range(s):
                    state["ia"] += 1
                    got = live_a.step_camera_frames(backbone, lf, cams, pool[state["ia"] % len(pool)], crops="center")
                    if got is not None:
                        state["a"] = got.scores

            def cycle_b():
                hist = state["hist"]
                for _ in range(s):
                    state["ib"] += 1
                    state["k"] += 1
                    frames = pool[state["ib"] % len(pool)]
                    for c in range(n):
                        hist[c] = torch.cat((hist[c][1:], frames[c:c + 1]))
                    k = state["k"]
                    if k >= FPC and (k - FPC) % s == 0:
                        clips = torch.stack(hist).view(n * FPC, FH, FW, 3)
                        state["b"] = live_b.step_frames(backbone, clips, cams, crops="center").scores

            for _ in range(max(2, FPC // s + 1)):  # the same frames to both legs until clips have come due twice: the same bits
                cycle_a()
                cycle_b()
            equal = state["a"] is not None and state["b"] is not None and bool(torch.equal(state["a"], state["b"]))
            if not equal:
                raise SystemExit(f"time_live_frames: (a) and (b) disagree at {n} cameras, clip_stride {s}")
            runs, turns = alternate({A: (cycle_a, args.cycles), B: (cycle_b, args.cycles)}, args.rounds)
            med = {k: float(np.median(v)) for k, v in runs.items()}
            spread_b = max(runs[B]) - min(runs[B])
            entry["strides"][str(s)] = {
                "ms_per_cycle": {k: median_range(v) for k, v in runs.items()}, "ms_per_cycle_runs": runs, "leg_order": turns,
                "a_over_b": round(med[A] / med[B], 4), "a_minus_b_ms": round(med[A] - med[B], 4), "b_spread_ms": round(spread_b, 4),
                "a_not_slower_than_b_by_more_than_b_spread": bool(med[A] - med[B] <= spread_b),
                "every_round_of_a_below_every_round_of_b": bool(max(runs[A]) < min(runs[B])), "a_and_b_same_bits": equal}
            print(json.dumps({"cameras": n, "clip_stride": s, **entry["strides"][str(s)]["ms_per_cycle"]}), flush=True)
            del lf, live_a, live_b, state
            torch.cuda.empty_cache()

        # the two new launches alone, and two existing gathers on the same byte count as frame_ring_windows
        lf = LiveFrames(n, frame_hw=(FH, FW), frames_per_clip=FPC, device=DEV)
        for t in range(FPC):
            lf.push(cams, pool[t % len(pool)])
        ids = torch.arange(n, dtype=torch.int32, device=DEV)
        dst = torch.empty((n * FPC, FH, FW, 3), dtype=torch.uint8, device=DEV)
        rowf = FRAME // 4  # a frame as fp32 elements
        store = lf.ring.view(-1).view(torch.float32).view(n * FPC, rowf)
        idx = torch.randperm(n * FPC, generator=g).to(DEV)
        out_f = torch.empty((n * FPC, rowf), device=DEV)
        ring_f = store.view(n, 1, FPC, rowf)
        counts_f = torch.full((n,), FPC + 3, dtype=torch.int64, device=DEV)
        dst_f = torch.empty((n, 1, FPC, rowf), device=DEV)
        launches, _ = alternate({
            "frame_ring_push (two launches)": (lambda: mil_ops.frame_ring_push(pool[0], ids, lf.ring, lf.counts), 20),
            "frame_ring_windows": (lambda: mil_ops.frame_ring_windows(lf.ring, lf.counts, ids, dst, FPC, 1), 20),
            "gather_rows (same bytes)": (lambda: mil_ops.gather_rows(store, idx, out_f), 20),
            "ring_windows (same bytes)": (lambda: mil_ops.ring_windows(ring_f, counts_f, ids, dst_f), 20)}, args.rounds)
        moved = {"frame_ring_push (two launches)": 2 * n * FRAME, "frame_ring_windows": 2 * n * FPC * FRAME,
                 "gather_rows (same bytes)": 2 * n * FPC * FRAME, "ring_windows (same bytes)": 2 * n * FPC * FRAME}
        entry["launches_ms"] = {k: median_range(v) for k, v in launches.items()}
        entry["launches_ms_runs"] = launches
        entry["bytes_moved"] = moved
        entry["tb_per_s"] = {k: {"median": round(moved[k] / (float(np.median(v)) * 1e-3) / 1e12, 3), "min": round(moved[k] / (max(v) * 1e-3) / 1e12, 3),
                                 "max": round(moved[k] / (min(v) * 1e-3) / 1e12, 3)} for k, v in launches.items()}
        print(json.dumps({"cameras": n, "launches_ms": entry["launches_ms"], "tb_per_s": entry["tb_per_s"]}), flush=True)
        del lf, dst, store, out_f, ring_f, dst_f, pool
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
