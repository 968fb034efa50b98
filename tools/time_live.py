#!/usr/bin/env python3
"""What one live-scoring step costs (anomaly_detection_on_video_amd/live.py): every one of N cameras pushes one clip and all N
sliding windows are re-scored; one JSON record -> argv[1] (default profiles/live.json).

N = 16 / 64 / 256 cameras, W = 32 clips, 10 crops, C = 2048, every window full (the steady state).  Three legs do the same step:

  (a) LiveScorer.push + LiveScorer.score: rings on the device, one padded pass;
  (b) what can be written without the rings: the windows kept as one (N, 10, W, C + 1) tensor, moved on with torch.cat of
      win[:, :, 1:] and the new clips (mil_ops.add_magnitude_np appends their magnitude channel), then ONE
      scorer.score_padded call on it with prebuilt lengths;
  (c) the same windows scored camera by camera with scorer(video=win[v:v+1]).

One process; per N the legs are run alternately (their order rotates from round to round), `--rounds` rounds after a warm-up
round, each round timing `iters` steps between two HIP events (the last one synchronised); medians and min-max over the rounds,
in ms per step; `leg_order` keeps which leg ran behind which.  Before timing, (a) and (b) are fed the same clips and must give
the same bits.  Also the three new launches alone (ring_push, ring_windows, crop_mean_last) at
each N, timed the same way.  The scorer is the default MGFN at synthetic weights (the time does not depend on them).

    python tools/time_live.py [out.json] [--rounds 5] [--cameras 16 64 256] [--label TEXT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "live.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cameras", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--crops", type=int, default=10)
ap.add_argument("--channels", type=int, default=2048)
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch

from anomaly_detection_on_video_amd import mil_ops
from anomaly_detection_on_video_amd.live import LiveScorer
from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
from anomaly_detection_on_video_amd.models.mgfn.modeling_mgfn import PaddedLens
from anomaly_detection_on_video_amd.weights import synth_module_state_dict

if not torch.cuda.is_available():
    raise SystemExit("time_live: no GPU visible")
DEV = torch.device("cuda", 0)
W, K, C = args.window, args.crops, args.channels


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
    one leg from round to round (the leg behind the host-bound one finds the device's clocks lowered); round -1 warms up."""
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

A, B, PER_CAM = "(a) LiveScorer push + score", "(b) torch.cat windows + add_magnitude_np + one score_padded", "(c) the same windows, one scorer pass per camera"
rec = {"tool": "tools/time_live.py", "label": args.label, "rounds": args.rounds, "window": W, "crops": K, "channels": C,
       "device": torch.cuda.get_device_name(0), "unit": "ms per step (every camera pushes one clip, every window is scored)", "cameras": {}}
with torch.no_grad():
    for n in args.cameras:
        g = torch.Generator().manual_seed(n)
        pool = [torch.rand((n, K, C), generator=g).to(DEV) for _ in range(4)]
        cams = tuple(range(n))
        live = LiveScorer(scorer, n, window=W, ncrops=K, channels=C, device=DEV)
        state = {"win": torch.zeros((n, K, W, C + 1), device=DEV), "i": 0, "a": None, "b": None}
        pl = PaddedLens([W] * n, K, W, DEV)

        def feats():
            state["i"] += 1
            return pool[state["i"] % len(pool)]

        def step_a(f=None):
            live.push(cams, feats() if f is None else f)
            state["a"] = live.score(cams).scores

        def move_windows(f):
            state["win"] = torch.cat([state["win"][:, :, 1:], mil_ops.add_magnitude_np(f).unsqueeze(2)], dim=2)

        def step_b(f=None):
            move_windows(feats() if f is None else f)
            state["b"] = scorer.score_padded(state["win"], pl)

        def step_c():
            move_windows(feats())
            for v in range(n):
                scorer(video=state["win"][v:v + 1]).scores

        # the same clips to (a) and (b) until every window is full and has wrapped: the same bits
        for t in range(W + 3):
            f = pool[t % len(pool)] * (1.0 + 0.01 * t)
            live.push(cams, f)
            move_windows(f)
        step_a(pool[0])
        step_b(pool[0])
        equal = bool(torch.equal(state["a"], state["b"]))
        if not equal:
            raise SystemExit(f"time_live: (a) and (b) disagree at {n} cameras")
        runs, turns = alternate({A: (step_a, 20), B: (step_b, 20), PER_CAM: (step_c, max(1, 32 // n))}, args.rounds)

        # the three new launches alone
        ids = torch.arange(n, dtype=torch.int32, device=DEV)
        dst = torch.empty((n, K, W, C + 1), device=DEV)
        rows = torch.rand((n * K, W, 1), device=DEV)
        lens = torch.full((n,), W, dtype=torch.int32, device=DEV)
        launches, _ = alternate({"ring_push (two launches)": (lambda: mil_ops.ring_push(pool[0], ids, live.ring, live.counts), 20),
                              "ring_windows": (lambda: mil_ops.ring_windows(live.ring, live.counts, ids, dst), 20),
                              "crop_mean_last": (lambda: mil_ops.crop_mean_last(rows, lens, ids, live.latest, K), 20)}, args.rounds)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        rec["cameras"][str(n)] = {
            "ms_per_step": {k: median_range(v) for k, v in runs.items()}, "ms_per_step_runs": runs, "leg_order": turns,
            "launches_ms": {k: median_range(v) for k, v in launches.items()},
            "ring_windows_bytes_moved": 2 * n * K * W * (C + 1) * 4,
            "a_over_b": round(med[A] / med[B], 4), "a_over_c": round(med[A] / med[PER_CAM], 4),
            "every_round_of_a_below_every_round_of_b": max(runs[A]) < min(runs[B]),
            "a_and_b_same_bits": equal, "state_bytes": int(live.ring.numel() * 4 * 2)}
        print(json.dumps({n: rec["cameras"][str(n)]["ms_per_step"], "launches": rec["cameras"][str(n)]["launches_ms"]}), flush=True)
        del live, state, dst, pool
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
