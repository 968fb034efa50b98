#!/usr/bin/env python3
"""What live events add to one live-scoring step (LiveScorer(events=), anomaly_detection_on_video_amd/events.py:
LiveEventTracker); one JSON record -> argv[1] (default profiles/live_events.json).

N = 16 / 64 / 256 cameras, W = 32 clips, 10 crops, C = 2048, every window full (the steady state).  Four legs do the same step,
every camera pushes one clip and all N windows are re-scored (LiveScorer.push + LiveScorer.score):

  (none)       LiveScorer without events: the yardstick;
  (smooth=S)   LiveScorer(events=EventSpec(smooth=S, ...)) for S = 1, 9 and 255: the same step plus one live_events_update launch.

One process; per N the legs are run alternately (their order rotates from round to round), `--rounds` rounds after a warm-up
round, each round timing `iters` steps between two HIP events (the last one synchronised); medians and min-max over the rounds,
in ms per step; `leg_order` keeps which leg ran behind which.  Before timing, all legs are fed the same clips and must give the
same score bits.  Also, timed the same way at each N: the update launch alone (mil_ops.live_events_update on N cameras, per
smooth) and two LiveEventTracker.drain() calls eight steps apart (host wall time, a drain synchronises; the first one of a process
also pays torch's one-time costs).  The thresholds are the quartiles of the scores the warm-up saw, so that candidates open and
close.  The scorer is the default MGFN at synthetic weights.

    python tools/time_live_events.py [out.json] [--rounds 5] [--cameras 16 64 256] [--label TEXT]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "live_events.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cameras", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--smooth", type=int, nargs="+", default=[1, 9, 255])
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--crops", type=int, default=10)
ap.add_argument("--channels", type=int, default=2048)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch

from anomaly_detection_on_video_amd import mil_ops
from anomaly_detection_on_video_amd.events import EventSpec
from anomaly_detection_on_video_amd.live import LiveScorer
from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
from anomaly_detection_on_video_amd.weights import synth_module_state_dict

if not torch.cuda.is_available():
    raise SystemExit("time_live_events: no GPU visible")
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

NONE = "(none) LiveScorer push + score"
rec = {"tool": "tools/time_live_events.py", "label": args.label, "rounds": args.rounds, "window": W, "crops": K, "channels": C,
       "device": torch.cuda.get_device_name(0), "unit": "ms per step (every camera pushes one clip, every window is scored)",
       "yardstick": NONE, "cameras": {}}
with torch.no_grad():
    for n in args.cameras:
        g = torch.Generator().manual_seed(n)
        pool = [torch.rand((n, K, C), generator=g).to(DEV) * (1.0 + 0.5 * i) for i in range(4)]
        cams = tuple(range(n))
        state = {"i": 0}

        def feats():
            state["i"] += 1
            return pool[state["i"] % len(pool)]

        # the thresholds: quartiles of the scores of a warm-up without events
        probe = LiveScorer(scorer, n, window=W, ncrops=K, channels=C, device=DEV)
        seen = []
        for t in range(W + 3):
            probe.push(cams, pool[t % len(pool)])
            seen.append(probe.score(cams).latest.cpu().numpy())
        low, high = (float(q) for q in np.quantile(np.concatenate(seen), [0.5, 0.75]))
        del probe
        lives = {NONE: LiveScorer(scorer, n, window=W, ncrops=K, channels=C, device=DEV)}
        for s in args.smooth:
            lives[f"(smooth={s}) LiveScorer(events=) push + score"] = LiveScorer(scorer, n, window=W, ncrops=K, channels=C, device=DEV,
                                                                                events=EventSpec(low, high, s, 2, 2))
        last = {}

        def make_step(name):
            live = lives[name]

            def step(f=None):
                live.push(cams, feats() if f is None else f)
                last[name] = live.score(cams).scores
            return step

        steps = {name: make_step(name) for name in lives}
        for t in range(W + 3):  # the same clips to every leg until every window is full and has wrapped: the same bits
            for name in steps:
                steps[name](pool[t % len(pool)])
        equal = all(bool(torch.equal(last[name], last[NONE])) for name in steps)
        if not equal:
            raise SystemExit(f"time_live_events: the legs disagree at {n} cameras")
        runs, turns = alternate({name: (step, args.iters) for name, step in steps.items()}, args.rounds)

        # the update launch alone, and two drains
        ids = torch.arange(n, dtype=torch.int32, device=DEV)
        sc = torch.rand((n,), device=DEV)
        alone = {}
        for s in args.smooth:
            st = mil_ops.live_events_state(n, s, 64, DEV)
            alone[f"live_events_update smooth={s}"] = ((lambda st=st, s=s: mil_ops.live_events_update(sc, ids, st, low, high, s, 2, 2)), 50)
        launches, _ = alternate(alone, args.rounds)
        drains, emitted = {}, {}
        for name, live in lives.items():
            if live.events is None:
                continue
            for which in ("first", "second"):  # (the first drain of a process also pays torch's one-time costs of the gather)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = live.events.drain()
                torch.cuda.synchronize()
                drains.setdefault(name, {})[which] = round((time.perf_counter() - t0) * 1e3, 4)
                emitted.setdefault(name, {})[which] = {"events": len(d.events), "lost": int(d.lost.sum())}
                for _ in range(8):
                    steps[name]()
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = max(runs[NONE]) - min(runs[NONE])
        rec["cameras"][str(n)] = {
            "ms_per_step": {k: median_range(v) for k, v in runs.items()}, "ms_per_step_runs": runs, "leg_order": turns,
            "thresholds": {"low": low, "high": high},
            "added_ms_vs_none": {k: round(med[k] - med[NONE], 4) for k in runs if k != NONE},
            "none_spread_ms": round(spread, 4),
            "added_inside_none_spread": {k: bool(abs(med[k] - med[NONE]) <= spread) for k in runs if k != NONE},
            "launch_ms": {k: median_range(v) for k, v in launches.items()},
            "drain_ms_host_wall": drains, "drained": emitted, "legs_same_bits": equal}
        print(json.dumps({n: rec["cameras"][str(n)]["ms_per_step"], "launch": rec["cameras"][str(n)]["launch_ms"], "drain": drains}), flush=True)
        del lives, steps, pool
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
