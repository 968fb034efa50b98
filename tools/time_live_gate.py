#!/usr/bin/env python3
"""What the live frames' motion gate costs and saves (anomaly_detection_on_video_amd/live.py: MotionGate, LiveFrames(motion=),
LiveScorer.hold), after tools/time_live_frames.py's protocol; one JSON record -> argv[1] (default profiles/live_gate.json).

N = 16 / 64 / 256 cameras, frames 256 x 340 already at ring size on the device, frames_per_clip 16, clip_stride 16, crops
"center", a scorer window of 32 clips (full from the start: the feature rings are pre-filled).  Every camera delivers one frame
per step; every 16 steps every camera has a clip due.  Four legs do the same steps through LiveScorer.step_camera_frames:

  (a) no gate: the yardstick, from the same run;
  (b) the gate, every camera moving (random frames): what the gate costs when it saves nothing -- the update launches on every
      step and the one read-back on the due step;
  (c) the gate, half of the cameras still;
  (d) the gate, nine tenths of the cameras still.

A still camera shows one fixed frame plus one-sided noise in [0, pixel_delta]; a moving camera shows the random frames of (a), the
same in every leg.  The gate's numbers (pixel_delta 6, max_changed 0.001) are this tool's, chosen for its synthetic frames: nobody
has measured what suits a real camera.  The unit is one CYCLE of 16 steps in ms.  One process; per N the legs are run alternately
(their order rotates from round to round), `--rounds` rounds after a warm-up round, each timing `--cycles` cycles between two HIP
events (the last one synchronised); medians and min-max over the rounds; `leg_order` keeps which leg ran behind which.  Before
timing, every leg is fed its frames for three cycles and the moving cameras are compared with (a): in (b), which extracts as many
clips per launch as (a), their score bits must equal (a)'s.  In (c) and (d) the backbone runs on fewer clips per launch, and its
bits follow its batch (the tuned plan picks tiles and K slices by it), so there the moving cameras' newest features must equal,
bit for bit, the backbone on (a)'s windows of the same cameras in a launch of the leg's own shape; whether their scores equal
(a)'s, and by how much they differ, is recorded.
(b) - (a) is reported against (a)'s own min-max spread; a gain of (c) / (d) is claimed only where every round lies below every
round of (a).  Also the gate's update alone at each N -- all cameras still (two frames read per camera) and all moving (the frame
read twice, the anchor read and written) -- and ring_repeat alone, in microseconds and bytes (read + written, counted from the
shapes) per second.  Backbone and scorer at synthetic weights (the time does not depend on them).

    python tools/time_live_gate.py [out.json] [--rounds 5] [--cameras 16 64 256] [--label TEXT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "live_gate.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cycles", type=int, default=2)
ap.add_argument("--cameras", type=int, nargs="+", default=[16, 64, 256])
ap.add_argument("--window", type=int, default=32)
ap.add_argument("--label", default="")
args = ap.parse_args()

import torch

from anomaly_detection_on_video_amd import mil_ops
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.live import LiveFrames, LiveScorer, MotionGate
from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_module_state_dict

if not torch.cuda.is_available():
    raise SystemExit("time_live_gate: no GPU visible")
DEV = torch.device("cuda", 0)
FH, FW, FPC, STRIDE, C, W = 256, 340, 16, 16, 2048, args.window
FRAME = FH * FW * 3
GATE = MotionGate(pixel_delta=6, max_changed=0.001)
POOL = 4


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

LEGS = {"(a) no gate": None, "(b) gate, every camera moving": 0.0, "(c) gate, half of the cameras still": 0.5,
        "(d) gate, nine tenths of the cameras still": 0.9}
A = "(a) no gate"
rec = {"tool": "tools/time_live_gate.py", "label": args.label, "rounds": args.rounds, "cycles_per_round": args.cycles, "frame_hw": [FH, FW],
       "frames_per_clip": FPC, "clip_stride": STRIDE, "crops": "center", "window": W, "device": torch.cuda.get_device_name(0),
       "gate": {"pixel_delta": GATE.pixel_delta, "max_changed": GATE.max_changed, "max_hold": GATE.max_hold, "limit_bytes": GATE.limit(FRAME),
                "note": "this tool's numbers for its synthetic frames, not a recommendation"},
       "unit": "ms per cycle of 16 steps (every camera delivers 16 frames; one clip per camera comes due and is extracted or held, pushed and scored)",
       "cameras": {}}
with torch.no_grad():
    for n in args.cameras:
        g = torch.Generator().manual_seed(n)
        pool = [torch.randint(0, 256, (n, FH, FW, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(POOL)]
        scene = torch.randint(0, 256 - GATE.pixel_delta, (n, FH, FW, 3), generator=g, dtype=torch.uint8).to(DEV)
        noise = [torch.randint(0, GATE.pixel_delta + 1, (n, FH, FW, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(POOL)]
        fill = [torch.rand((n, 1, C), generator=g).to(DEV) for _ in range(W)]
        cams = tuple(range(n))
        entry = rec["cameras"][str(n)] = {}
        legs, state = {}, {}
        for name, share in LEGS.items():
            n_still = 0 if not share else int(round(share * n))
            frames = pool
            if n_still:  # the last n_still cameras are still: a fixed frame plus one-sided noise within pixel_delta
                frames = [p.clone() for p in pool]
                for j in range(POOL):
                    frames[j][n - n_still:] = scene[n - n_still:] + noise[j][n - n_still:]
            lf = LiveFrames(n, frame_hw=(FH, FW), frames_per_clip=FPC, clip_stride=STRIDE, device=DEV, motion=None if share is None else GATE)
            live = LiveScorer(scorer, n, window=W, ncrops=1, channels=C, device=DEV)
            for f in fill:  # full scorer windows from the start: the padded pass has its steady shape
                live.push(cams, f)
            st = state[name] = {"i": 0, "scores": None, "lf": lf, "live": live, "frames": frames, "moving": n - n_still}

            def cycle(st=st):
                for _ in range(STRIDE):
                    st["i"] += 1
                    got = st["live"].step_camera_frames(backbone, st["lf"], cams, st["frames"][st["i"] % POOL], crops="center")
                    if got is not None:
                        st["scores"] = got.scores

            legs[name] = (cycle, args.cycles)
        for _ in range(3):  # the first cycle anchors the still cameras, the second extracts their reference, the third holds
            for name in legs:
                legs[name][0]()
        torch.cuda.synchronize()
        same, diff, same_feats = {}, {}, {}
        for name, st in state.items():
            m = st["moving"]
            same[name] = bool(torch.equal(st["scores"][:m].view(torch.int32), state[A]["scores"][:m].view(torch.int32)))
            diff[name] = float((st["scores"][:m] - state[A]["scores"][:m]).abs().max())
            if st["lf"].motion is None:
                continue
            want = (tuple(range(m)), tuple(range(m, n)))
            if st["lf"].last_decision != want:
                raise SystemExit(f"time_live_gate: {name} at {n} cameras decided {st['lf'].last_decision}, not {m} extracted and {n - m} held")
            # the newest features of the moving cameras against the backbone on (a)'s windows of the same cameras in one launch of
            # the same shape (m clips): the backbone's bits follow its batch (the tuned plan picks tiles and K slices by it)
            ref = backbone.forward_frames(state[A]["lf"].windows(tuple(range(m))), 0, m, frames_per_clip=FPC, crops="center").reshape(m, C)
            slot = (st["live"].counts_host[0] - 1) % W
            same_feats[name] = bool(torch.equal(st["live"].ring[:m, 0, slot, :C].view(torch.int32), ref.view(torch.int32)))
        # where a leg extracts as many clips per launch as (a) does, (b), the scores themselves must be (a)'s
        bad = [k for k, st in state.items() if not same_feats.get(k, True) or (st["moving"] == n and not same[k])]
        if bad:
            raise SystemExit(f"time_live_gate: at {n} cameras the moving cameras of {bad} differ: scores equal (a)'s {same}, features equal the "
                             f"backbone's at the leg's own launch shape {same_feats}")
        runs, turns = alternate(legs, args.rounds)
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread_a = max(runs[A]) - min(runs[A])
        entry["ms_per_cycle"] = {k: median_range(v) for k, v in runs.items()}
        entry["ms_per_cycle_runs"] = runs
        entry["leg_order"] = turns
        entry["a_spread_ms"] = round(spread_a, 4)
        entry["moving_cameras_same_score_bits_as_a"] = same
        entry["moving_cameras_max_abs_score_difference_from_a"] = diff
        entry["moving_cameras_same_feature_bits_as_the_backbone_at_the_legs_launch_shape"] = same_feats
        entry["windows"] = {k: {"extracted": st["lf"].extracted_total, "held": st["lf"].held_total} for k, st in state.items() if st["lf"].motion is not None}
        entry["vs_a"] = {k: {"minus_a_ms": round(med[k] - med[A], 4), "over_a": round(med[k] / med[A], 4),
                             "within_a_spread": bool(abs(med[k] - med[A]) <= spread_a),
                             "every_round_below_every_round_of_a": bool(max(runs[k]) < min(runs[A]))} for k in runs if k != A}
        print(json.dumps({"cameras": n, **entry["ms_per_cycle"]}), flush=True)
        del legs, state, lf, live, st
        torch.cuda.empty_cache()

        # the gate's update alone (three launches) and ring_repeat alone (two launches)
        ids = torch.arange(n, dtype=torch.int32, device=DEV)
        limit = GATE.limit(FRAME)
        anchor = pool[0].clone()
        gstate = torch.tensor([[0, 1, 0, 0]] * n, dtype=torch.int32).to(DEV)
        scratch = torch.zeros((mil_ops.frame_gate_scratch(n, FRAME),), dtype=torch.int32, device=DEV)
        flip = {"i": 0}

        def update_moving():
            flip["i"] ^= 1
            mil_ops.frame_gate_update(pool[1 + flip["i"]], ids, anchor, gstate, scratch, GATE.pixel_delta, limit)

        ring = torch.rand((n, 1, W, C + 1), generator=g).to(DEV)
        counts = torch.full((n,), W + 3, dtype=torch.int64, device=DEV)
        STILL, MOVING, REPEAT = "frame_gate_update, every camera still", "frame_gate_update, every camera moving", "ring_repeat"
        launches, _ = alternate({STILL: (lambda: mil_ops.frame_gate_update(pool[0], ids, anchor, gstate, scratch, GATE.pixel_delta, limit), 20)},
                                args.rounds)
        epoch = int(gstate[0, 1])
        if epoch != 1:
            raise SystemExit(f"time_live_gate: the still launches moved the anchor (epoch {epoch})")
        more, _ = alternate({MOVING: (update_moving, 20), REPEAT: (lambda: mil_ops.ring_repeat(ids, ring, counts), 20)}, args.rounds)
        launches.update(more)
        if int(gstate[0, 1]) != 1 + 20 * (args.rounds + 1):
            raise SystemExit(f"time_live_gate: not every moving launch moved the anchor (epoch {int(gstate[0, 1])})")
        moved = {STILL: 2 * n * FRAME, MOVING: 4 * n * FRAME, REPEAT: 2 * n * (C + 1) * 4}
        entry["launches_us"] = {k: median_range([1e3 * x for x in v]) for k, v in launches.items()}
        entry["launches_us_runs"] = {k: [round(1e3 * x, 3) for x in v] for k, v in launches.items()}
        entry["bytes_moved"] = moved
        entry["tb_per_s"] = {k: {"median": round(moved[k] / (float(np.median(v)) * 1e-3) / 1e12, 3), "min": round(moved[k] / (max(v) * 1e-3) / 1e12, 3),
                                 "max": round(moved[k] / (min(v) * 1e-3) / 1e12, 3)} for k, v in launches.items()}
        print(json.dumps({"cameras": n, "launches_us": entry["launches_us"], "tb_per_s": entry["tb_per_s"]}), flush=True)
        del pool, scene, noise, anchor, ring, scratch
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
