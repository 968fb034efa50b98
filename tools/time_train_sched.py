#!/usr/bin/env python3
"""What a per-step learning-rate schedule and a gradient-norm clip cost the captured training step; one JSON record -> argv[1]
(default profiles/train_sched.json).

One process, the scorer at the runner's batch shape (32, 10, 32, 2049), the batch already in the step's input buffers (as
bench.py's mgfn_train_step).  Five legs, each its own model + optimizer + train_graph.GraphedTrainStep, all warmed first:
  (a) constant lr, default HipAdam: the replay as it was before these options existed (the yardstick)
  (b) HipAdam(device_lr=True), the lr set from optim.lr_at (cosine) before every step: still one graph
  (c) (b) plus max_grad_norm: the norm reduction and the scale-on-read Adam launch inside the graph
  (d) default HipAdam with GraphedTrainStep(clip_grad_norm=): torch.nn.utils.clip_grad_norm_'s launches inside the graph
  (e) default HipAdam with the lr changed before every step: re-captured four times, then eager for good
A round times `--steps` consecutive steps of every leg between two HIP events, the legs alternated; `--rounds` rounds; medians
and min-max per leg.  (b)-(e) are judged against (a) of the same run, give or take (a)'s own spread.  Also `norm_alone`: the
norm op (its launches back to back, nothing else: issued from Python, and as a captured graph of their own) over the scorer's gradient set.

    python tools/time_train_sched.py [out.json] [--rounds 5] [--steps 30] [--label TEXT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
from anomaly_detection_on_video_amd.optim import HipAdam, lr_at
from anomaly_detection_on_video_amd.train_graph import GraphedTrainStep
from anomaly_detection_on_video_amd.weights import synth_module_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "train_sched.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--batch", type=int, default=16, help="videos per class (the step sees 2 x batch)")
ap.add_argument("--clip", type=float, default=1.0)
ap.add_argument("--label", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_train_sched: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
SPEC = {"name": "cosine", "warmup_steps": 10, "total_steps": 10 + (args.rounds + 2) * args.steps, "min_lr_ratio": 0.01}
BASE_LR = 1e-3

gen = torch.Generator(device=dev).manual_seed(0)
vb = torch.rand(2 * args.batch, 10, 32, 2048, device=dev, generator=gen) * 3
vb = torch.cat([vb, vb.norm(dim=3, keepdim=True)], dim=3)
al, nl = torch.ones(args.batch, device=dev), torch.zeros(args.batch, device=dev)


class Leg:
    def __init__(self, name, adam=None, clip_grad_norm=None, scheduled=False):
        self.name, self.scheduled, self.taken = name, scheduled, 0
        self.model = MGFNForVideoAnomalyDetection(MGFNConfig())
        self.model.load_state_dict(synth_module_state_dict(self.model))
        self.model = self.model.to(dev).train()
        self.opt = HipAdam(self.model.parameters(), lr=BASE_LR, weight_decay=5e-4, **(adam or {}))
        self.step = GraphedTrainStep(self.model, self.opt, eager_steps=3, clip_grad_norm=clip_grad_norm)

    def run(self, n):
        for _ in range(n):
            if self.scheduled:
                lr = lr_at(SPEC, BASE_LR, self.taken)
                for g in self.opt.param_groups:
                    g["lr"] = lr
            self.step(*(self.step.inputs() or (vb, al, nl)))
            self.taken += 1

    def timed(self, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self.run(n)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n


legs = [Leg("a: constant lr, replay"),
        Leg("b: device_lr, cosine per step", adam={"device_lr": True}, scheduled=True),
        Leg("c: device_lr + max_grad_norm", adam={"device_lr": True, "max_grad_norm": args.clip}, scheduled=True),
        Leg("d: torch clip_grad_norm_ in the graph", clip_grad_norm=args.clip),
        Leg("e: by-value lr changed per step", scheduled=True)]
for leg in legs:
    leg.run(14)  # eager steps, the capture(s), first replays; leg (e) uses up its four captures and settles on the eager loop
    torch.cuda.synchronize()
    print(leg.name, "captures", leg.step.captures, "graph" if leg.step.graph is not None else "eager", flush=True)

rec = {"tool": "tools/time_train_sched.py", "label": args.label, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
       "steps_per_round": args.steps, "batch_shape": list(vb.shape), "schedule": SPEC, "max_grad_norm": args.clip, "ms_per_step": {leg.name: [] for leg in legs}}
for rnd in range(args.rounds):
    for leg in legs:
        ms = leg.timed(args.steps)
        rec["ms_per_step"][leg.name].append(round(ms, 4))
        print(rnd, leg.name, round(ms, 4), flush=True)
rec["legs"] = {}
for leg in legs:
    v = rec["ms_per_step"][leg.name]
    rec["legs"][leg.name] = {"median_ms": round(float(np.median(v)), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                             "captures": leg.step.captures, "mode": "graph replay" if leg.step.graph is not None else "eager",
                             "replays": leg.step.replays}
a = rec["legs"][legs[0].name]
spread = round(a["max_ms"] - a["min_ms"], 3)
med = [rec["legs"][leg.name]["median_ms"] for leg in legs]
rec["verdict"] = {"a_median_ms": med[0], "a_spread_ms": spread,
                  "b_minus_a_ms": round(med[1] - med[0], 3), "b_within_a_spread": bool(abs(med[1] - med[0]) <= spread),
                  "c_minus_a_ms": round(med[2] - med[0], 3), "c_minus_d_ms": round(med[2] - med[3], 3), "c_below_d": bool(med[2] < med[3]),
                  "e_over_a": round(med[4] / med[0], 3)}
rec["grad_norm_last"] = {"c": float(legs[2].opt.grad_norm)}

# the norm op alone: its launches back to back over the gradients leg (c)'s graph left in place
opt = legs[2].opt
grads = [p.grad for p in legs[2].model.parameters() if p.grad is not None]
lib_calls = 200
from anomaly_detection_on_video_amd import _lib

for _ in range(10):
    opt._launch_grad_norm(_lib.load(), grads, False)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(lib_calls):
    opt._launch_grad_norm(_lib.load(), grads, False)
e1.record()
torch.cuda.synchronize()
elements = sum(g.numel() for g in grads)
us = e0.elapsed_time(e1) * 1e3 / lib_calls
# ... and the same launches as a captured graph of their own, replayed back to back: no Python between them
side = torch.cuda.Stream()
norm_graph = torch.cuda.CUDAGraph()
torch.cuda.synchronize()
with torch.cuda.graph(norm_graph, stream=side):
    opt._launch_grad_norm(_lib.load(), grads, True)
for _ in range(10):
    norm_graph.replay()
e0.record()
for _ in range(lib_calls):
    norm_graph.replay()
e1.record()
torch.cuda.synchronize()
us_graph = e0.elapsed_time(e1) * 1e3 / lib_calls
rec["norm_alone"] = {"calls": lib_calls, "tensors": len(grads), "elements": elements, "launches_per_call": -(-len(grads) // 240) + 1,
                     "partial_sums": sum((g.numel() + 4095) // 4096 for g in grads), "us_per_call": round(us, 2),
                     "us_per_graph_replay": round(us_graph, 2), "GB_per_s_read_graph_replay": round(elements * 4 / (us_graph * 1e-6) / 1e9, 1),
                     "note": "us_per_call: issued from Python back to back (host-bound: the item table is built per call); us_per_graph_replay: the same "
                             "launches captured alone and replayed back to back.  The gradients (115 MB) fit the Infinity Cache in such a loop"}
print(json.dumps({"legs": rec["legs"], "verdict": rec["verdict"], "norm_alone": rec["norm_alone"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
