#!/usr/bin/env python3
"""What a training step costs INSIDE Trainer.fit, input path included; one JSON record -> argv[1] (default
profiles/train_input_run.json).  bench.py's mgfn_train_step times the captured step alone, its input already in the graph's
buffers; this times the loop a user runs.

Corpus: write_synthetic_feature_zips, 64 normal + 64 abnormal train videos at C = 2048 (336 MB of features), batch_size 16 (a step
reads 2 x 16 videos: 83.9 MB with the magnitude channel), 4 steps per epoch.  Five configurations of the same fit:
  (a) the host loaders, num_workers=0     (b) the host loaders, num_workers=8     (c) data.resident=true
  (d) (c) with data.shuffle=true: one advhip_gather_batch_f32 launch per step into the graph's buffers
  (e) (d)'s order served by four torch.index_select(..., out=) launches per step instead (the formulation the kernel replaces)
Each fit runs `--epochs` epochs without validation; a callback records a HIP event after every step.  Steps up to `--skip` (the
eager steps, the capture, the first replays) are left out; over the rest (>= 20 steps):
  ms_per_step              median interval between two consecutive steps' events (the steady step; an epoch's first step, where
                           the loaders are started again, is an outlier the median leaves out)
  ms_per_step_with_starts  (last event - first event) / steps: the epoch starts included, at this corpus' 4 steps per epoch
The five are alternated, `--rounds` rounds in one process; medians over rounds and every configuration's own spread are kept.
(d) and (e) are judged against (c) of the same run, give or take (c)'s own spread (max - min over the rounds): `shuffle` in the record.
Also: the one-time resident load (seconds, both zips, synchronised), the replay alone (the captured step called back to back
on the buffers as they are), for scale, and the gather alone (`gather_alone`: the launch called back to back at the step's shape on
stores of this corpus' size, against the four index_select launches on the same rows).

    python tools/time_train_input.py [out.json] [--rounds 5] [--epochs 8] [--skip 8] [--label TEXT]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from anomaly_detection_on_video_amd.config import _locate, compose, instantiate
from anomaly_detection_on_video_amd import mil_ops
from anomaly_detection_on_video_amd.dataset import StoreRows, epoch_order, write_synthetic_feature_zips
from anomaly_detection_on_video_amd.runner import Trainer

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "train_input_run.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--epochs", type=int, default=8)
ap.add_argument("--skip", type=int, default=8)
ap.add_argument("--videos", type=int, default=64, help="train videos per class")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--label", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_train_input: no GPU visible (the numbers are device times)")
steps_per_epoch = args.videos // args.batch
if steps_per_epoch * args.epochs - args.skip < 20:
    raise SystemExit("time_train_input: fewer than 20 timed steps; raise --epochs")


class StepClock:
    """A HIP event on the current stream after every step (Trainer calls on_step once per step at log_every_n_steps=1)."""

    def __init__(self):
        self.events = []

    def on_step(self, trainer, optimizer):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.events.append(ev)
        return {}


REAL_FEED = Trainer._feed_graph_inputs


def feed_index_select(graphed, batch):
    """Trainer._feed_graph_inputs for leg (e): the StoreRows pair through torch.index_select into the graph's buffers."""
    static = graphed.inputs()
    if static is None or not all(isinstance(b, StoreRows) for b in batch):
        return REAL_FEED(graphed, batch)
    video, s_al, s_nl = static
    n, a = batch
    b = n.rows.shape[0]
    torch.index_select(n.dataset.features, 0, n.rows, out=video[:b])
    torch.index_select(a.dataset.features, 0, a.rows, out=video[b:])
    torch.index_select(n.dataset.anomaly, 0, n.rows, out=s_nl)
    torch.index_select(a.dataset.anomaly, 0, a.rows, out=s_al)
    return True


def fit(data_dir, overrides, feed=None):
    cfg = compose(os.path.join(ROOT, "configs"), "default", ["data=synthetic", f"data.local_path={data_dir}", f"data.batch_size={args.batch}"] + overrides)
    torch.manual_seed(0)
    model = _locate(cfg.runner.model_class)(instantiate(cfg.runner.model_config))
    runner = _locate(cfg.runner.cls)(model=model, optimizer=cfg.runner.optimizer, data=cfg.data)
    setup, load = runner.setup, {}

    def timed_setup(stage="fit"):
        torch.cuda.synchronize()
        t = time.perf_counter()
        setup(stage)
        torch.cuda.synchronize()
        load["s"] = time.perf_counter() - t

    runner.setup = timed_setup
    clock = StepClock()
    trainer = Trainer(max_epochs=args.epochs, check_val_every_n_epoch=10**9, log_every_n_steps=1, callbacks=[clock])
    Trainer._feed_graph_inputs = staticmethod(feed or REAL_FEED)
    try:
        trainer.fit(model=runner)
    finally:
        Trainer._feed_graph_inputs = staticmethod(REAL_FEED)
    torch.cuda.synchronize()
    ev = clock.events[args.skip:]
    gaps = [ev[i].elapsed_time(ev[i + 1]) for i in range(len(ev) - 1)]
    out = {"ms_per_step": float(np.median(gaps)), "ms_per_step_with_starts": ev[0].elapsed_time(ev[-1]) / len(gaps), "steps": len(gaps),
           "setup_s": load["s"], "graph_captures": trainer.graphed_step.captures if trainer.graphed_step is not None else 0}
    g = trainer.graphed_step
    if g is not None and g.inputs() is not None:
        for _ in range(3):
            g(*g.inputs())
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            g(*g.inputs())
        b.record()
        torch.cuda.synchronize()
        out["replay_alone_ms"] = a.elapsed_time(b) / 20
    return out


def gather_alone(videos, batch, calls=40):
    """The gather launch alone, back to back, at the step's shape: two (videos, 10, 32, 2049) stores, `batch` shuffled rows of each per
    call (another window of the order every call), against the four index_select launches on the same rows.  The stores together
    (336 MB at 64 videos) exceed the 256 MB Infinity Cache, but a back-to-back loop still finds part of them there: a lower bound of
    what the launch costs between two training steps."""
    shape = (videos, 10, 32, 2049)
    stores = [torch.randn(shape, device="cuda") for _ in range(2)]
    labels = [torch.zeros(videos, device="cuda"), torch.ones(videos, device="cuda")]
    orders = [torch.from_numpy(epoch_order(videos, 0, s, 0)).cuda() for s in (0, 1)]
    video = torch.empty((2 * batch,) + shape[1:], device="cuda")
    dl = [torch.empty(batch, device="cuda") for _ in range(2)]
    windows = videos // batch

    def rows(i):
        lo = (i % windows) * batch
        return orders[0][lo:lo + batch], orders[1][lo:lo + batch]

    def kernel(i):
        r0, r1 = rows(i)
        mil_ops.gather_batch(stores[0], r0, stores[1], r1, video, labels0=labels[0], labels1=labels[1], dst_labels0=dl[0], dst_labels1=dl[1])

    def index_select(i):
        r0, r1 = rows(i)
        torch.index_select(stores[0], 0, r0, out=video[:batch])
        torch.index_select(stores[1], 0, r1, out=video[batch:])
        torch.index_select(labels[0], 0, r0, out=dl[0])
        torch.index_select(labels[1], 0, r1, out=dl[1])

    out = {"calls": calls, "bytes_read_plus_written": 2 * video.numel() * 4}
    for name, fn in (("kernel", kernel), ("index_select_x4", index_select)):
        for i in range(5):
            fn(i)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(calls):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / calls
        out[name] = {"us": round(us, 2), "TB_per_s": round(out["bytes_read_plus_written"] / (us * 1e-6) / 1e12, 3)}
    r0, r1 = rows(1)
    kernel(1)
    out["kernel_equals_torch_indexing"] = bool(torch.equal(video.view(torch.int32), torch.cat((stores[0][r0], stores[1][r1])).view(torch.int32)))
    return out


SHUFFLED = ["data.resident=true", "data.shuffle=true", "data.seed=1"]
CONFIGS = {"loader, num_workers=0": ["data.num_workers=0"], "loader, num_workers=8": ["data.num_workers=8"], "resident": ["data.resident=true"],
           "resident, shuffled": SHUFFLED, "resident, shuffled, index_select": SHUFFLED}
FEEDS = {"resident, shuffled, index_select": feed_index_select}
rec = {"tool": "tools/time_train_input.py", "label": args.label, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
       "corpus": {"train_videos_per_class": args.videos, "channels": 2048, "batch_size": args.batch, "steps_per_epoch": steps_per_epoch,
                  "epochs": args.epochs, "skipped_steps": args.skip}, "runs": {k: [] for k in CONFIGS}}
with tempfile.TemporaryDirectory() as tmp:
    t = time.perf_counter()
    data_dir = write_synthetic_feature_zips(tmp, n_normal=args.videos, n_abnormal=args.videos, n_test=2)
    print(f"corpus written in {time.perf_counter() - t:.1f} s", flush=True)
    for rnd in range(args.rounds):
        for name, ov in CONFIGS.items():
            r = fit(data_dir, ov, FEEDS.get(name))
            rec["runs"][name].append(r)
            print(rnd, name, json.dumps(r), flush=True)

summary = {}
for name, runs in rec["runs"].items():
    summary[name] = {}
    for key in ("ms_per_step", "ms_per_step_with_starts", "replay_alone_ms", "setup_s"):
        v = [r[key] for r in runs if key in r]
        summary[name][key] = {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
rec["summary"] = summary
res = summary["resident"]["ms_per_step"]["median"]
rec["ratios"] = {f"resident / {k}": round(res / summary[k]["ms_per_step"]["median"], 4) for k in CONFIGS if k != "resident"}
spread = round(summary["resident"]["ms_per_step"]["max"] - summary["resident"]["ms_per_step"]["min"], 3)
shuf, isel = (summary[k]["ms_per_step"]["median"] for k in ("resident, shuffled", "resident, shuffled, index_select"))
rec["shuffle"] = {"resident_ms": res, "resident_spread_ms": spread, "shuffled_ms": shuf, "index_select_ms": isel,
                  "shuffled_minus_resident_ms": round(shuf - res, 3), "shuffled_minus_index_select_ms": round(shuf - isel, 3),
                  "shuffled_costs_no_more_than_resident": bool(shuf <= res + spread),
                  "kernel_not_slower_than_index_select": bool(shuf <= isel + spread)}
rec["gather_alone"] = gather_alone(args.videos, args.batch)
print(json.dumps({"shuffle": rec["shuffle"], "gather_alone": rec["gather_alone"]}), flush=True)
rec["ratios"]["resident / replay alone"] = round(res / summary["resident"]["replay_alone_ms"]["median"], 4)
rec["resident_load_s"] = summary["resident"]["setup_s"]
print(json.dumps({"summary": summary, "ratios": rec["ratios"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
