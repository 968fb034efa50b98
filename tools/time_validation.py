#!/usr/bin/env python3
"""What `Trainer.validate` costs with the frame-level AUC on the host (data.device_metrics=false: one device-to-host copy per
video, then numpy's repeat / sort / cumulative sums) and on the device (data.device_metrics=true: the scores stay in a
FrameAucPlan, mil_ops.roc_counts sorts and counts, one synchronisation); one JSON record -> argv[1] (default
profiles/validation_run.json).

Corpus: UCF-Crime's test set in size -- `--videos` (290) test videos of T ~ U[50, 500] clips, 10 crops, C = 2048, every other one
with an annotated event; both runs read it resident (the flag needs data.resident=true, and flag off with resident is the path
without it).  The two runners are validated alternately, `--rounds` rounds after one warm-up each in one process: wall time of
Trainer.validate (its result is a pair of Python floats, so the pass has ended when it returns), medians and ranges; every
round's two results must be equal.  The model is the configured MGFN at its initial weights (the time does not depend on them).

Batched validation (data.val_batch_videos = 8, 16, 32 with device_metrics=true: length-sorted padded buckets, one scoring pass per
bucket) runs as three more legs of the same alternation, on the same resident corpus (all legs read ONE resident copy).  Its
baseline is the device_metrics=true leg of the same run.  Per leg also: buckets, padded / real positions, the plan's input buffer and
the peak of device memory allocated during a pass above what was allocated before it, the two AUC floats and their difference
from the per-video leg's, and the largest per-video relative error (max |a - b| / max |b|) of the scores against that leg's.

Also mil_ops.roc_counts alone (its read-back included: wall time) against metrics._ranked on the expanded frames, on the two
item shapes the plan makes of about 1.1 M frames: 70 000 items of 16 frames each (the default stride) and 1 100 000 items of one
frame each (overlapping windows).

The driver starts no GPU work itself: every step is a child process under its own `timeout`, chained -- the first one that
fails ends the run.

    python tools/time_validation.py [out.json] [--rounds 5] [--videos 290] [--label TEXT]
"""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "validation_run.json"))
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--videos", type=int, default=290)
ap.add_argument("--channels", type=int, default=2048)
ap.add_argument("--label", default="")
ap.add_argument("--step", choices=["corpus", "validate", "counts"], help="(internal) run one step in this process")
ap.add_argument("--dir", help="(internal) the working directory of the steps")
args = ap.parse_args()


BATCH_LEGS = (8, 16, 32)


def median_range(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def write_corpus(outdir):
    """train.zip of write_synthetic_feature_zips (a few videos: setup loads it, validation does not read it) and a test.zip of
    UCF-Crime's size: video i is the first T_i clips of one random (500, 10, C) block, scaled by its own factor (what a video
    holds does not change what the pass costs; drawing 1.6 G normals would only make the tool slow)."""
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips
    from anomaly_detection_on_video_amd.gt import frame_ground_truth

    write_synthetic_feature_zips(outdir, n_normal=2, n_abnormal=2, n_test=1, channels=args.channels)
    rng = np.random.default_rng(0)
    base = np.abs(rng.standard_normal((500, 10, args.channels))).astype(np.float32)
    gt, clips = {}, []
    with zipfile.ZipFile(os.path.join(outdir, "test.zip"), "w") as z:
        for i in range(args.videos):
            t = int(rng.integers(50, 501))
            f = base[:t] * np.float32(1.0 + 0.002 * i)
            if i % 2 == 0:
                name, ev = f"Normal_Videos_{900 + i}_x264", ((-1, -1), (-1, -1))
            else:
                c0 = int(rng.integers(2, t - 8))
                f[c0:c0 + 6] *= 2.5
                name, ev = f"Burglary{i:03d}_x264", ((c0 * 16, (c0 + 6) * 16 - 1), (-1, -1))
            buf = io.BytesIO()
            np.save(buf, f)
            z.writestr(f"test/{name}_i3d.npy", buf.getvalue())
            gt[name] = frame_ground_truth(t, ev[0], ev[1])
            clips.append(t)
    with open(os.path.join(outdir, "ground_truth.json"), "w") as f:
        json.dump(gt, f)
    return {"test_videos": args.videos, "clips": int(sum(clips)), "frames": int(sum(clips)) * 16, "clips_per_video": [min(clips), max(clips)],
            "channels": args.channels, "crops": 10}


def step_validate(workdir):
    import torch

    from anomaly_detection_on_video_amd.config import _locate, compose, instantiate
    from anomaly_detection_on_video_amd.runner import Trainer

    if not torch.cuda.is_available():
        raise SystemExit("time_validation: no GPU visible")

    loaded = []

    def runner_for(flag, batch_videos=1):
        cfg = compose(os.path.join(ROOT, "configs"), "default", ["data=synthetic", f"data.local_path={workdir}", "data.batch_size=2",
                                                                 "data.resident=true", f"data.device_metrics={flag}",
                                                                 f"data.val_batch_videos={batch_videos}"])
        torch.manual_seed(0)
        model = _locate(cfg.runner.model_class)(instantiate(cfg.runner.model_config))
        runner = _locate(cfg.runner.cls)(model=model, optimizer=cfg.runner.optimizer, data=cfg.data)
        trainer = Trainer(max_epochs=1)
        runner.to(trainer.device)
        if not loaded:
            runner.setup("fit")
            loaded.append(runner)
        else:  # the same resident corpus for every leg: what setup does after loading
            runner.train_dataset, runner.valid_dataset = loaded[0].train_dataset, loaded[0].valid_dataset
            runner.build_validation_plans()
        return trainer, runner

    HOST, DEVICE = "host metrics (device_metrics=false)", "device metrics (device_metrics=true)"
    sides = {HOST: runner_for("false"), DEVICE: runner_for("true")}
    batched = {f"batched, val_batch_videos={k} (device_metrics=true)": k for k in BATCH_LEGS}
    sides.update({name: runner_for("true", k) for name, k in batched.items()})
    runs = {k: [] for k in sides}
    peak = {k: 0 for k in sides}
    results, got = [], {}
    for rnd in range(-1, args.rounds):  # round -1: the warm-up
        got = {}
        for name, (trainer, runner) in sides.items():
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t = time.perf_counter()
            got[name] = trainer.validate(runner)
            ms = (time.perf_counter() - t) * 1e3
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - before)
            if rnd >= 0:
                runs[name].append(ms)
            print(rnd, name, f"{ms:.2f} ms", json.dumps(got[name]), flush=True)
        if got[HOST] != got[DEVICE]:
            raise SystemExit(f"time_validation: the two per-video paths disagree: {got[HOST]} vs {got[DEVICE]}")
        results.append(got[HOST])
    # the batched legs against the per-video leg of the same process: scores video by video, the two AUCs
    base_runner = sides[DEVICE][1]
    base = base_runner.auc_plan.scores.double().cpu().numpy()
    offs = base_runner.auc_plan.items.window_offsets
    legs = {}
    for name, k in batched.items():
        runner = sides[name][1]
        sc = runner.auc_plan.scores.double().cpu().numpy()
        errs = [float(np.abs(sc[int(offs[i]):int(offs[i + 1])] - base[int(offs[i]):int(offs[i + 1])]).max() / np.abs(base[int(offs[i]):int(offs[i + 1])]).max())
                for i in range(len(offs) - 1)]
        plan = runner.score_plan
        legs[name] = {"val_batch_videos": k, "buckets": len(plan.buckets), "padded_over_real_positions": round(plan.padding_ratio, 4),
                      "plan_input_buffer_bytes": plan.buffer_bytes, "peak_bytes_allocated_during_a_pass": int(peak[name]),
                      "metrics": got[name], "metrics_minus_per_video": {m: got[name][m] - got[DEVICE][m] for m in got[name]},
                      "max_per_video_rel_err_vs_per_video": max(errs),
                      "every_round_below_every_per_video_round": max(runs[name]) < min(runs[DEVICE])}
    return {"ms_per_validate": {k: median_range(v) for k, v in runs.items()}, "ms_per_validate_runs": runs, "metrics": results[-1],
            "peak_bytes_allocated_during_a_pass": {k: int(v) for k, v in peak.items()}, "batched": legs, "device": torch.cuda.get_device_name(0)}


def step_counts():
    import torch

    from anomaly_detection_on_video_amd import metrics, mil_ops

    out = {}
    rng = np.random.default_rng(1)
    for m, w in ((70_000, 16), (1_100_000, 1)):
        scores = rng.random(m).astype(np.float32)
        pos = rng.integers(0, w + 1, m).astype(np.int32)
        neg = (w - pos).astype(np.int32)
        labels = (np.arange(w)[None, :] < pos[:, None]).ravel().astype(np.float32)
        preds = np.repeat(scores, w)
        dev = [torch.from_numpy(x).cuda() for x in (scores, pos, neg)]
        ws = mil_ops.roc_counts_workspace(m, dev[0].device)
        d_ms, h_ms = [], []
        for rnd in range(-1, args.rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            thr, tps, fps = mil_ops.roc_counts(*dev, workspace=ws)
            d = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            want = metrics._ranked(labels, preds)
            h = (time.perf_counter() - t) * 1e3
            if rnd >= 0:
                d_ms.append(d)
                h_ms.append(h)
        if not (np.array_equal(tps.cpu().numpy(), want[0]) and np.array_equal(fps.cpu().numpy(), want[1])):
            raise SystemExit(f"time_validation: roc_counts differs from _ranked at M = {m}")
        out[f"M={m}, {w} frames per item"] = {"frames": int(preds.size), "groups": int(tps.numel()), "roc_counts_ms": median_range(d_ms),
                                              "host_ranked_ms": median_range(h_ms)}
        print(json.dumps(out), flush=True)
    return out


if args.step:
    path = os.path.join(args.dir, args.step + ".json")
    rec = write_corpus(args.dir) if args.step == "corpus" else step_validate(args.dir) if args.step == "validate" else step_counts()
    with open(path, "w") as f:
        json.dump(rec, f)
    sys.exit(0)

rec = {"tool": "tools/time_validation.py", "label": args.label, "rounds": args.rounds}
with tempfile.TemporaryDirectory() as tmp:
    for step, limit in (("corpus", 600), ("validate", 600), ("counts", 180)):  # seconds; the first failure ends the run
        t = time.perf_counter()
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", tmp,
               "--rounds", str(args.rounds), "--videos", str(args.videos), "--channels", str(args.channels)]
        rc = subprocess.run(cmd).returncode
        print(f"step {step}: exit {rc} after {time.perf_counter() - t:.1f} s", flush=True)
        if rc != 0:
            raise SystemExit(f"time_validation: step {step} ended with {rc}; nothing further is started")
        with open(os.path.join(tmp, step + ".json")) as f:
            rec[step] = json.load(f)
v = rec["validate"]["ms_per_validate"]
off, on = (v[k]["median"] for k in list(v)[:2])  # the two per-video legs: metrics on the host, on the device
rec["device"] = rec["validate"].pop("device")
rec["ratio_device_over_host_metrics"] = round(on / off, 4)
rec["ratio_batched_over_per_video_device_metrics"] = {k: round(v[k]["median"] / on, 4) for k in list(v)[2:]}
print(json.dumps({"ms_per_validate": v, "ratio": rec["ratio_device_over_host_metrics"], "batched_ratio": rec["ratio_batched_over_per_video_device_metrics"],
                  "batched": rec["validate"]["batched"], "counts": rec["counts"]}), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
