#!/usr/bin/env python3
"""Decoder surfaces (surface=) against the compact 8-bit call; one JSON record -> argv[1] (default profiles/surface.json).
The method of tools/time_yuv420.py: 48 frames per call, device events around a window of at least `--window-s` seconds of
back-to-back calls, the configurations alternated over `--reps` rounds, every round's value kept, one process.

1. Kernels, at 240x320 and 1080x1920 with resize=256 bilinear, as us per frame, for the fused call and the conversion alone:
   (a)  compact NV12 through the existing entry points of this tree
   (a0) the same two entry points of another build of the library (`--parent-lib`: the parent commit's libadvhip.so), called
        with the same arguments; (a) and (a0) both go through raw ctypes calls, so they differ by the library alone
   (s)  the same compact NV12 bytes as the compact surface, surface("nv12", H, W), through the two surface entry points of this
        tree, raw ctypes calls as (a) and (a0): what the compact calls would cost on the surface kernels
   (b)  NV12 with an aligned pitch and aligned rows (1080p: pitch 2048, rows 1088; 240x320: pitch 384, rows 256)
   (c)  P010 with an aligned pitch and aligned rows (1080p: pitch 4096, rows 1088; 240x320: pitch 768) -- twice the source bytes
   (d)  compact yuv420p10le
   (b), (c), (d) and a second (a) go through resize.resize_u8 / resize.yuv420_to_rgb_u8 and are recorded against that (a).
   The rule for the compact calls: they may run through the surface kernels only if the median of (s) does not exceed the
   median of (a0) by more than (a0)'s own spread over its rounds, fused and conversion alone, at both sizes.  (a) against (a0)
   is recorded the same way: it shows that the compact calls as this tree runs them cost what the parent's do.
2. extract_video_frames windows/s from pinned host 1080p frames, ten crops and the centre crop: P010 pitched, NV12 pitched and
   packed RGB of the same video (the P010 samples are four times the NV12 ones: the limited-range conversions agree exactly).
   P010 crosses the bus at RGB's byte count; what it saves is a conversion on the host, which this tool does not time.
3. `--bench-tree FILE --bench-parent FILE`: the JSON lines of one bench.py run of this tree and of the parent, kept for the record.

    python tools/time_surface.py [out.json] [--parent-lib PATH] [--calls 100] [--window-s 0.3] [--reps 5] [--frames 48]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from anomaly_detection_on_video_amd import _lib, resize
from anomaly_detection_on_video_amd.extract import extract_video_frames
from anomaly_detection_on_video_amd.i3d import I3Res50
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "surface.json"))
ap.add_argument("--parent-lib", default=None, help="libadvhip.so of the parent commit, for (a0)")
ap.add_argument("--calls", type=int, default=100, help="the least calls per timed window")
ap.add_argument("--window-s", type=float, default=0.3, help="the least length of a timed window")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--frames", type=int, default=48, help="video length of part 2")
ap.add_argument("--bench-tree", default=None)
ap.add_argument("--bench-parent", default=None)
ap.add_argument("--label", default="")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("time_surface: no GPU visible (the numbers are device times)")
dev = torch.device("cuda:0")
NF = 48
COMPACT = ("advhip_yuv420_to_rgb_u8", "advhip_resize_yuv420_u8")
libs = {"a_raw": _lib.load()}
if args.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in COMPACT:
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    libs["a0_raw"] = parent
rec = {"tool": "tools/time_surface.py", "label": args.label, "device": torch.cuda.get_device_name(0), "frames_per_call": NF,
       "min_calls_per_window": args.calls, "min_window_s": args.window_s, "rounds": args.reps, "parent_lib": bool(args.parent_lib), "kernels": [],
       "rule": "the compact 8-bit calls may run through the surface kernels only if median(s_raw) - median(a0_raw) <= max(a0_raw) - min(a0_raw), "
               "fused and conversion alone, at both sizes; otherwise they keep the parent's kernels (a_raw - a0_raw: this tree's compact calls "
               "against the parent's, recorded the same way)"}


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3 / NF  # us per frame


def align(v, a):
    return -(-v // a) * a


def noise(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).to(dev)


within = {"a_raw": True, "s_raw": True}
for h, w in [(240, 320), (1080, 1920)]:
    oh, ow = resize.output_size(h, w, 256)
    t = resize.tables(h, w, oh, ow, "bilinear", dev)
    p, tb, (o_xb, o_xk, o_yb, o_yk) = t.plan, t.buf, t.offsets
    rows, pa = (align(h, 32), 256) if h > 240 else (256, 128)  # (a 1080p surface is 2048 x 1088; a small one aligns its pitch less)
    surfaces = {"a": None, "b_nv12_pitched": resize.surface("nv12", h, w, pitch=align(w, pa), rows=rows),
                "c_p010_pitched": resize.surface("nv12", h, w, pitch=align(2 * w, 2 * pa), rows=rows, bits=10),
                "d_yuv420p10le": resize.surface("i420", h, w, bits=10)}
    layouts = {"a": "nv12", "b_nv12_pitched": "nv12", "c_p010_pitched": "nv12", "d_yuv420p10le": "i420"}
    src = {k: noise((NF, h // 2 * 3, w) if s is None else (NF, s.frame_bytes_min), h + i) for i, (k, s) in enumerate(surfaces.items())}
    full = torch.empty((NF, h, w, 3), device=dev, dtype=torch.uint8)
    out = torch.empty((NF, oh, ow, 3), device=dev, dtype=torch.uint8)
    ws = torch.empty((NF * p.rows * ow * 3,), device=dev, dtype=torch.uint8)
    coef, s0 = resize.yuv_coefficients("nv12"), _lib.stream(out)
    fused, alone = {}, {}
    for k, s in surfaces.items():
        fused[k] = lambda k=k, s=s: resize.resize_u8(src[k], 256, out=out, pixel_format=layouts[k], surface=s)
        alone[k] = lambda k=k, s=s: resize.yuv420_to_rgb_u8(src[k], layouts[k], out=full, surface=s)
    for k, lib in libs.items():  # the compact entry points of either library, the same arguments
        fused[k] = lambda lib=lib: lib.advhip_resize_yuv420_u8(src["a"].data_ptr(), out.data_ptr(), ws.data_ptr(), NF, 1, h, w, 3, oh, ow,
                                                               tb[o_xb:].data_ptr(), tb[o_xk:].data_ptr(), p.xcoef.shape[1], tb[o_yb:].data_ptr(),
                                                               tb[o_yk:].data_ptr(), p.ycoef.shape[1], p.row0, p.rows, 0, *coef, s0)
        alone[k] = lambda lib=lib: lib.advhip_yuv420_to_rgb_u8(src["a"].data_ptr(), full.data_ptr(), NF, 1, h, w, 0, *coef, s0)
    cs = resize.surface("nv12", h, w)  # the compact frame as a surface, through this tree's surface entry points
    geo = (cs.bits, cs.shift, cs.y_offset, cs.y_pitch, cs.cb_offset, cs.cr_offset, cs.chroma_pitch, cs.chroma_step)
    fused["s_raw"] = lambda: libs["a_raw"].advhip_resize_yuv420_surface_u8(src["a"].data_ptr(), out.data_ptr(), ws.data_ptr(), NF, 1, cs.frame_bytes_min, h, w, 3,
                                                                        oh, ow, tb[o_xb:].data_ptr(), tb[o_xk:].data_ptr(), p.xcoef.shape[1],
                                                                        tb[o_yb:].data_ptr(), tb[o_yk:].data_ptr(), p.ycoef.shape[1], p.row0, p.rows, *geo,
                                                                        *coef, s0)
    alone["s_raw"] = lambda: libs["a_raw"].advhip_yuv420_surface_to_rgb_u8(src["a"].data_ptr(), full.data_ptr(), NF, 1, cs.frame_bytes_min, h, w, *geo, *coef, s0)
    for what, runs in (("fused", fused), ("convert_alone", alone)):
        want = runs["a"]().clone()
        same = {k: bool(fn() == 0 and torch.equal(out if what == "fused" else full, want)) for k, fn in runs.items() if k.endswith("_raw")}
        for fn in runs.values():  # warm-up: code objects, tables, the allocator's blocks
            for _ in range(10):
                fn()
        calls = {k: max(args.calls, int(args.window_s * 1e6 / (timed(fn, 20) * NF)) + 1) for k, fn in runs.items()}
        us = {k: [] for k in runs}
        for _ in range(args.reps):
            for k, fn in runs.items():
                us[k].append(round(timed(fn, calls[k]), 3))
        med = {k: float(np.median(v)) for k, v in us.items()}
        row = {"geometry": f"{h}x{w}->{oh}x{ow}", "what": what, "raw_calls_equal_a": same, "calls_per_window": calls, "us_per_frame": us,
               "median_us_per_frame": med, "spread_us_per_frame": {k: [min(v), max(v)] for k, v in us.items()},
               "source_bytes_per_frame": {k: (h * w * 3 // 2 if s is None else s.frame_bytes_min) for k, s in surfaces.items()},
               "over_a": {k: round(med[k] / med["a"], 3) for k in surfaces if k != "a"}}
        if "a0_raw" in us:
            row["a0_spread"] = round(max(us["a0_raw"]) - min(us["a0_raw"]), 3)
            for k in within:
                row[k[0] + "_minus_a0"] = round(med[k] - med["a0_raw"], 3)
                row[k[0] + "_spread"] = round(max(us[k]) - min(us[k]), 3)
                row[k[0] + "_within_rule"] = row[k[0] + "_minus_a0"] <= row["a0_spread"]
                within[k] = within[k] and row[k[0] + "_within_rule"]
        rec["kernels"].append(row)
        print(json.dumps(row), flush=True)
    del src, full, out, ws
if "a0_raw" in libs:
    rec["a_within_a0_spread_everywhere"], rec["s_within_a0_spread_everywhere"] = within["a_raw"], within["s_raw"]

# 2. the driver from pinned host 1080p frames: P010 pitched, NV12 pitched, packed RGB of the same video
m = I3Res50()
m.load_state_dict(synth_i3d_state_dict())
m = m.eval().to(dev)
F, h, w, rows = args.frames, 1080, 1920, 1088
g = np.random.default_rng(5)
y, cb, cr = g.integers(0, 256, (F, h, w), dtype=np.uint8), g.integers(0, 256, (F, h // 2, w // 2), dtype=np.uint8), g.integers(0, 256, (F, h // 2, w // 2), dtype=np.uint8)
s8, s10 = resize.surface("nv12", h, w, pitch=2048, rows=rows), resize.surface("nv12", h, w, pitch=4096, rows=rows, bits=10)
nv12 = g.integers(0, 256, (F, rows * 3 // 2, 2048), dtype=np.uint8)  # noise in the padding
nv12[:, :h, :w], nv12[:, rows : rows + h // 2, 0:w:2], nv12[:, rows : rows + h // 2, 1:w:2] = y, cb, cr
p010 = g.integers(0, 256, (F, rows * 3 // 2, 4096), dtype=np.uint8)
p16 = p010.view("<u2")
p16[:, :h, :w] = y.astype(np.uint16) << 8 | (p16[:, :h, :w] & 63)  # (4 Y) << 6, noise kept in the low six bits
p16[:, rows : rows + h // 2, 0:w:2] = cb.astype(np.uint16) << 8 | (p16[:, rows : rows + h // 2, 0:w:2] & 63)
p16[:, rows : rows + h // 2, 1:w:2] = cr.astype(np.uint16) << 8 | (p16[:, rows : rows + h // 2, 1:w:2] & 63)
hosts = {"p010_pitched": torch.from_numpy(p010).view(F, -1).pin_memory(), "nv12_pitched": torch.from_numpy(nv12).view(F, -1).pin_memory()}
hosts["rgb"] = resize.yuv420_to_rgb_u8(hosts["nv12_pitched"].to(dev), "nv12", surface=s8).cpu().pin_memory()
del y, cb, cr, nv12, p010, p16
more = {"p010_pitched": dict(pixel_format="nv12", surface=s10), "nv12_pitched": dict(pixel_format="nv12", surface=s8), "rgb": {}}
rec["extract"] = []
for crops in ("ten", "center"):
    runs = {k: (lambda k=k: extract_video_frames(m, hosts[k], resize=256, crops=crops, **more[k])) for k in hosts}
    feats = {k: fn() for k, fn in runs.items()}
    same = all(np.array_equal(v, feats["rgb"]) for v in feats.values())
    n = 1 + max(0, -(-(F - 16) // 16))
    calls = {}
    for k, fn in runs.items():  # (warm: all ran above) one call's time -> the calls that fill a window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        calls[k] = int(args.window_s / (time.perf_counter() - t0)) + 1
    rates = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls[k]):
                fn()  # ends in .cpu(): synchronised
            rates[k].append(round(n * calls[k] / (time.perf_counter() - t0), 2))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    row = {"frames": f"{h}x{w}", "video_frames": F, "windows": n, "source": "pinned host", "crops": crops, "same_features": same, "calls_per_sample": calls,
           "windows_per_s": rates, "median": med, "spread": {k: [min(v), max(v)] for k, v in rates.items()},
           "h2d_MiB": {k: round(v.numel() / 2**20, 1) for k, v in hosts.items()},
           "over_rgb": {k: round(med[k] / med["rgb"], 4) for k in hosts if k != "rgb"}}
    rec["extract"].append(row)
    print(json.dumps(row), flush=True)

# 3. bench.py's line of this tree and of the parent, for the record
for key, path in (("bench_tree", args.bench_tree), ("bench_parent", args.bench_parent)):
    if path and os.path.exists(path):
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        rec[key] = json.loads(lines[-1]) if lines else None

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", args.out)
