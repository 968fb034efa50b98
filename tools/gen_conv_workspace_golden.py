#!/usr/bin/env python3
"""Record advhip_conv3d_workspace_bytes over a small grid as tests/golden/conv_workspace_bytes.json (host only, no GPU).

    python tools/gen_conv_workspace_golden.py [--out FILE]

Run it on the revision whose sizes are to be kept -- the parent of a change to the conv launchers' host code --
and commit the file: tests/test_conv_algo_table.py asserts that the built library still answers the same (-1, "refused",
included).  The grid pins split_layout, padded_rows and choose: rows of 98 positions (the padded-rows path), rows of a
multiple of 4, a temporal conv (with a T-fold id that its T = 4 frames do not admit: -1), splits 1..3.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from anomaly_detection_on_video_amd import _lib  # noqa: E402

# (B, Cin, T, H, W, Cout, kernel, padding), stride 1
DESCS = [(3, 64, 2, 7, 7, 128, (1, 1, 1), (0, 0, 0)), (2, 64, 4, 13, 11, 128, (1, 1, 1), (0, 0, 0)), (2, 64, 4, 13, 11, 128, (3, 1, 1), (1, 0, 0))]
ALGOS = [0, 3, 35, 67, 99, 134, 162, 163, 169, 192, 200, 226, 234]
TEMPORAL_ONLY = [211]  # a T-fold id: on the (3,1,1) descriptor only

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "conv_workspace_bytes.json"))
    out = ap.parse_args().out
    lib = _lib.load()
    rows = []
    for b, cin, t, h, w, cout, k, p in DESCS:
        for algo in ALGOS + (TEMPORAL_ONLY if k[0] > 1 else []):
            for splits in (1, 2, 3):
                d = _lib.ConvDesc(b, cin, t, h, w, cout, *k, 1, 1, 1, *p, 1, algo, splits)
                rows.append({"desc": [b, cin, t, h, w, cout, *k, *p], "algo": algo, "splits": splits, "bytes": int(lib.advhip_conv3d_workspace_bytes(C.byref(d)))})
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} sizes -> {out}")
