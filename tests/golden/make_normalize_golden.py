#!/usr/bin/env python3
"""Generate tests/golden/normalize.npz by running the REFERENCE's three normalisers (src/gtransforms.py:57-112:
GroupStandardizationTenCrop, GroupPixelMinmaxTenCrop, GroupRGBChannelMinmaxTenCrop) on one small uint8 input.

    python -B tests/golden/make_normalize_golden.py [--out DIR] [--reference DIR]

Dev-only: needs the reference tree (read-only; absent on the GPU box).  Its src/gtransforms.py is imported with an empty
placeholder module for `torchvision`, which the three normalisers do not touch; no reference arithmetic is restated or replaced
here.  The file holds the input `x` uint8 (3, 10, 3, 8, 8) = (frames, crops, C, H, W) -- one constant crop and one constant
channel planted, so the reference's 0 / 0 = NaN is part of the fixture -- and one fp32 array of that shape per key of
tests/_normalize_ref.CASES.  Nothing at test time reads the reference.
"""
from __future__ import annotations

import argparse
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("ADV_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))

from _normalize_ref import CASES, golden_input  # noqa: E402


def load_gtransforms(ref: str):
    try:
        import torchvision.transforms  # noqa: F401
    except ImportError:  # (absent from this image: an empty placeholder, as make_golden.py registers)
        tv = types.ModuleType("torchvision")
        tv.__spec__ = importlib.machinery.ModuleSpec("torchvision", None)
        tv.transforms = types.ModuleType("torchvision.transforms")
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    spec = importlib.util.spec_from_file_location("_reference_gtransforms", os.path.join(ref, "src", "gtransforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_normaliser(g, case):
    """A key's normalisation as the reference's object.  Its constructors test isinstance(x, float): every number goes in as a
    float, per-channel values as lists of floats."""
    if case is None:
        return g.GroupStandardizationTenCrop()
    if isinstance(case, str):
        return {"pixel_minmax": g.GroupPixelMinmaxTenCrop, "channel_minmax": g.GroupRGBChannelMinmaxTenCrop}[case]()
    kind, a, b = case
    arg = lambda v: [float(e) for e in v] if isinstance(v, tuple) else float(v)
    cls = {"standardize": g.GroupStandardizationTenCrop, "pixel_minmax": g.GroupPixelMinmaxTenCrop,
           "channel_minmax": g.GroupRGBChannelMinmaxTenCrop}[kind]
    return cls(arg(a), arg(b))


def generate(ref: str = REF):
    g = load_gtransforms(ref)
    x = golden_input()
    arrays = {"x": x}
    for key, case in CASES.items():
        t = torch.from_numpy(x.copy()).float()  # ToTensorTenCrop's .float(); the normalisers write into their argument
        arrays[key] = reference_normaliser(g, case)(t).numpy().astype(np.float32)
    return arrays


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--reference", default=REF)
    a = ap.parse_args()
    arrays = generate(a.reference)
    path = os.path.join(a.out, "normalize.npz")
    np.savez_compressed(path, **arrays)
    nans = {k: int(np.isnan(v).sum()) for k, v in arrays.items() if k != "x"}
    print(f"{path}: {os.path.getsize(path)} bytes, NaNs {nans}")
