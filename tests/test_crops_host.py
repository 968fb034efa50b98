"""Crop subsets of TenCrop (crops=): the host-side rules -- names, checks, the 4-bit packing, file-name tags -- and the C ABI of
the four `_crops` entry points, which refuse a malformed set or range before anything launches.  No GPU."""
import itertools
import os
import re
import subprocess
import sys

import pytest

from conftest import REPO

TEN = tuple(range(10))


def test_resolve_crops_names_and_tuples():
    from anomaly_detection_on_video_amd.ops import resolve_crops

    assert resolve_crops(None) == TEN and resolve_crops("ten") == TEN
    assert resolve_crops("five") == (0, 1, 2, 3, 4)
    assert resolve_crops("center") == resolve_crops("centre") == (4,)
    assert resolve_crops("center_flip") == (4, 9)
    assert resolve_crops((0, 3, 5, 9)) == (0, 3, 5, 9) and resolve_crops([4]) == (4,) and resolve_crops(TEN) == TEN
    import numpy as np

    assert resolve_crops(np.array([4, 9])) == (4, 9) and all(type(c) is int for c in resolve_crops(np.array([4, 9])))
    # every strictly ascending subset is accepted as it is
    for n in (1, 2, 9):
        for sub in itertools.combinations(range(10), n):
            assert resolve_crops(sub) == sub


@pytest.mark.parametrize("bad", [(4, 4), (9, 4), (10,), (), (-1,), (0, 1, 1), (4.0,), (True,), "centre_flip", "", 4, TEN + (9,), ("4",)])
def test_resolve_crops_refuses(bad):
    from anomaly_detection_on_video_amd.ops import resolve_crops

    with pytest.raises(ValueError):
        resolve_crops(bad)


def test_packing_round_trip():
    from anomaly_detection_on_video_amd.ops import pack_crops, unpack_crops

    assert pack_crops(None) == (10, 0x9876543210) == pack_crops("ten")
    assert pack_crops("center") == (1, 0x4) and pack_crops("center_flip") == (2, 0x94) and pack_crops("five") == (5, 0x43210)
    for n in range(1, 11):
        for sub in itertools.combinations(range(10), n):
            nc, packed = pack_crops(sub)
            assert nc == n and packed < 1 << (4 * n) and unpack_crops(nc, packed) == sub
            for j, c in enumerate(sub):  # the kernels' lookup
                assert (packed >> (4 * j)) & 15 == c


def test_file_name_tags_for_every_stride_and_crop_combination():
    from anomaly_detection_on_video_amd.extract import feature_tag
    from anomaly_detection_on_video_amd.ops import crops_tag

    assert crops_tag(None) == crops_tag("ten") == crops_tag(TEN) == ""
    assert crops_tag("center") == "_c4" and crops_tag("five") == "_c01234" and crops_tag((4, 9)) == "_c49" and crops_tag((0, 3, 5, 9)) == "_c0359"
    for stride, stag in ((None, ""), (16, ""), (8, "_s8"), (1, "_s1")):
        for crops, ctag in ((None, ""), ("ten", ""), ("center", "_c4"), ("center_flip", "_c49"), ("five", "_c01234"), ((0, 4, 9), "_c049")):
            assert feature_tag(16, stride, crops) == stag + ctag
    assert feature_tag() == ""  # the reference's own names
    assert feature_tag(16, 8, (4,)) == "_s8_c4"  # the stride first: <name>_i3d_s8_c4.npy, <name>_s8_c4_<seg>.npy
    tags = {feature_tag(16, s, c) for s in (16, 8, 4) for c in itertools.chain([None], itertools.combinations(range(10), 2))}
    assert len(tags) == 3 * (1 + 45)  # no two ways of extracting share a name
    with pytest.raises(ValueError):
        feature_tag(16, 8, (9, 4))
    with pytest.raises(ValueError):
        feature_tag(16, 17, None)


def test_frame_crops_key_carries_the_set():
    import torch

    from anomaly_detection_on_video_amd.pipeline import FrameCrops

    fr = torch.zeros((16, 8, 8, 3), dtype=torch.uint8)
    plain = FrameCrops(fr, 0, 10, 16, 8)
    assert plain.key() == ("u8", 10, (8, 8), 16, 8, 16) == FrameCrops(fr, 0, 10, 16, 8, crops=None).key()  # today's key
    keys = {FrameCrops(fr, 0, 2, 16, 8, crops=c).key() for c in ((4, 9), (0, 9), "center_flip", None)}
    assert len(keys) == 3
    assert FrameCrops(fr, 0, 2, 16, 8, crops="center_flip").crops == (4, 9)
    with pytest.raises(ValueError):
        FrameCrops(fr, 0, 2, 16, 8, crops=(9, 4))


NEW_SYMBOLS = {
    "advhip_tencrop_normalize_u8_crops": 14,
    "advhip_tencrop_normalize_planes_u8_crops": 16,
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_crops_f32": 20,
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_crops_f32": 21,
}


def _header_prototypes():
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(advhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_and_ctypes_agree_on_the_new_entry_points():
    """Each new symbol: declared in include/advhip.h, exported, and its ctypes signature has the header's argument list, type by
    type -- (ncrops, crops_packed) sit right behind clip_stride as (int32_t, uint64_t) in all four."""
    import ctypes as C

    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    protos = _header_prototypes()
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_float: "float"}
    for name, n_args in NEW_SYMBOLS.items():
        assert name in protos, f"{name} not declared in include/advhip.h"
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(argtypes) == n_args, name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p)
            else:
                assert p.split()[0] == kinds[t], (name, p, t)
        names = [p.split()[-1] for p in params]
        i = names.index("ncrops")
        assert names[i - 1 : i + 2] == (["crop", "ncrops", "crops_packed"] if "normalize" in name else ["clip_stride", "ncrops", "crops_packed"])
        assert argtypes[i] is C.c_int32 and argtypes[i + 1] is C.c_uint64
    assert lib.advhip_abi_version() == 2  # (the ABI only gained entry points)


BAD_SETS = [
    (0, 0x0, b"ncrops outside [1, 10]"),
    (11, 0x9876543210, b"ncrops outside [1, 10]"),
    (-1, 0x4, b"ncrops outside [1, 10]"),
    (1, 0xA, b"crop index above 9"),
    (2, 0xF4, b"crop index above 9"),
    (2, 0x44, b"not strictly ascending"),
    (2, 0x49, b"not strictly ascending"),
    (1, 0x94, b"bits set above the last crop index"),
    (10, 0x19876543210, b"bits set above the last crop index"),
    (2, 0x94 | 1 << 63, b"bits set above the last crop index"),
]


def test_crops_entry_points_validate_before_any_launch():
    """Bad ncrops, bad packing and out-of-range crop-clip ranges are refused with a message (nothing below launches: every call
    fails validation; the pointers are not device memory)."""
    import ctypes as C

    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    p = C.c_void_p(4096)  # stands for a device pointer
    f = C.c_float
    stem = _lib.ConvDesc(8, 3, 16, 224, 224, 64, 5, 7, 7, 2, 2, 2, 2, 3, 3, 1, 0, 0)
    FH, FW = 256, 340
    dense = lambda F, s, nc, pk, first: (p, p, F, FH, FW, 3, 16, s, 224, nc, pk, f(114.75), f(57.375), None)
    planes = lambda F, s, nc, pk, first: (p, p, F, FH, FW, 3, 16, s, 224, nc, pk, first, 8, f(114.75), f(57.375), None)
    taps = lambda F, s, nc, pk, first: (C.byref(stem), p, F, FH, FW, s, nc, pk, F * FH * FW * 3 + 4, first, p, p, p, p, p, f(57.375), p, 0, p,
                                        1 << 40, None)
    byts = lambda F, s, nc, pk, first: (C.byref(stem), p, F, FH, FW, s, nc, pk, first, p, p, p, p, p, f(57.375), p, 0, p, 1 << 40, None)
    fns = ((lib.advhip_tencrop_normalize_u8_crops, dense), (lib.advhip_tencrop_normalize_planes_u8_crops, planes),
           (lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_crops_f32, taps), (lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_crops_f32, byts))
    for fn, args in fns:
        for nc, pk, msg in BAD_SETS:
            assert fn(*args(40, 8, nc, pk, 0)) == -1, (fn, nc, hex(pk))
            assert msg in lib.advhip_last_error() and b"crop set" in lib.advhip_last_error(), (nc, hex(pk), lib.advhip_last_error())
        assert fn(*args(40, 17, 2, 0x94, 0)) == -1 and b"clip stride 17" in lib.advhip_last_error()  # (the stride's checks are kept)
    # ranges: 40 frames at stride 8 = 4 windows; batches of 8 crop-clips
    for fn, args in fns[1:]:
        assert fn(*args(40, 8, 2, 0x94, 1)) == -1  # 4 x 2 = 8 crop-clips: [1, 9) is one past the end
        assert (b"outside the video's 8" in lib.advhip_last_error()) or (b"outside the 4 clips x 2 crops" in lib.advhip_last_error())
        assert fn(*args(40, 8, 5, 0x43210, 13)) == -1  # 4 x 5 = 20: [13, 21)
        assert (b"outside the video's 20" in lib.advhip_last_error()) or (b"outside the 4 clips x 5 crops" in lib.advhip_last_error())
        assert fn(*args(40, 8, 1, 0x4, 0)) == -1  # 4 x 1 = 4 < 8
        assert fn(*args(40, 8, 10, 0x9876543210, 33)) == -1
        assert fn(*args(40, 8, 2, 0x94, -1)) == -1


def test_cli_crops_needs_frame_size_and_a_valid_set():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "extract_features.py"), *a], capture_output=True, text=True, cwd=REPO)
    r = run("--crops", "center")
    assert r.returncode == 2 and "--crops needs --frame-size" in r.stderr
    r = run("--frame-size", "240x320", "--crops", "9,4")
    assert r.returncode == 2 and "strictly ascending" in r.stderr
    r = run("--frame-size", "240x320", "--crops", "middle")
    assert r.returncode == 2 and "--crops" in r.stderr


def test_cli_parse_crops_and_main_refusal():
    import argparse

    import extract_features

    assert extract_features.parse_crops("center") == (4,) and extract_features.parse_crops("0,4,9") == (0, 4, 9)
    assert extract_features.parse_crops("ten") == TEN and extract_features.parse_crops("five") == (0, 1, 2, 3, 4)
    for bad in ("4,4", "10", "", "a,b"):
        with pytest.raises(argparse.ArgumentTypeError):
            extract_features.parse_crops(bad)
    with pytest.raises(ValueError, match="--crops needs --frame-size"):
        extract_features.main(crops=(4,))
