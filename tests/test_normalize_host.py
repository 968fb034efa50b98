"""Normalisation modes of the uint8-frame path: the numpy restatement against the reference's recorded outputs, the argument
forms, file-name tags, the command line and the C ABI of the three new entry points.  No GPU."""
import ctypes as C
import hashlib
import importlib.util
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

from _normalize_ref import CASES, crop_minmax_ref, golden_input, normalize_ref

GOLDEN = os.path.join(REPO, "tests", "golden", "normalize.npz")
NEW_SYMBOLS = {"advhip_crop_minmax_u8": 9, "advhip_tencrop_normalize_u8_modes": 18, "advhip_tencrop_normalize_planes_u8_modes": 20}


def _generator():
    spec = importlib.util.spec_from_file_location("make_normalize_golden", os.path.join(REPO, "tests", "golden", "make_normalize_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_restatement_equals_the_reference_outputs():
    """normalize_ref on the fixture's input gives the reference's arrays bit for bit, NaN positions included; the planted constant
    crop and constant channel put NaNs exactly where the issue says."""
    from anomaly_detection_on_video_amd import ops

    g = np.load(GOLDEN)
    x = g["x"]
    assert x.dtype == np.uint8 and x.shape == (3, 10, 3, 8, 8) and np.array_equal(x, golden_input())
    assert set(g.files) == {"x"} | set(CASES)
    for key, case in CASES.items():
        want = g[key]
        assert want.dtype == np.float32 and want.shape == x.shape
        got = normalize_ref(x.astype(np.float32), *ops.resolve_normalize(case))
        assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True), key
        nan = np.isnan(want)
        planted = np.zeros(x.shape, dtype=bool)
        if key.startswith("pix"):
            planted[1, 4] = True
        elif key.startswith("ch"):
            planted[1, 4] = True
            planted[2, 7, 1] = True
        assert np.array_equal(nan, planted), key
    # (0.1, 0.7) is the range that tells a fused multiply-add from the two rounded operations: an FMA would change outputs
    q = normalize_ref(x.astype(np.float32), "pixel_minmax", (0.0,) * 3, (1.0,) * 3).astype(np.float64)
    fused = (q * np.float64(np.float32(0.7 - 0.1)) + np.float64(np.float32(0.1))).astype(np.float32)
    ok = ~np.isnan(g["pix_01_07"])
    assert (fused[ok] != g["pix_01_07"][ok]).sum() > 100


def test_fixture_regenerates_from_the_reference():
    gen = _generator()
    if not os.path.exists(os.path.join(gen.REF, "src", "gtransforms.py")):
        pytest.skip("the reference tree is not on this machine")
    pytest.importorskip("PIL.Image")
    arrays = gen.generate()
    g = np.load(GOLDEN)
    assert set(arrays) == set(g.files)
    for k, v in arrays.items():
        assert v.dtype == g[k].dtype and np.array_equal(v, g[k], equal_nan=True), k


def test_resolve_normalize_forms():
    from anomaly_detection_on_video_amd import ops

    default = ops.Normalize("standardize", (114.75,) * 3, (57.375,) * 3)
    for spec in (None, "standardize", ("standardize", 114.75, 57.375), ("standardize", (114.75,) * 3, [57.375] * 3), default):
        assert ops.resolve_normalize(spec) == default
        assert ops.normalize_is_default(spec) and ops.normalize_tag(spec) == ""
    n = ops.resolve_normalize(("standardize", [123.675, 116.28, 103.53], (58.395, 57.12, 57.375)))
    assert n == ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)) and not ops.normalize_is_default(n)
    assert all(isinstance(v, float) for v in n.a + n.b)
    assert ops.resolve_normalize("pixel_minmax") == ("pixel_minmax", (0.0,) * 3, (1.0,) * 3)
    assert ops.resolve_normalize(("pixel_minmax", 0.1, 0.7)) == ("pixel_minmax", (0.1,) * 3, (0.7,) * 3)
    assert ops.resolve_normalize("channel_minmax") == ("channel_minmax", (0.0,) * 3, (1.0,) * 3)
    assert ops.resolve_normalize(("channel_minmax", (0, -1, 0.1), 1)) == ("channel_minmax", (0.0, -1.0, 0.1), (1.0,) * 3)
    # numbers are numbers: ints (the reference would build an empty tensor from them), numpy scalars
    assert ops.resolve_normalize(("pixel_minmax", -1, 1)) == ops.resolve_normalize(("pixel_minmax", -1.0, 1.0))
    assert ops.resolve_normalize(("standardize", 100, np.float32(50))) == ("standardize", (100.0,) * 3, (50.0,) * 3)
    assert ops.resolve_normalize(("channel_minmax", np.int64(0), 2)) == ("channel_minmax", (0.0,) * 3, (2.0,) * 3)
    # the reference's condition for the channel mode: ONE channel with lo < hi is enough
    assert ops.resolve_normalize(("channel_minmax", (0, 1, 1), (1, 1, 0))).kind == "channel_minmax"
    assert ops.resolve_normalize(n) == n  # canonical form in, canonical form out
    bad = ["minmax", "", 3, ("pixel_minmax",), ("pixel_minmax", 0), ("pixel_minmax", 0, 1, 2), ("pixel_minmax", 1, 1), ("pixel_minmax", 1, 0),
           ("pixel_minmax", (0, 0, 0.5), 1), ("pixel_minmax", float("nan"), 1), ("channel_minmax", 1, 1), ("channel_minmax", (1, 2, 3), (1, 2, 0)),
           ("channel_minmax", (0, 0), 1), ("channel_minmax", "0", 1), ("standardize", 0, 0), ("standardize", 1, (1, 0, 1)),
           ("standardize", 1, 1e-60), ("standardize", True, 1), ("standardize", 1, float("inf")), (None, 0, 1), ("standardize", None, 1)]
    for spec in bad:
        with pytest.raises(ValueError):
            ops.resolve_normalize(spec)


def test_tags_and_file_names():
    from anomaly_detection_on_video_amd import ops
    from anomaly_detection_on_video_amd.extract import feature_tag

    sha = lambda *six: hashlib.sha1(struct.pack("<6f", *six)).hexdigest()[:8]
    assert ops.normalize_tag("pixel_minmax") == ops.normalize_tag(("pixel_minmax", 0, 1)) == "_npix"
    assert ops.normalize_tag("channel_minmax") == ops.normalize_tag(("channel_minmax", (0, 0, 0), 1.0)) == "_nch"
    assert ops.normalize_tag(("pixel_minmax", -1, 1)) == "_npix-" + sha(-1, -1, -1, 1, 1, 1)
    assert ops.normalize_tag(("channel_minmax", -1, 1)) == "_nch-" + sha(-1, -1, -1, 1, 1, 1)
    assert ops.normalize_tag(("channel_minmax", (0, -1, 0.1), (1, 1, 0.7))) == "_nch-" + sha(0, -1, 0.1, 1, 1, 0.7)
    assert ops.normalize_tag(("standardize", 100, 50)) == "_nstd-" + sha(100, 100, 100, 50, 50, 50)
    assert re.fullmatch(r"_nstd-[0-9a-f]{8}", ops.normalize_tag(("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))))
    tags = {ops.normalize_tag(c) for c in CASES.values()}
    assert len(tags) == len(CASES)  # one normalisation, one name
    # every existing name is unchanged: the default's tag is empty under each spelling
    for spec in (None, "standardize", ("standardize", 114.75, 57.375)):
        assert feature_tag(normalize=spec) == "" and feature_tag(16, 8, "center", 2, spec) == "_d2_s8_c4"
    assert feature_tag(16, 8, "center", 2) == "_d2_s8_c4" and feature_tag(16, 8) == "_s8"
    assert feature_tag(normalize="pixel_minmax") == "_npix"
    assert feature_tag(16, 8, "center", 2, ("pixel_minmax", -1, 1)) == "_d2_s8_c4_npix-" + sha(-1, -1, -1, 1, 1, 1)  # the normalisation comes last
    assert feature_tag(16, None, "five", None, "channel_minmax") == "_c01234_nch"
    with pytest.raises(ValueError):
        feature_tag(normalize=("pixel_minmax", 1, 0))


def test_crop_stats_pitch_and_frame_crops_key():
    from anomaly_detection_on_video_amd import ops
    from anomaly_detection_on_video_amd.pipeline import FrameCrops

    assert ops.crop_stats_pitch(16) == 1 and ops.crop_stats_pitch(16, 8) == 1 and ops.crop_stats_pitch(16, 5, 2) == 1
    assert ops.crop_stats_pitch(16, 8, 2) == 2 and ops.crop_stats_pitch(16, None, 3) == 3 and ops.crop_stats_pitch(16, 12, 8) == 4
    for fpc, s, d in ((16, 8, 2), (16, 5, 2), (8, 12, 8), (4, 6, 9)):  # every sampled frame is a multiple of the pitch
        p = ops.crop_stats_pitch(fpc, s, d)
        assert all(i % p == 0 for w in range(ops.n_windows(100, fpc, s, d)) for i in ops.window_frame_indices(100, w, fpc, s, d))
    fr = torch.zeros((47, 72, 90, 3), dtype=torch.uint8)
    base = FrameCrops(fr, 0, 10, 16, 64)
    assert base.key() == ("u8", 10, (72, 90), 16, 64, 16)  # unchanged without the argument
    for spec in (None, "standardize", ("standardize", 114.75, 57.375)):
        assert FrameCrops(fr, 0, 10, 16, 64, normalize=spec).key() == base.key()
    keys = {base.key(), FrameCrops(fr, 0, 10, 16, 64, normalize="pixel_minmax").key(), FrameCrops(fr, 0, 10, 16, 64, normalize="channel_minmax").key(),
            FrameCrops(fr, 0, 10, 16, 64, normalize=("pixel_minmax", -1, 1)).key(), FrameCrops(fr, 0, 10, 16, 64, normalize=("standardize", 100, 50)).key(),
            FrameCrops(fr, 0, 10, 16, 64, crops="center", normalize="pixel_minmax").key()}
    assert len(keys) == 6
    assert FrameCrops(fr, 0, 10, 16, 64, normalize=("pixel_minmax", 0, 1)).key() == FrameCrops(fr, 0, 10, 16, 64, normalize="pixel_minmax").key()
    with pytest.raises(ValueError):
        FrameCrops(fr, 0, 10, 16, 64, normalize=("pixel_minmax", 1, 1))


def test_crop_minmax_ref_on_a_known_frame():
    """The test helper itself: six windows (the mirrored frame's centre crop sits one column to the right of the centre crop
    where W - crop is odd), Python-rounded centre offsets, per channel."""
    fr = np.full((2, 9, 11, 3), 100, dtype=np.uint8)
    fr[0, 0, 0, 0] = 1      # top-left only
    fr[0, 8, 10, 2] = 250   # bottom-right only
    fr[1, 4, 5, 1] = 7      # inside every window that reaches the middle
    st = crop_minmax_ref(fr, 6)
    assert st.shape == (2, 6, 3, 2)
    assert st[0, 0, 0].tolist() == [1, 100] and all(st[0, j, 0].tolist() == [100, 100] for j in (1, 2, 3, 4, 5))
    assert st[0, 3, 2].tolist() == [100, 250] and all(st[0, j, 2].tolist() == [100, 100] for j in (0, 1, 2, 4, 5))
    assert [st[1, j, 1, 0] for j in range(6)] == [7] * 6  # rows 3..8 / 0..5 / 2..7 and columns 5..10 / 0..5 / 2..7 / 3..8 all hold (4, 5)
    assert crop_minmax_ref(fr, 6, 2).shape == (1, 6, 3, 2) and np.array_equal(crop_minmax_ref(fr, 6, 2)[0], st[0])
    # W - crop = 5 is odd: the centre crop is columns 2..7, the mirrored frame's centre crop columns 3..8 of the frame
    fr[1, 4, 2, 0], fr[1, 4, 8, 2] = 9, 11
    st = crop_minmax_ref(fr, 6)
    assert [st[1, j, 0, 0] for j in range(6)] == [9, 100, 9, 100, 9, 100] and [st[1, j, 2, 0] for j in range(6)] == [100, 11, 100, 11, 100, 11]
    # ... which is what TenCrop's mirrored centre crop holds
    from oracle.host_oracle import ten_crop_clips

    raw = ten_crop_clips(fr[1:], 1, 6, mean=0.0, std=1.0)[0]  # (10, C, 1, 6, 6)
    window = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 1, 6: 0, 7: 3, 8: 2, 9: 5}
    for crop, j in window.items():
        assert raw[crop].min(axis=(1, 2, 3)).tolist() == st[1, j, :, 0].tolist() and raw[crop].max(axis=(1, 2, 3)).tolist() == st[1, j, :, 1].tolist(), crop


def test_cli_normalize_argument():
    import extract_features
    from anomaly_detection_on_video_amd import ops

    p = extract_features.parse_normalize
    assert p("pixel_minmax") == ops.resolve_normalize("pixel_minmax")
    assert p("pixel_minmax:-1,1") == ops.resolve_normalize(("pixel_minmax", -1, 1))
    assert p("channel_minmax:0.1,0.7") == ops.resolve_normalize(("channel_minmax", 0.1, 0.7))
    assert p("channel_minmax:0,-1,0.1:1,1,0.7") == ops.resolve_normalize(("channel_minmax", (0, -1, 0.1), (1, 1, 0.7)))
    assert p("standardize:123.675,116.28,103.53:58.395,57.12,57.375") == ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))
    assert p("standardize:114.75:57.375") == p("standardize") and ops.normalize_is_default(p("standardize"))
    import argparse

    for bad in ("minmax", "pixel_minmax:1,0", "pixel_minmax:0", "pixel_minmax:0,1,2", "pixel_minmax:a,b", "standardize:1:0", "standardize:1:2:3",
                "channel_minmax:0,0:1,1"):
        with pytest.raises(argparse.ArgumentTypeError):
            p(bad)
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "extract_features.py"), *a], capture_output=True, text=True, cwd=REPO)
    r = run("--normalize", "pixel_minmax:-1,1")
    assert r.returncode == 2 and "--normalize needs --frame-size" in r.stderr
    r = run("--frame-size", "240x320", "--normalize", "pixel_minmax:1,0")
    assert r.returncode == 2 and "lo must be below hi" in r.stderr
    with pytest.raises(ValueError, match="--normalize needs --frame-size"):
        extract_features.main(normalize="pixel_minmax")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def _header_prototypes():
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(advhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def _lib_built():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib, _lib.load()


def test_header_and_ctypes_agree_on_the_new_entry_points():
    _lib, lib = _lib_built()
    protos = _header_prototypes()
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_float: "float", C.c_uint64: "uint64_t"}
    for name, n_args in NEW_SYMBOLS.items():
        assert name in protos and hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert not name.endswith(("_sampled", "_sampled_f32", "_crops", "_strided"))
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(argtypes) == n_args, (name, len(params), len(argtypes))
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, p)
                if "double" in p:
                    assert t is C.POINTER(C.c_double), (name, p)
            else:
                assert p.split()[0] == kinds[t], (name, p, t)
    assert set(protos) <= set(_lib.SIGNATURES)
    assert lib.advhip_abi_version() == 2
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    for macro, val in (("ADVHIP_NORM_STANDARDIZE", _lib.NORM_STANDARDIZE), ("ADVHIP_NORM_PIXEL_MINMAX", _lib.NORM_PIXEL_MINMAX),
                       ("ADVHIP_NORM_CHANNEL_MINMAX", _lib.NORM_CHANNEL_MINMAX)):
        assert re.search(rf"#define\s+{macro}\s+{val}\b", text), macro


def test_new_entry_points_refuse_before_any_launch():
    """Every call below fails validation with ADVHIP_EINVAL (-1) and a message: nothing is launched, the fake device pointers are
    never dereferenced (the constant triples are host memory and real)."""
    _lib, lib = _lib_built()
    p = C.c_void_p(4096)  # stands for a device pointer
    ten = 0x9876543210
    tri = lambda *v: (C.c_double * 3)(*v)
    one, zero = tri(1, 1, 1), tri(0, 0, 0)
    err = lambda: lib.advhip_last_error()

    mm = lambda **k: lib.advhip_crop_minmax_u8(k.get("frames", p), k.get("stats", p), k.get("F", 48), 256, 340, 3, k.get("crop", 224), k.get("pitch", 1), None)
    assert mm(frames=None) == -1 and b"null pointer" in err()
    assert mm(stats=None) == -1 and b"null pointer" in err()
    assert mm(pitch=0) == -1 and b"frame pitch 0" in err()
    assert mm(pitch=-2) == -1
    assert mm(F=0) == -1 and b"bad arguments" in err()
    assert mm(crop=257) == -1 and b"smaller than the 257 crop" in err()

    def dense(**k):
        return lib.advhip_tencrop_normalize_u8_modes(k.get("frames", p), k.get("y", p), k.get("F", 70), 256, 340, k.get("C", 3), 16, k.get("s", 16), k.get("d", 1),
                                                     224, k.get("nc", 10), k.get("crops", ten), k.get("mode", 1), k.get("a", zero), k.get("b", one),
                                                     k.get("stats", p), k.get("pitch", 1), None)

    def planes(**k):
        return lib.advhip_tencrop_normalize_planes_u8_modes(k.get("frames", p), k.get("y", p), k.get("F", 70), 256, 340, k.get("C", 3), 16, k.get("s", 16),
                                                            k.get("d", 1), 224, k.get("nc", 10), k.get("crops", ten), k.get("first", 0), k.get("count", 10),
                                                            k.get("mode", 1), k.get("a", zero), k.get("b", one), k.get("stats", p), k.get("pitch", 1), None)

    for fn in (dense, planes):
        assert fn(frames=None) == -1 and b"null pointer" in err()
        assert fn(y=None) == -1 and b"null pointer" in err()
        assert fn(a=None) == -1 and b"null constants" in err()
        assert fn(b=None) == -1 and b"null constants" in err()
        for mode in (-1, 3, 7):
            assert fn(mode=mode) == -1 and b"unknown normalisation mode" in err()
        assert fn(mode=0, a=zero, b=tri(1, 0, 1)) == -1 and b"std must be non-zero" in err()
        assert fn(mode=0, a=zero, b=tri(1, 1, 1e-60)) == -1 and b"std must be non-zero" in err()  # zero as the fp32 the kernel takes
        assert fn(mode=1, a=one, b=one) == -1 and b"min must be below max" in err()
        assert fn(mode=1, a=tri(0, 0, 1), b=one) == -1 and b"min must be below max" in err()  # pixel mode: every entry
        assert fn(mode=1, a=tri(float("nan"), 0, 0), b=one) == -1
        assert fn(mode=2, a=one, b=tri(1, 0, -1)) == -1 and b"at least one channel" in err()
        for mode in (1, 2):
            assert fn(mode=mode, stats=None) == -1 and b"need the statistics table" in err()
            assert fn(mode=mode, pitch=0) == -1 and b"stats pitch 0" in err()
            assert fn(mode=mode, s=8, d=2, pitch=4) == -1 and b"stats pitch 4 does not divide clip stride 8 and frame step 2" in err()
            assert fn(mode=mode, s=5, d=2, pitch=2) == -1 and b"does not divide" in err()
        assert fn(crops=0x49, nc=2) == -1 and b"crop set" in err()  # descending
        assert fn(nc=11) == -1 and b"crop set" in err()
        assert fn(d=0) == -1 and b"frame step 0" in err()
        assert fn(s=17) == -1 and b"clip stride 17 outside [1, 16]" in err()
        assert fn(s=33, d=2, pitch=1) == -1 and b"clip stride 33 outside [1, 32]" in err()
        assert fn(C=4) == -1 and b"triples" in err()
        assert fn(F=0) == -1
    assert planes(first=45, count=6) == -1 and b"outside the video's 50" in err()  # 70 frames: 5 windows x 10
    assert planes(first=-1) == -1
    assert planes(count=0) == -1


TENCROP_NAMES = [f"tencrop_normalize{p}_u8{k}" for p in ("", "_planes") for k in ("", "_strided", "_crops", "_sampled", "_modes")]
# what each spelling takes beyond (frames, out, F, H, W, C, frames_per_clip, crop, [first, count,] the normalisation, stream)
TENCROP_TAKES = {"": (), "_strided": ("s",), "_crops": ("s", "crops"), "_sampled": ("s", "crops", "d"), "_modes": ("s", "crops", "d")}


@pytest.mark.parametrize("name", TENCROP_NAMES)
def test_every_tencrop_name_refuses_before_any_launch(name):
    """The ten C names of the two TenCrop passes, 70 frames of 256 x 340 x 3 in clips of 16: the refusals they share, and those of
    the arguments each one takes.  Every call returns ADVHIP_EINVAL (-1) with its message; nothing is launched, the stand-in
    device pointers are never dereferenced."""
    _lib, lib = _lib_built()
    p = C.c_void_p(4096)
    kind = name.rsplit("u8", 1)[1]
    takes, is_planes = TENCROP_TAKES[kind], "_planes" in name
    tri = lambda *v: (C.c_double * 3)(*v)

    def call(**k):
        assert set(k) <= {"frames", "out", "H", "crop", "std", "first", "count"} | set(takes) | ({"nc"} if "crops" in takes else set()), k
        args = [k.get("frames", p), k.get("out", p), 70, k.get("H", 256), 340, 3, 16]
        if "s" in takes:
            args.append(k.get("s", 16))
        if "d" in takes:
            args.append(k.get("d", 1))
        args.append(k.get("crop", 224))
        if "crops" in takes:
            args += [k.get("nc", 10), k.get("crops", 0x9876543210)]
        if is_planes:
            args += [k.get("first", 0), k.get("count", 10)]
        if kind == "_modes":  # per-channel standardisation: the mode whose constants are (mean, std)
            args += [_lib.NORM_STANDARDIZE, tri(114.75, 114.75, 114.75), tri(57.375, k.get("std", 57.375), 57.375), None, 1]
        else:
            args += [C.c_float(114.75), C.c_float(k.get("std", 57.375))]
        return getattr(lib, "advhip_" + name)(*args, None)

    err = lambda: lib.advhip_last_error()
    assert call(H=200) == -1 and b"frames (200 x 340) smaller than the 224 crop" in err()
    assert call(frames=None) == -1
    assert call(out=None) == -1
    assert call(crop=0) == -1
    assert call(crop=-2) == -1
    assert call(std=0.0) == -1 and b"std must be non-zero" in err()
    if "d" in takes:
        assert call(d=0) == -1 and b"frame step 0" in err()
        assert call(d=2, s=33) == -1 and b"clip stride 33 outside [1, 32]" in err()
    if "s" in takes:
        assert call(s=0) == -1 and b"clip stride 0 outside [1, 16]" in err()
        assert call(s=17) == -1 and b"clip stride 17 outside [1, 16]" in err()
    if "crops" in takes:
        assert call(nc=2, crops=0x49) == -1 and b"crop set" in err()    # descending
        assert call(nc=2, crops=0x44) == -1 and b"crop set" in err()    # a duplicate
        assert call(nc=1, crops=0xa) == -1 and b"crop set" in err()     # index 10
        assert call(nc=1, crops=0x14) == -1 and b"crop set" in err()    # bits above the last index
        assert call(nc=0, crops=0) == -1 and b"crop set" in err()
        assert call(nc=11) == -1 and b"crop set" in err()
    if is_planes:
        assert call(first=45, count=6) == -1 and b"outside the video's 50" in err()  # 70 frames: 5 windows x 10 crops
        assert call(first=-1) == -1 and b"outside the video's 50" in err()
        assert call(count=0) == -1 and b"outside the video's 50" in err()
