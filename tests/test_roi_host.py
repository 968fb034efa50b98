"""Regions of interest, host side (no GPU): the box rule restated in numpy (tests/_roi_ref.py) against the Pillow goldens and
live Pillow, resize.box_coefficients / box_plan / roi_tables against the restatement, the pass rule and the identity tables, every
refusal by its message, and the C ABI of the three roi entry points (argument checks before any launch; header, exports and
ctypes signatures)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import _roi_ref as ref
from anomaly_detection_on_video_amd import resize
from conftest import GOLDEN, REPO

FILTERS = ref.FILTERS
ONE = 1 << 22


def _goldens():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "roi_*.npz")))
    assert len(paths) == 2
    for p in paths:
        h, w = (int(v) for v in os.path.basename(p)[len("roi_"):-len(".npz")].split("x"))
        yield (h, w), np.load(p)


def test_goldens_record_pillow_and_their_boxes():
    kinds = set()
    for (h, w), g in _goldens():
        assert str(g["pillow_version"]), "the goldens record the Pillow version they were made with"
        boxes = ref.golden_boxes(h, w)
        assert [str(n) for n in g["names"]] == list(boxes) and np.array_equal(g["boxes"], np.array(list(boxes.values()), dtype=np.float64))
        oh, ow = (int(v) for v in g["out_hw"])
        for name, (l, t, r, b) in boxes.items():
            assert 0 <= l < r <= w and 0 <= t < b <= h
            for f in FILTERS:
                assert g[f"{f}/{name}"].shape == (oh, ow, 3) and g[f"{f}/{name}"].dtype == np.uint8
            kinds |= {k for k, hit in (("integer", all(float(v).is_integer() for v in (l, t, r, b))), ("fractional", not float(l).is_integer()),
                                       ("left", l == 0), ("top", t == 0), ("right", r == w), ("bottom", b == h), ("thin", r - l < 1),
                                       ("flat", b - t < 1), ("full_height", (t, b) == (0, h) and (l, r) != (0, w)),
                                       ("full_width", (l, r) == (0, w) and (t, b) != (0, h)), ("odd_left", float(l).is_integer() and int(l) % 2 == 1)) if hit}
        assert os.path.getsize(os.path.join(GOLDEN, f"roi_{h}x{w}.npz")) < 32 * 1024
    assert kinds == {"integer", "fractional", "left", "top", "right", "bottom", "thin", "flat", "full_height", "full_width", "odd_left"}


def test_restatement_equals_pillow_goldens():
    for (h, w), g in _goldens():
        x = ref.roi_input(h, w)[0]
        out_hw = tuple(int(v) for v in g["out_hw"])
        for name, box in ref.golden_boxes(h, w).items():
            for f in FILTERS:
                got = ref.resize_box(x, out_hw, box, f)
                assert np.array_equal(got, g[f"{f}/{name}"]), ((h, w), name, f, int((got != g[f"{f}/{name}"]).sum()))


def _random_box(rng, h, w, integer):
    while True:
        if integer:
            l, r = sorted(int(v) for v in rng.integers(0, w + 1, 2))
            t, b = sorted(int(v) for v in rng.integers(0, h + 1, 2))
        else:
            l, r = sorted(float(v) for v in rng.uniform(0, w, 2))
            t, b = sorted(float(v) for v in rng.uniform(0, h, 2))
        if np.float32(np.float32(r) - np.float32(l)) > 0 and np.float32(np.float32(b) - np.float32(t)) > 0:
            return (l, t, r, b)


def test_restatement_equals_live_pillow_on_random_boxes():
    """A few hundred random integer and float boxes, sizes 2 - 120, the four filters: the order of the float32 roundings is part
    of the rule (with the box left in double, or the extent subtracted in double, some dozens of these cases differ)."""
    Image = pytest.importorskip("PIL.Image")
    codes = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
    rng = np.random.default_rng(20261021)
    for case in range(300):
        h, w, oh, ow = (int(v) for v in rng.integers(2, 121, 4))
        box = _random_box(rng, h, w, integer=case % 3 == 0)
        x = ref.roi_input(h, w, 1, f"live/{case}")[0]
        f = FILTERS[case % 4]
        want = np.asarray(Image.fromarray(x).resize((ow, oh), codes[f], box=box, reducing_gap=None))
        got = ref.resize_box(x, (oh, ow), box, f)
        assert np.array_equal(got, want), (case, (h, w), (oh, ow), box, f, int((got != want).sum()))


def test_box_coefficients_equal_the_restatement_and_coefficients():
    rng = np.random.default_rng(5)
    for case in range(120):
        n, m = (int(v) for v in rng.integers(1, 200, 2))
        a, b = sorted(float(v) for v in rng.uniform(0, n, 2))
        if case % 4 == 0:
            a, b = float(int(a)), float(int(b) + 1)
        if not np.float32(np.float32(b) - np.float32(a)) > 0:
            continue
        for f in FILTERS:
            bounds, coef = resize.box_coefficients(n, a, b, m, f)
            wb, wk = ref.axis_tables(n, a, b, m, f)
            assert bounds.dtype == coef.dtype == np.int32 and np.array_equal(bounds, wb) and np.array_equal(coef, wk), (n, m, a, b, f)
            assert bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n and bounds[:, 1].min() >= 1
    for n, m in ((5, 5), (64, 20), (341, 256), (7, 1), (1, 9), (240, 256), (1080, 256)):
        for f in FILTERS:
            got, want = resize.box_coefficients(n, 0, n, m, f), resize.coefficients(n, m, f)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, m, f)
    # the float32 rounding is visible: 0.1 and 0.1 + 2^-30 are one float32, and a box edge is that float32, not the double
    a = resize.box_coefficients(50, 0.1, 40.7, 13, "bicubic")
    b = resize.box_coefficients(50, float(np.float32(0.1)), float(np.float32(40.7)), 13, "bicubic")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad in ((10, -0.5, 5), (10, 2, 10.5), (10, 4, 4), (10, 5, 4), (10, 3, 3 + 1e-9), (10, float("nan"), 4), (10, 0, float("inf"))):
        with pytest.raises(ValueError, match="is not a non-empty part of"):
            resize.box_coefficients(bad[0], bad[1], bad[2], 8)


def test_pass_rule_and_identity_tables():
    h, w = 38, 46
    for box, oh, ow, want in [
        (None, 38, 46, (False, False)), ((0, 0, 46, 38), 38, 46, (False, False)), ((0, 0, 46, 38), 38, 30, (True, False)),
        ((1, 0, 46, 38), 38, 46, (True, False)), ((0, 0, 45.5, 38), 38, 46, (True, False)), ((0, 0.5, 46, 38), 38, 46, (False, True)),
        ((0, 0, 46, 37), 38, 46, (False, True)), ((0, 0, 46, 38), 20, 46, (False, True)), ((3, 2, 40, 30), 38, 46, (True, True)),
    ]:
        for f in FILTERS:
            p = resize.box_plan(h, w, oh, ow, box, f)
            assert (p.horizontal, p.vertical) == want == ref.passes(h, w, oh, ow, box), (box, oh, ow)
            if not p.horizontal:  # the explicit identity, not a computed table
                assert p.xbounds.tolist() == [[i, 1] for i in range(w)] and p.xcoef.tolist() == [[ONE]] * w
            if not p.vertical:
                assert p.ybounds.tolist() == [[i, 1] for i in range(h)] and p.ycoef.tolist() == [[ONE]] * h and (p.row0, p.rows) == (0, h)
            assert (p.row0, p.rows) == (int(p.ybounds[0, 0]), int(p.ybounds[-1, 0] + p.ybounds[-1, 1] - p.ybounds[0, 0]))
    p = resize.box_plan(h, w, 16, 70, (5, 10, 40.5, 30.25), "bilinear")
    assert 8 <= p.row0 <= 10 and p.row0 + p.rows <= 32  # the horizontal pass covers the rows the vertical table reads, and no more
    # the computed scale-1 tables happen to be identities too, but nothing rests on it
    for n in (5, 64):
        for f in FILTERS:
            bounds, coef = resize.coefficients(n, n, f)
            assert all(int(coef[i, j]) == (ONE if bounds[i, 0] + j == i else 0) for i in range(n) for j in range(bounds[i, 1]))


def test_box_output_size():
    assert resize.box_output_size((0, 0, 340, 256), 256) == resize.output_size(256, 340, 256) == (256, 340)
    assert resize.box_output_size((0, 0, 320, 240), 256) == resize.output_size(240, 320, 256)
    assert resize.box_output_size((10, 20, 90, 80), (7, 9)) == (7, 9)
    assert resize.box_output_size((1.3, 2.7, 40.2, 30.1), 16) == (16, int(16 * float(np.float32(np.float32(40.2) - np.float32(1.3))) / float(np.float32(np.float32(30.1) - np.float32(2.7)))))
    assert resize.box_output_size((0, 0, 30, 90), 10) == (30, 10)
    with pytest.raises(ValueError):
        resize.box_output_size((0, 0, 900, 1), (0, 4))


def test_roi_tables_padding_and_rowspan():
    h, w, oh, ow = 38, 46, 20, 12
    boxes = [None, (1, 0, 40.5, 38), (20.2, 3, 20.9, 30), (0, 10.5, 46, 11.25), (3, 2, 9, 8)]
    t = resize.roi_tables(h, w, (oh, ow), boxes, "bicubic", "cpu")
    assert isinstance(t, resize.RoiTables) and t.n_tables == 5 and (t.in_h, t.in_w, t.out_h, t.out_w, t.resample) == (h, w, oh, ow, "bicubic")
    plans = [resize.box_plan(h, w, oh, ow, b, "bicubic") for b in boxes]
    kx, ky = max(p.xcoef.shape[1] for p in plans), max(p.ycoef.shape[1] for p in plans)
    assert len({p.xcoef.shape[1] for p in plans}) > 1 and len({p.ycoef.shape[1] for p in plans}) > 1  # a downscale and an upscale share the table
    assert t.xbounds.shape == (5, ow, 2) and t.xcoef.shape == (5, ow, kx) and t.ybounds.shape == (5, oh, 2) and t.ycoef.shape == (5, oh, ky)
    for k, p in enumerate(plans):
        assert np.array_equal(t.xbounds[k], p.xbounds) and np.array_equal(t.ybounds[k], p.ybounds)
        nx, ny = p.xcoef.shape[1], p.ycoef.shape[1]
        assert np.array_equal(t.xcoef[k, :, :nx], p.xcoef) and not t.xcoef[k, :, nx:].any()
        assert np.array_equal(t.ycoef[k, :, :ny], p.ycoef) and not t.ycoef[k, :, ny:].any()
        assert t.rowspan[k].tolist() == [p.row0, p.rows]
    assert t.rowspan.dtype == np.int32 and t.ws_rows == max(p.rows for p in plans) == h
    assert t.boxes[0] == (0.0, 0.0, float(w), float(h)) and t.boxes[2][0] == float(np.float32(20.2))
    buf = t.buf.numpy()
    assert t.buf.dtype.is_floating_point is False and buf.dtype == np.int32
    parts = [t.xbounds, t.xcoef, t.ybounds, t.ycoef, t.rowspan]
    assert buf.size == sum(a.size for a in parts)
    for o, a in zip(t.offsets, parts):
        assert np.array_equal(buf[o : o + a.size], a.reshape(-1))
    small = resize.roi_tables(h, w, (oh, ow), [(3, 2, 9, 8)], "box", "cpu")
    assert small.ws_rows == 6 and small.rowspan.tolist() == [[2, 6]]


def test_refusals_by_message():
    h, w = 38, 46
    for box, msg in [
        ((1, 2, 3), "four host numbers"), ("abcd", "four host numbers"), (5, "four host numbers"), ((1, 2, 3, 4, 5), "four host numbers"),
        ((0, 0, float("nan"), 4), "not a finite host number"), ((0, 0, float("inf"), 4), "not a finite host number"), ((0, 0, "4", 4), "not a finite host number"),
        ((0, 0, True, 4), "not a finite host number"), ((0, 0, None, 4), "not a finite host number"),
        ((-1, 0, 4, 4), "leaves the 38 x 46 frame"), ((0, -0.5, 4, 4), "leaves the 38 x 46 frame"), ((0, 0, 46.5, 4), "leaves the 38 x 46 frame"),
        ((0, 0, 4, 39), "leaves the 38 x 46 frame"),
        ((4, 0, 4, 4), "is empty"), ((5, 0, 4, 4), "is empty"), ((0, 7, 4, 7), "is empty"), ((3, 0, 3 + 1e-9, 4), "is empty"),
    ]:
        for call in (lambda: resize.resolve_box("resize_u8", box, h, w), lambda: resize.roi_tables(h, w, (8, 8), [None, box], "bilinear", "cpu"),
                     lambda: resize.box_plan(h, w, 8, 8, box)):
            with pytest.raises(ValueError, match=msg):
                call()
    import torch

    with pytest.raises(ValueError, match="four host numbers"):
        resize.resolve_box("resize_u8", torch.tensor([0, 0, 4, 4]), h, w)
    for boxes in ([], None, "ab", 7):
        with pytest.raises(ValueError, match="at least one box"):
            resize.roi_tables(h, w, (8, 8), boxes, "bilinear", "cpu")
    with pytest.raises(ValueError, match="not an .h, w. pair"):
        resize.roi_tables(h, w, 8, [None], "bilinear", "cpu")
    with pytest.raises(ValueError, match="at least 1 x 1"):
        resize.roi_tables(h, w, (0, 8), [None], "bilinear", "cpu")
    for bad in (0, 5, "nearest", "hamming"):
        with pytest.raises(ValueError, match="not supported"):
            resize.roi_tables(h, w, (8, 8), [None], bad, "cpu")
        with pytest.raises(ValueError, match="not supported"):
            resize.box_coefficients(10, 1, 5, 4, bad)
    from anomaly_detection_on_video_amd import extract

    with pytest.raises(ValueError, match="box= names a part of the decoded frames: it needs resize="):
        extract.extract_video_frames(None, torch.zeros((16, 8, 8, 3), dtype=torch.uint8), box=(0, 0, 4, 4))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

ROI_SYMBOLS = {"advhip_resize_roi_u8": 23, "advhip_resize_roi_yuv420_u8": 30, "advhip_resize_roi_surface_u8": 38}


def _lib_built():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib, _lib.load()


def test_header_exports_and_ctypes_agree_on_the_roi_entry_points():
    _lib, lib = _lib_built()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "advhip.h")).read(), flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(advhip_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    assert {n for n in protos if "_roi_" in n} == set(ROI_SYMBOLS)
    assert not any(n.endswith("_sampled") or n.endswith("_sampled_f32") for n in ROI_SYMBOLS)
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t"}
    for name, n_args in ROI_SYMBOLS.items():
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int
        params = [p.strip() for p in protos[name].split(",")]
        assert len(params) == len(argtypes) == n_args, (name, len(params), len(argtypes))
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            else:
                assert p.split()[0] == kinds[t], (name, p, t)
    assert lib.advhip_abi_version() == 2


def test_roi_entry_points_validate_before_any_launch():
    """Every call below fails validation, so nothing is launched; the pointers are never dereferenced on the host."""
    _lib, lib = _lib_built()
    p = C.c_void_p(4096)  # stands for a device pointer
    H, W = 38, 46
    coef = (16, 76309, 104597, 25675, 53279, 132201)
    nv12 = (8, 0, 0, 64, 64 * 40, 64 * 40 + 1, 64, 2)  # pitch 64, 40 allocated rows
    pitch = 64 * 40 + 64 * 20

    def call(form, src=p, dst=p, ws=p, F=3, N=7, src_of=p, step=1, table_of=p, nt=5, H=H, W=W, Ch=3, OH=16, OW=70, xb=p, xk=p, kx=7, yb=p, yk=p, ky=5,
             rowspan=p, ws_rows=H, layout=0, surface=nv12, frame_pitch=pitch):
        head = (src, dst, ws, F, N, src_of, step, table_of, nt)
        tail = (H, W, Ch, OH, OW, xb, xk, kx, yb, yk, ky, rowspan, ws_rows)
        if form == "rgb":
            return lib.advhip_resize_roi_u8(*head, *tail, None)
        if form == "yuv":
            return lib.advhip_resize_roi_yuv420_u8(*head, *tail, layout, *coef, None)
        return lib.advhip_resize_roi_surface_u8(*head, frame_pitch, *tail, *surface, *coef, None)

    shared = [
        (dict(src=None), b"null frames or output"), (dict(dst=None), b"null frames or output"), (dict(ws=None), b"null workspace"),
        (dict(step=0), b"frame step 0"), (dict(F=0), b"sizes must be >= 1"), (dict(N=0), b"sizes must be >= 1"), (dict(OW=0), b"sizes must be >= 1"),
        (dict(OH=-1), b"sizes must be >= 1"), (dict(Ch=4), b"3 channels"), (dict(nt=0), b"0 tables"),
        (dict(xb=None), b"null horizontal tables"), (dict(xk=None), b"null horizontal tables"), (dict(yb=None), b"null vertical tables"),
        (dict(yk=None), b"null vertical tables"), (dict(kx=0), b"horizontal ksize 0"), (dict(ky=0), b"vertical ksize 0"),
        (dict(rowspan=None), b"null rowspan"), (dict(ws_rows=0), b"ws_rows 0 outside [1, 38]"), (dict(ws_rows=39), b"ws_rows 39 outside [1, 38]"),
        (dict(N=1 << 40, OH=1 << 20, OW=1 << 20), b"overflow int64"),
        (dict(src_of=None, N=4), b"output frame 3 at frame step 1 is past the 3 source frames"),
        (dict(src_of=None, N=3, step=2), b"output frame 2 at frame step 2 is past the 3 source frames"),
    ]
    for form in ("rgb", "yuv", "surface"):
        for kw, msg in shared:
            assert call(form, **kw) == -1, (form, kw)
            assert msg in lib.advhip_last_error(), (form, kw, lib.advhip_last_error())
    assert call("rgb", H=0) == -1 and b"sizes must be >= 1" in lib.advhip_last_error()
    assert call("rgb", W=1 << 30, ws_rows=1) == -1 and b"too long" in lib.advhip_last_error()
    for kw, msg in [(dict(H=37, ws_rows=37), b"even H and W"), (dict(W=45), b"even H and W"), (dict(layout=2), b"neither NV12 (0) nor I420 (1)")]:
        assert call("yuv", **kw) == -1 and msg in lib.advhip_last_error(), (kw, lib.advhip_last_error())
    for kw, msg in [
        (dict(surface=(9,) + nv12[1:]), b"9-bit samples"), (dict(surface=nv12[:3] + (45,) + nv12[4:]), b"luma pitch 45 below a row"),
        (dict(frame_pitch=100), b"a plane ends past the frame's 100 bytes"), (dict(surface=nv12[:7] + (3,)), b"chroma step 3"),
        (dict(W=45), b"even H and W"),
    ]:
        assert call("surface", **kw) == -1 and msg in lib.advhip_last_error(), (kw, lib.advhip_last_error())
