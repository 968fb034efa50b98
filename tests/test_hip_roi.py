"""GPU tests of the regions of interest (csrc/resize.hip: advhip_resize_roi_u8 and its 4:2:0 forms; resize.resize_rois_u8,
resize_u8(box=), extract_video_frames(box=), LiveFrames(rois=, source_of=)): bytes equal the numpy restatement of Pillow's box
resize (tests/_roi_ref.py) with no tolerance, from every source form; what must not be written; the equivalences with the calls
without a box; features and rings through the public entry points."""
import numpy as np
import pytest
import torch

import _roi_ref as ref
import _surface_ref
import _yuv_ref
from _live_frames_ref import FrameRingRef
from _live_gate_ref import MotionGateRef

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
H, W, F_SRC, N = 38, 46, 3, 7  # even sizes (4:2:0); N is no multiple of the 4 rows a block computes
# a row longer than one wave's 64 lanes; a 3 x downscale; the whole height kept (the identity table for the whole-frame box)
OUTS = [(16, 70), (20, 12), (38, 30)]
# the whole frame; an odd left edge (the 4:2:0 tap walk starts mid chroma pair) touching the top and the right edge; fractional;
# under one pixel wide; touching the left and the bottom edge
BOXES = [None, (5, 0, 46, 30), (1.3, 2.7, 42.6, 36.85), (23.2, 12, 23.9, 24.5), (0, 10.5, 20, 38)]
SRC_OF = [2, 0, 1, 1, 0, 2, 0]    # repeats, out of order
TABLE_OF = [0, 1, 2, 3, 4, 1, 3]
FILTERS = ref.FILTERS


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _sources():
    """form -> (device frames, keyword arguments, the RGB frames they stand for)"""
    from anomaly_detection_on_video_amd import resize

    out = {}
    rgb = ref.roi_input(H, W, F_SRC, "hip")
    out["rgb"] = (rgb, {}, rgb)
    for layout in ("nv12", "i420"):
        yuv = _yuv_ref.noise(H, W, F_SRC, 11)
        out[layout] = (yuv, {"pixel_format": layout}, _yuv_ref.yuv420_to_rgb(yuv, layout))
    for name, bits, pitch in (("nv12_surface", 8, 64), ("p010", 10, 128)):  # a pitch above W (2 W bytes at 10 bits), 40 allocated rows
        geo = _surface_ref.geometry("nv12", H, W, pitch=pitch, rows=40, bits=bits)
        buf = _surface_ref.pack(*_surface_ref.noise_planes(H, W, F_SRC, bits, 12), geo, seed=3)
        out[name] = (buf, {"pixel_format": "nv12", "surface": resize.Surface(*geo)}, _surface_ref.to_rgb(buf, geo))
    return out


_CACHE = {}


def _source(form):
    if not _CACHE:
        _CACHE.update(_sources())
    return _CACHE[form]


_WANT = {}


def _want(form, out_hw, f):
    """The restatement's (N, OH, OW, 3) for the module's boxes, SRC_OF and TABLE_OF: computed once per (form, size, filter)."""
    key = (form, out_hw, f)
    if key not in _WANT:
        rgb = _source(form)[2]
        _WANT[key] = np.stack([ref.resize_box(rgb[s], out_hw, BOXES[t], f) for s, t in zip(SRC_OF, TABLE_OF)])
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _guarded(n, pad=37):
    """A view of n bytes inside a sentinel-filled buffer, at an odd offset."""
    big = torch.full((n + 2 * pad,), FILL, dtype=torch.uint8, device=DEV)
    return big, big[pad : pad + n]


def _untouched(big, n, pad=37):
    return bool((big[:pad] == FILL).all()) and bool((big[pad + n :] == FILL).all())


def test_the_shapes_take_the_paths_they_are_meant_for():
    from anomaly_detection_on_video_amd import resize

    assert N % 4 and OUTS[0][1] > 64 and H % 2 == 0 and W % 2 == 0
    t = resize.roi_tables(H, W, OUTS[1], BOXES, "bilinear", DEV)
    plans = [resize.box_plan(H, W, *OUTS[1], b, "bilinear") for b in BOXES]
    assert len({p.xcoef.shape[1] for p in plans}) > 1 and len({p.ycoef.shape[1] for p in plans}) > 1  # a downscale and an upscale share the padded table
    assert t.xcoef.shape[2] == max(p.xcoef.shape[1] for p in plans) and len(set(t.rowspan[:, 1].tolist())) > 1
    assert np.array_equal(_np(t.buf[t.offsets[4] :]).reshape(-1, 2), t.rowspan)
    whole = resize.box_plan(H, W, *OUTS[2], None, "bilinear")
    assert whole.horizontal and not whole.vertical  # the identity table runs through the vertical kernel
    assert int(BOXES[1][0]) % 2 == 1 and BOXES[3][2] - BOXES[3][0] < 1
    assert sorted(set(SRC_OF)) == list(range(F_SRC)) and SRC_OF != sorted(SRC_OF) and sorted(set(TABLE_OF)) == list(range(len(BOXES)))


@pytest.mark.parametrize("out_hw", OUTS)
@pytest.mark.parametrize("form,filters", [("rgb", FILTERS), ("nv12", ("bilinear", "lanczos")), ("i420", ("bilinear", "bicubic")),
                                          ("nv12_surface", ("bilinear", "box")), ("p010", ("bilinear", "bicubic"))])
def test_bytes_equal_the_restatement_and_nothing_else_is_written(form, filters, out_hw):
    from anomaly_detection_on_video_amd import resize

    frames, kw, _ = _source(form)
    d = _dev(frames)
    oh, ow = out_hw
    for f in filters:
        t = resize.roi_tables(H, W, out_hw, BOXES, f, DEV)
        n_out, n_ws = N * oh * ow * 3, N * t.ws_rows * ow * 3
        big, flat = _guarded(n_out)
        big_ws, ws = _guarded(n_ws)
        got = resize.resize_rois_u8(d, t, table_of=TABLE_OF, src_of=SRC_OF, out=flat.view(N, oh, ow, 3), ws=ws, **kw)
        assert np.array_equal(_np(got), _want(form, out_hw, f)), (form, out_hw, f)
        assert _untouched(big, n_out) and _untouched(big_ws, n_ws), (form, out_hw, f)
    # device index vectors, and a workspace and an output of the call's own: the same bytes
    got = resize.resize_rois_u8(d, t, table_of=_dev(np.array(TABLE_OF, dtype=np.int32)), src_of=_dev(np.array(SRC_OF, dtype=np.int32)), **kw)
    assert tuple(got.shape) == (N, oh, ow, 3) and np.array_equal(_np(got), _want(form, out_hw, f))


@pytest.mark.parametrize("form", ["rgb", "i420", "p010"])
def test_a_bad_source_or_table_index_leaves_its_frame_alone(form):
    from anomaly_detection_on_video_amd import resize

    frames, kw, _ = _source(form)
    out_hw, f = OUTS[1], "bilinear"
    oh, ow = out_hw
    t = resize.roi_tables(H, W, out_hw, BOXES, f, DEV)
    src_of, table_of = list(SRC_OF), list(TABLE_OF)
    src_of[1], src_of[4], table_of[2], table_of[6] = F_SRC, -1, len(BOXES), -1
    bad = (1, 2, 4, 6)
    big, flat = _guarded(N * oh * ow * 3)
    got = _np(resize.resize_rois_u8(_dev(frames), t, table_of=table_of, src_of=src_of, out=flat.view(N, oh, ow, 3), **kw))
    want = _want(form, out_hw, f)
    for i in range(N):
        assert np.array_equal(got[i], np.full_like(want[i], FILL) if i in bad else want[i]), (form, i)
    assert _untouched(big, N * oh * ow * 3)


def test_a_rowspan_outside_the_frame_counts_no_taps():
    """rowspan is device memory the host cannot check: a span that leaves the frame or the workspace reads nothing (the frame
    comes out as the sums without taps, 0) and its neighbours are right."""
    from anomaly_detection_on_video_amd import resize

    frames, kw, _ = _source("rgb")
    out_hw, f = OUTS[1], "bilinear"
    t = resize.roi_tables(H, W, out_hw, BOXES, f, DEV)
    for span in ((-1, 10), (30, 20), (0, H + 1), (5, -3)):
        buf = t.buf.clone()
        buf[t.offsets[4] + 2 : t.offsets[4] + 4] = torch.tensor(span, dtype=torch.int32, device=DEV)  # table 1
        got = _np(resize.resize_rois_u8(_dev(frames), t._replace(buf=buf), table_of=TABLE_OF, src_of=SRC_OF))
        want = _want("rgb", out_hw, f)
        for i in range(N):
            assert np.array_equal(got[i], np.zeros_like(want[i]) if TABLE_OF[i] == 1 else want[i]), (span, i)


def test_resize_u8_with_a_box():
    from anomaly_detection_on_video_amd import resize

    for form in ("rgb", "nv12"):
        frames, kw, rgb = _source(form)
        d = _dev(frames)
        for box, size, f in (((5, 0, 46, 30), (20, 12), "bicubic"), ((1.3, 2.7, 42.6, 36.85), 16, "bilinear"), ([0, 10.5, 20, 38], (16, 70), "lanczos")):
            out_hw = resize.box_output_size(box, size)
            want = ref.resize_box(rgb, out_hw, box, f)
            got = resize.resize_u8(d, size, f, box=box, **kw)
            assert tuple(got.shape) == (F_SRC,) + out_hw + (3,) and np.array_equal(_np(got), want), (form, box)
            n_tables = len(resize._ROI_TABLES)
            got2 = resize.resize_u8(d, size, f, box=tuple(box), frame_step=2, **kw)  # frames 0 and 2, the cached tables
            assert np.array_equal(_np(got2), want[::2]) and len(resize._ROI_TABLES) == n_tables, (form, box)
        # the whole frame as a box is the call without one; one None box through resize_rois_u8 is resize_u8
        for size in ((20, 12), (38, 30), 16, (H, W)):
            plain = resize.resize_u8(d, size, "bicubic", **kw)
            assert torch.equal(resize.resize_u8(d, size, "bicubic", box=(0, 0, W, H), **kw), plain), (form, size)
            t = resize.roi_tables(H, W, tuple(plain.shape[1:3]), [None], "bicubic", DEV)
            assert torch.equal(resize.resize_rois_u8(d, t, **kw), plain), (form, size)


def test_resize_rois_refusals():
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    frames, _, _ = _source("rgb")
    d = _dev(frames)
    t = resize.roi_tables(H, W, (8, 8), [None, (1, 1, 9, 9)], "bilinear", DEV)
    for kw, msg in [
        (dict(table_of=[0, 1], src_of=[0]), "table_of has 2 entries, src_of 1"), (dict(table_of=[0] * 4), "table_of has 4 entries"),
        (dict(src_of=[0, 1], frame_step=2), "frame_step has no meaning"), (dict(table_of=[0.5]), "sequence of host integers"),
        (dict(table_of=torch.zeros(3, dtype=torch.int64, device=DEV)), "contiguous int32 vector"),
        (dict(out=torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)), "out must be uint8"),
        (dict(ws=torch.zeros((10,), dtype=torch.uint8, device=DEV)), "ws must be a contiguous uint8 tensor of at least"),
    ]:
        with pytest.raises((HipExtensionError, ValueError), match=msg):
            resize.resize_rois_u8(d, t, **kw)
    with pytest.raises(HipExtensionError, match="the tables are for 38 x 46 frames, these are 8 x 8"):
        resize.resize_rois_u8(torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV), t)
    with pytest.raises(HipExtensionError, match="rois must be a RoiTables"):
        resize.resize_rois_u8(d, None)
    with pytest.raises(ValueError, match="leaves the 38 x 46 frame"):
        resize.resize_u8(d, 8, box=(0, 0, 47, 8))


def test_extract_video_frames_with_a_box():
    """16 frames of 60 x 80, a fractional box resized to (256, 340), the centre crop: the features are those of the restatement's
    box-resized frames with no resize, bit for bit."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames
    from anomaly_detection_on_video_amd.i3d import I3Res50
    from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

    m = I3Res50()
    m.load_state_dict(synth_i3d_state_dict())
    m = m.eval().to(DEV)
    box = (10.25, 7, 70.5, 52.75)
    decoded = ref.roi_input(60, 80, 16, "video")
    resized = ref.resize_box(decoded, (256, 340), box, "bilinear")
    want = extract_video_frames(m, torch.from_numpy(resized), crops="center")
    got = extract_video_frames(m, torch.from_numpy(decoded), resize=(256, 340), box=box, crops="center")
    assert want.shape == (1, 1, 2048) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got_dev = extract_video_frames(m, _dev(decoded), resize=(256, 340), box=box, crops="center")
    assert np.array_equal(got_dev.view(np.uint32), want.view(np.uint32))


# ---- LiveFrames(rois=, source_of=) ---------------------------------------------------------------------------------------------
N_CAM, RING_HW, FPC = 5, (16, 20), 4
CAM_BOXES = {0: (5, 0, 46, 30), 2: (1.3, 2.7, 42.6, 36.85), 3: (0, 10.5, 20, 38)}  # cameras 1 and 4: the whole frame
PUSHES = [(0, 1, 2, 3, 4), (4, 2, 0), (0, 1, 2, 3, 4), (3, 1), (2, 4, 0, 1, 3), (0, 1, 2, 3, 4), (1, 0), (4, 3, 2, 1, 0), (0, 2, 4)]


def _live_frames(form, step, n):
    """n decoded frames of `form` for step `step`, and the RGB frames they stand for."""
    if form == "rgb":
        rgb = ref.roi_input(H, W, n, f"live/{step}")
        return rgb, {}, rgb
    yuv = _yuv_ref.noise(H, W, n, 100 + step)
    return yuv, {"pixel_format": "nv12"}, _yuv_ref.yuv420_to_rgb(yuv, "nv12")


@pytest.mark.parametrize("form", ["rgb", "nv12"])
def test_live_frames_with_rois_ring_and_windows(form):
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd.live import LiveFrames

    lf = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, clip_stride=2, device=DEV, rois=resize.RoiSpec((H, W), CAM_BOXES))
    assert lf.rois.boxes == [CAM_BOXES.get(c) for c in range(N_CAM)] and lf._roi_tables.n_tables == N_CAM
    model = FrameRingRef(N_CAM, RING_HW + (3,), FPC, 1, 2)
    seen_due = False
    for step, cams in enumerate(PUSHES):
        frames, kw, rgb = _live_frames(form, step, len(cams))
        resized = np.stack([ref.resize_box(rgb[i], RING_HW, CAM_BOXES.get(c), "bilinear") for i, c in enumerate(cams)])
        due = lf.push(cams, _dev(frames), **kw)
        assert due == model.push(list(cams), resized), (step, cams)
        assert np.array_equal(_np(lf.ring), model.ring), (step, cams)
        if due:
            seen_due = True
            assert np.array_equal(_np(lf.windows(due)), model.windows(list(due))), (step, due)
    assert seen_due and lf.counts.tolist() == list(lf.counts_host) == model.counts.tolist()


def test_live_frames_source_of_equals_repeated_frames():
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd.live import LiveFrames

    spec = resize.RoiSpec((H, W), [CAM_BOXES.get(c) for c in range(N_CAM)], "bicubic")
    a = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=spec)
    b = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=spec)
    for step in range(FPC + 1):
        frames, kw, rgb = _live_frames("nv12", step, 2)
        due_a = a.push((3, 0, 2), _dev(frames), source_of=(0, 0, 1), **kw)
        due_b = b.push((3, 0, 2), _dev(frames[[0, 0, 1]]), **kw)
        assert due_a == due_b and torch.equal(a.ring, b.ring), step
        want = np.stack([ref.resize_box(rgb[s], RING_HW, CAM_BOXES.get(c), "bicubic") for c, s in zip((3, 0, 2), (0, 0, 1))])
        assert np.array_equal(_np(a.ring[[3, 0, 2], step % FPC]), want), step
    assert (0, 0, 1) in a._sources.items and len(a._sources.items) == 1  # one upload for the five pushes
    assert torch.equal(a.windows((0, 2, 3)), b.windows((0, 2, 3)))


def test_live_frames_steady_roi_push_dispatches_no_torch_arithmetic():
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd.live import LiveFrames
    from test_hip_strict import AtenAudit

    cams, src = (0, 2, 3), (1, 0, 1)
    lf = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, clip_stride=1, device=DEV, rois=resize.RoiSpec((H, W), CAM_BOXES))
    steps = [_live_frames("nv12", s, 2) for s in range(FPC + 2)]
    dev = [_dev(f) for f, _, _ in steps]
    for d in dev[: FPC + 1]:
        due = lf.push(cams, d, pixel_format="nv12", source_of=src)
    lf.windows(due)  # (the id vector of this camera set)
    with AtenAudit() as audit:
        due = lf.push(cams, dev[FPC + 1], pixel_format="nv12", source_of=src)
        clips = lf.windows(due)
    assert due == cams
    assert audit.arithmetic() == {}, f"torch arithmetic on the live roi step: {audit.arithmetic()}"
    assert "_to_copy" not in audit.ops and "copy_" not in audit.ops and "empty" not in audit.ops, audit.ops
    rgb = steps[FPC + 1][2]
    want = np.stack([ref.resize_box(rgb[s], RING_HW, CAM_BOXES.get(c), "bilinear") for c, s in zip(cams, src)])
    assert np.array_equal(_np(clips.view(3, FPC, *RING_HW, 3)[:, -1]), want)


def test_live_frames_without_rois_is_as_before_and_refusals():
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames

    frames, _, rgb = _live_frames("rgb", 0, 3)
    plain = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV)
    none = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=None)
    assert plain.rois is None and not hasattr(plain, "_roi_tables") and not hasattr(none, "_roi_ws")
    plain.push((1, 3, 4), _dev(frames), resize=RING_HW)
    none.push((1, 3, 4), _dev(frames), resize=RING_HW)
    assert torch.equal(plain.ring, none.ring) and np.array_equal(_np(plain.ring[[1, 3, 4], 0]), ref.resize_box(rgb, RING_HW, None, "bilinear"))
    with pytest.raises(HipExtensionError, match="this LiveFrames has no rois"):
        plain.push((1, 3, 4), _dev(frames), resize=RING_HW, source_of=(0, 1, 2))
    # every camera with the None box: the bytes of push(resize=)
    whole = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=resize.RoiSpec((H, W), {}))
    whole.push((1, 3, 4), _dev(frames))
    assert torch.equal(whole.ring, plain.ring)
    lf = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=((H, W), CAM_BOXES))
    ring = lf.ring.clone()
    d = _dev(frames)
    for call, msg in [
        (lambda: lf.push((1, 3, 4), d, resize=RING_HW), "resize= together with rois"),
        (lambda: lf.push((1, 3, 4), torch.zeros((3, 40, 46, 3), dtype=torch.uint8, device=DEV)), "the rois are boxes of 38 x 46 frames, these are 40 x 46"),
        (lambda: lf.push((1, 3, 4), torch.zeros((3, 60, 46), dtype=torch.uint8, device=DEV), pixel_format="nv12"), "these are 40 x 46"),
        (lambda: lf.push((1, 3, 4), d, source_of=(0, 1)), "source_of has 2 entries for 3 listed cameras"),
        (lambda: lf.push((1, 3, 4), d, source_of=(0, 1, 3)), "source_of entry 3 is not a row of the 3 frames"),
        (lambda: lf.push((1, 3, 4), d, source_of=(0, -1, 1)), "is not a row of the 3 frames"),
        (lambda: lf.push((1, 3, 4), d, source_of=torch.tensor([0, 1, 2])), "sequence of host integers"),
        (lambda: lf.push((1, 3), d), "2 leading rows"),
    ]:
        with pytest.raises(HipExtensionError, match=msg):
            call()
    assert torch.equal(lf.ring, ring) and lf.counts_host == (0,) * N_CAM
    for rois, msg in [
        (((H, W), [None] * 4), "sequence of 5 boxes"), (((H, W), {5: (0, 0, 4, 4)}), r"cameras \[5\] outside \[0, 5\)"), (((H,), {}), "not a pair"),
        (((H, W), {0: (0, 0, 47, 4)}), "leaves the 38 x 46 frame"), (((H, W), {0: (4, 0, 4, 4)}), "is empty"), (((H, W), {}, "hamming"), "not supported"),
        ("boxes", "not a resize.RoiSpec"),
    ]:
        with pytest.raises(HipExtensionError, match=msg):
            LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=rois)


def test_live_frames_motion_gate_sees_the_resized_frames():
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd.live import LiveFrames, MotionGate

    tau, limit = 3, 40
    lf = LiveFrames(N_CAM, frame_hw=RING_HW, frames_per_clip=FPC, device=DEV, rois=resize.RoiSpec((H, W), CAM_BOXES), motion=MotionGate(tau, limit))
    gate = MotionGateRef(N_CAM, RING_HW + (3,), tau, limit, span=FPC)
    base, _, _ = _live_frames("rgb", 0, N_CAM)
    moved = False
    for step, cams in enumerate(PUSHES[:6]):
        frames = base[list(cams)].copy()
        if step % 2:  # a patch that changes inside some cameras' boxes only: whole frames would all move, the regions do not
            frames[:, 30:36, 2:12] ^= 0xFF
        resized = np.stack([ref.resize_box(frames[i], RING_HW, CAM_BOXES.get(c), "bilinear") for i, c in enumerate(cams)])
        verdicts = gate.push(list(cams), resized)
        moved |= len(set(verdicts)) == 2 and step > 1
        lf.push(cams, _dev(frames))
        assert np.array_equal(_np(lf.gate_state), gate.state) and np.array_equal(_np(lf.anchor), gate.anchor), (step, cams)
    assert moved  # a push after which some regions had moved and others had not
