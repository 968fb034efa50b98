"""4:2:0 frames on the device (resize.yuv420_to_rgb_u8 -> advhip_yuv420_to_rgb_u8, resize.resize_u8(pixel_format=) ->
advhip_resize_yuv420_u8): the conversion byte-equal to the numpy restatement over every (Y, Cb, Cr) and at awkward geometries,
the fused resize byte-equal to the Pillow restatement of the converted frames and to the two-launch path, and end to end
through extract_video_frames(pixel_format=) equal to the same video converted beforehand."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _yuv_ref as ref
from _pil_resample import resize_frames
from anomaly_detection_on_video_amd import _lib, resize

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LAYOUTS = ("nv12", "i420")


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pf(layout, matrix="bt601", full=False):
    return (layout, matrix, "full" if full else "limited")


@functools.lru_cache(maxsize=None)
def _every_triple():
    """Planes of 64 frames of 512 x 512 in which every (Y, Cb, Cr) appears exactly once: Cb = chroma column, Cr = chroma row,
    Y = 4 f + the pixel's position in its 2 x 2 block."""
    f, y, x = np.ogrid[:64, :512, :512]
    luma = (4 * f + 2 * (y & 1) + (x & 1)).astype(np.uint8)
    cb = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (64, 256, 256))
    cr = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (64, 256, 256))
    codes = (luma.astype(np.int64) << 16 | cb.repeat(2, 1).repeat(2, 2).astype(np.int64) << 8 | cr.repeat(2, 1).repeat(2, 2)).reshape(-1)
    assert np.array_equal(np.sort(codes), np.arange(1 << 24))
    return luma, cb, cr


@functools.lru_cache(maxsize=1)
def _every_triple_rgb(matrix, full):
    luma, cb, cr = _every_triple()
    return ref.convert(luma, cb.repeat(2, 1).repeat(2, 2), cr.repeat(2, 1).repeat(2, 2), matrix, full)


@pytest.mark.parametrize("matrix,full,layout", [(m, f, lay) for (m, f) in ref.MODES for lay in LAYOUTS])
def test_conversion_is_the_restatement_for_every_triple(matrix, full, layout):
    x = ref.pack(*_every_triple(), layout)
    assert x.shape == (64, 768, 512)
    got = resize.yuv420_to_rgb_u8(_dev(x), _pf(layout, matrix, full)).cpu().numpy()
    want = _every_triple_rgb(matrix, full)
    assert got.shape == want.shape == (64, 512, 512, 3)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("hw", [(2, 2), (6, 10), (38, 46), (6, 12)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_conversion_small_and_awkward_geometry(hw, layout):
    """W = 2 (one pair per row), W % 4 == 2 (the pair kernel, rows that start 2 bytes off a word), W % 4 == 0 (the quad kernel at
    less than a wave); 7 frames, all of them and every third; out= inside a larger buffer at an even and at an odd offset."""
    h, w = hw
    x = ref.noise(h, w, 7, 11 * h + w)
    want = ref.yuv420_to_rgb(x, layout, "bt709", False)
    d = _dev(x)
    pf = _pf(layout, "bt709")
    assert np.array_equal(resize.yuv420_to_rgb_u8(d, pf).cpu().numpy(), want)
    got3 = resize.yuv420_to_rgb_u8(d, pf, frame_step=3)
    assert tuple(got3.shape) == (3, h, w, 3) and np.array_equal(got3.cpu().numpy(), want[::3])
    for step, off in ((None, 0), (3, 0), (None, 5), (3, 6)):
        ref_out = want if step is None else want[::3]
        buf = torch.full((off + ref_out.size + 16,), 7, device=DEV, dtype=torch.uint8)
        out = buf[off : off + ref_out.size].view(ref_out.shape)
        assert resize.yuv420_to_rgb_u8(d, pf, out=out, frame_step=step) is out
        assert np.array_equal(out.cpu().numpy(), ref_out), (step, off)
        assert bool((buf[:off] == 7).all()) and bool((buf[off + ref_out.size :] == 7).all())  # guard bytes untouched
    one = resize.yuv420_to_rgb_u8(d[5:6], pf, frame_step=4)  # a single frame, whatever the step
    assert np.array_equal(one.cpu().numpy(), want[5:6])


# (H, W), size, filter, F, frame_step
RESIZES = [((240, 320), 256, "bilinear", 5, None), ((1080, 1920), 256, "bilinear", 2, None), ((38, 46), 64, "lanczos", 5, 2),
           ((6, 10), (5, 7), "bicubic", 5, None), ((64, 64), (64, 20), "box", 5, None), ((200, 32), (201, 32), "bicubic", 5, 2),
           ((8, 8), 8, "bilinear", 5, None), ((46, 38), (11, 90), "bilinear", 4, 3)]


@pytest.mark.parametrize("case,layout", list(itertools.product(RESIZES, LAYOUTS)), ids=lambda v: v if isinstance(v, str) else f"{v[0][0]}x{v[0][1]}-{v[2]}")
def test_fused_resize_equals_pillow_restatement_of_the_converted_frames(case, layout):
    (h, w), size, filt, F, step = case
    x = ref.noise(h, w, F, h * 7 + w)
    matrix, full = ("bt709", True) if layout == "i420" else ("bt601", False)
    rgb = ref.yuv420_to_rgb(x, layout, matrix, full)
    want = resize_frames(rgb[:: step or 1], size, filt)
    d, pf = _dev(x), _pf(layout, matrix, full)
    got = resize.resize_u8(d, size, filt, frame_step=step, pixel_format=pf)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    # the fused path against the two-launch path, on the device; and out= inside a larger buffer
    two = resize.resize_u8(resize.yuv420_to_rgb_u8(d, pf), size, filt, frame_step=step)
    assert torch.equal(got, two)
    buf = torch.full((want.size + 16,), 7, device=DEV, dtype=torch.uint8)
    out = buf[: want.size].view(want.shape)
    assert resize.resize_u8(d, size, filt, out=out, frame_step=step, pixel_format=pf) is out
    assert np.array_equal(out.cpu().numpy(), want) and bool((buf[want.size:] == 7).all())


def test_side_stream_interleaved_geometries():
    a, b = ref.noise(240, 320, 5, 1), ref.noise(1080, 1920, 3, 2)
    ra = resize_frames(ref.yuv420_to_rgb(a, "nv12"), 256, "bilinear")
    rb = resize_frames(ref.yuv420_to_rgb(b, "i420", "bt709"), 256, "bicubic")
    da, db = _dev(a), _dev(b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    outs = []
    with torch.cuda.stream(s):
        for _ in range(3):  # no synchronisation between the calls: tables, workspaces and launches are ordered on `s`
            outs.append((resize.resize_u8(da, 256, "bilinear", pixel_format="nv12"),
                         resize.resize_u8(db, 256, "bicubic", pixel_format=("yuv420p", "bt709"))))
    s.synchronize()
    for ya, yb in outs:
        assert np.array_equal(ya.cpu().numpy(), ra) and np.array_equal(yb.cpu().numpy(), rb)


@functools.lru_cache(maxsize=None)
def _model():
    from anomaly_detection_on_video_amd.i3d import I3Res50
    from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

    m = I3Res50()
    m.load_state_dict(synth_i3d_state_dict())
    return m.eval().to(DEV)


@pytest.mark.parametrize("hw,kw", [((240, 320), dict(resize=256)), ((240, 320), dict(resize=256, crops="center", clip_stride=8, frame_step=2)),
                                   ((256, 340), dict())], ids=["resize", "resize-center-s8-d2", "no-resize"])
def test_extract_video_frames_from_nv12_equals_converted_frames(hw, kw):
    """40 NV12 frames (2 whole clips + an 8-frame LoopPad clip at the defaults; 2 windows of 16 every-second frames at stride 8),
    from the host and from the device: the features of the frames converted beforehand by the restatement, bit for bit."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    yuv = ref.noise(*hw, 40, 3)
    rgb = ref.yuv420_to_rgb(yuv, "nv12")
    want = extract_video_frames(m, torch.from_numpy(rgb), **kw)
    assert want.shape[-1] == 2048 and want.shape[0] >= (2 if "frame_step" in kw else 3)
    got = extract_video_frames(m, torch.from_numpy(yuv), pixel_format="nv12", **kw)
    assert np.array_equal(got, want)
    got_dev = extract_video_frames(m, _dev(yuv), pixel_format=resize.PixelFormat("nv12", "bt601", False), **kw)
    assert np.array_equal(got_dev, want)


def test_refusals():
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    good = torch.zeros((2, 12, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        resize.yuv420_to_rgb_u8(good.cpu(), "nv12")
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        resize.resize_u8(good.cpu(), 4, pixel_format="nv12")
    for fn in (lambda t: resize.yuv420_to_rgb_u8(t, "i420"), lambda t: resize.resize_u8(t, 4, pixel_format="i420")):
        with pytest.raises(ValueError, match="even W"):
            fn(torch.zeros((2, 12, 7), dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="multiple of 3"):
            fn(torch.zeros((2, 13, 8), dtype=torch.uint8, device=DEV))
        with pytest.raises(_lib.HipExtensionError, match="3H/2"):  # packed RGB frames together with a pixel format
            fn(torch.zeros((2, 12, 8, 3), dtype=torch.uint8, device=DEV))
        with pytest.raises(_lib.HipExtensionError):
            fn(good.float())
    with pytest.raises(ValueError):
        resize.resize_u8(good, 4, pixel_format="nv21")
    with pytest.raises(ValueError):
        resize.yuv420_to_rgb_u8(good, None)
    with pytest.raises(_lib.HipExtensionError):  # without a pixel format a 3-dim tensor is still refused
        resize.resize_u8(good, 4)
    with pytest.raises(_lib.HipExtensionError, match="out must be"):
        resize.yuv420_to_rgb_u8(good, "nv12", out=torch.empty((2, 8, 8, 4), dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.HipExtensionError, match="overlaps"):
        big = torch.zeros((2 * 8 * 8 * 3,), dtype=torch.uint8, device=DEV)
        resize.yuv420_to_rgb_u8(big[: 2 * 12 * 8].view(2, 12, 8), "nv12", out=big.view(2, 8, 8, 3))
    with pytest.raises(ValueError, match="3H/2"):
        extract_video_frames(_model(), torch.zeros((16, 8, 8, 3), dtype=torch.uint8), pixel_format="nv12")
    with pytest.raises(ValueError):
        extract_video_frames(_model(), torch.zeros((16, 12, 8), dtype=torch.uint8))
    # a coefficient out of range through the raw C ABI: the error code, and nothing launched (dst keeps its bytes)
    lib = _lib.load()
    dst = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    ok = resize.yuv_coefficients("nv12")
    for coef in ((16, 76309, 1 << 18) + ok[3:], (16, 0) + ok[2:], (8,) + ok[1:], ok[:5] + (-5,)):
        assert lib.advhip_yuv420_to_rgb_u8(good.data_ptr(), dst.data_ptr(), 2, 1, 8, 8, 0, *coef, _lib.stream(good)) == -1
        assert b"yuv420_to_rgb_u8" in lib.advhip_last_error()
    t = resize.tables(8, 8, 4, 4, "bilinear", DEV)
    (o_xb, o_xk, o_yb, o_yk), p = t.offsets, t.plan
    ws = torch.empty((2 * p.rows * 4 * 3,), dtype=torch.uint8, device=DEV)
    small = torch.full((2, 4, 4, 3), 9, dtype=torch.uint8, device=DEV)
    args = (good.data_ptr(), small.data_ptr(), ws.data_ptr(), 2, 1, 8, 8, 3, 4, 4, t.buf[o_xb:].data_ptr(), t.buf[o_xk:].data_ptr(), p.xcoef.shape[1],
            t.buf[o_yb:].data_ptr(), t.buf[o_yk:].data_ptr(), p.ycoef.shape[1], p.row0, p.rows)
    assert lib.advhip_resize_yuv420_u8(*args, 0, 16, 76309, 104597, 25675, 1 << 18, 132201, _lib.stream(good)) == -1
    assert lib.advhip_resize_yuv420_u8(*args, 2, *ok, _lib.stream(good)) == -1
    torch.cuda.synchronize()
    assert bool((dst == 9).all()) and bool((small == 9).all())
    assert lib.advhip_resize_yuv420_u8(*args, 0, *ok, _lib.stream(good)) == 0  # (the same call with good coefficients runs)
    torch.cuda.synchronize()
    assert np.array_equal(small.cpu().numpy(), resize_frames(ref.yuv420_to_rgb(np.zeros((2, 12, 8), np.uint8), "nv12"), 4))
