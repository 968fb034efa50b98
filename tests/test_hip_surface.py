"""Decoder surfaces on the device (surface= of resize.yuv420_to_rgb_u8, resize.resize_u8 and extract_video_frames ->
advhip_yuv420_surface_to_rgb_u8, advhip_resize_yuv420_surface_u8): row pitch, allocated rows, plane offsets, NV21 / YV12 order and
10-bit samples (P010, yuv420p10le), byte-equal to the numpy restatement (_surface_ref) whatever the padding holds, over every
8-bit triple and every 10-bit chroma pair, through the fused resize (Pillow restatement of the converted frames, and the
two-launch path), against the compact calls, end to end, and on a side stream."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _surface_ref as sref
import _yuv_ref as ref
from _pil_resample import resize_frames
from anomaly_detection_on_video_amd import _lib, resize

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pf(layout, matrix="bt601", full=False):
    return (layout, matrix, "full" if full else "limited")


def _surface(geo) -> resize.Surface:
    return resize.Surface(*geo)  # raw construction, from the restatement's own geometry arithmetic


# name -> (H, W), and the geometry's keywords from (layout, sample bytes)
GEOMETRIES = {
    "2x2": ((2, 2), lambda lay, sb: {}),
    "6x10-pitch-odd": ((6, 10), lambda lay, sb: dict(pitch=10 * sb + sb)),  # W sb + 1 at 8 bits, W sb + 2 at 10
    "6x10-yoff2": ((6, 10), lambda lay, sb: dict(y_offset=2)),
    "6x12-aligned": ((6, 12), lambda lay, sb: dict(pitch=16 * sb)),  # every offset a multiple of 4 sb: the four-pixel path under one wave
    "38x46-pitch64": ((38, 46), lambda lay, sb: dict(pitch=64 * sb, rows=40, chroma_pitch=(64 if lay == "nv12" else 32) * sb)),
    "4x520": ((4, 520), lambda lay, sb: {}),  # a lane loops twice
}


@pytest.mark.parametrize("name", list(GEOMETRIES))
@pytest.mark.parametrize("layout,order,bits", list(itertools.product(("nv12", "i420"), ("uv", "vu"), (8, 10))))
def test_conversion_at_awkward_geometry(layout, order, bits, name):
    """7 frames whose size has 5 (8 bits) or 6 (10 bits) spare bytes, so odd frames start off a word: all of them, every third,
    every fourth (frames 0 and 4 are aligned again: the four-pixel path on more than one frame), single frames at an aligned and
    at an unaligned address; noise in every padding byte and ignored bit, reseeded; out= between guard bytes."""
    (h, w), kw = GEOMETRIES[name]
    sb = 1 if bits == 8 else 2
    geo = sref.geometry(layout, h, w, bits=bits, order=order, **kw(layout, sb))
    fb = sref.frame_bytes_min(geo) + (5 if bits == 8 else 6)
    planes = sref.noise_planes(h, w, 7, bits, 11 * h + w)
    a, b = sref.pack(*planes, geo, fb, seed=1), sref.pack(*planes, geo, fb, seed=2)
    matrix, full = ("bt709", False) if bits == 8 else ("bt601", True)
    want = sref.to_rgb(a, geo, matrix, full)
    assert want.shape == (7, h, w, 3) and np.array_equal(want, sref.to_rgb(b, geo, matrix, full)) and not np.array_equal(a, b)
    sf, pf = _surface(geo), _pf(layout, matrix, full)
    da, db = _dev(a), _dev(b)
    for d in (da, db):  # the padding noise reseeded: the same result
        got = resize.yuv420_to_rgb_u8(d, pf, surface=sf)
        assert tuple(got.shape) == (7, h, w, 3) and np.array_equal(got.cpu().numpy(), want)
    for step in (3, 4):
        got = resize.yuv420_to_rgb_u8(da, pf, frame_step=step, surface=sf)
        assert np.array_equal(got.cpu().numpy(), want[::step]), step
    for f in (0, 1, 4):
        assert np.array_equal(resize.yuv420_to_rgb_u8(da[f : f + 1], pf, frame_step=4, surface=sf).cpu().numpy(), want[f : f + 1]), f
    for step, off in ((None, 0), (3, 0), (None, 5), (3, 6), (4, 8), (4, 3)):
        ref_out = want if step is None else want[::step]
        buf = torch.full((off + ref_out.size + 16,), 7, device=DEV, dtype=torch.uint8)
        out = buf[off : off + ref_out.size].view(ref_out.shape)
        assert resize.yuv420_to_rgb_u8(da, pf, out=out, frame_step=step, surface=sf) is out
        assert np.array_equal(out.cpu().numpy(), ref_out), (step, off)
        assert bool((buf[:off] == 7).all()) and bool((buf[off + ref_out.size :] == 7).all())  # guard bytes untouched


@functools.lru_cache(maxsize=None)
def _every_triple():
    """Planes of 64 frames of 512 x 512 in which every 8-bit (Y, Cb, Cr) appears exactly once (the construction of
    test_hip_yuv420._every_triple): Cb = chroma column, Cr = chroma row, Y = 4 f + the pixel's position in its 2 x 2 block."""
    f, y, x = np.ogrid[:64, :512, :512]
    luma = (4 * f + 2 * (y & 1) + (x & 1)).astype(np.uint8)
    cb = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (64, 256, 256))
    cr = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (64, 256, 256))
    codes = (luma.astype(np.int64) << 16 | sref.up2(cb).astype(np.int64) << 8 | sref.up2(cr)).reshape(-1)
    assert np.array_equal(np.sort(codes), np.arange(1 << 24))
    return luma, cb, cr


@functools.lru_cache(maxsize=None)
def _every_triple_nv21():
    geo = sref.geometry("nv12", 512, 512, pitch=576, rows=520, order="vu")
    return geo, _dev(sref.pack(*_every_triple(), geo, seed=3))


@pytest.mark.parametrize("matrix,full", sref.MODES)
def test_every_8_bit_triple_through_a_pitched_nv21_surface(matrix, full):
    geo, d = _every_triple_nv21()
    assert tuple(d.shape) == (64, 576 * 520 + 576 * 255 + 512)
    luma, cb, cr = _every_triple()
    want = sref.convert(luma, sref.up2(cb), sref.up2(cr), matrix, full, 8)
    got = resize.yuv420_to_rgb_u8(d, _pf("nv12", matrix, full), surface=_surface(geo)).cpu().numpy()
    assert got.shape == want.shape == (64, 512, 512, 3)
    assert np.array_equal(got, want), int((got != want).sum())


@functools.lru_cache(maxsize=None)
def _ten_bit_planes():
    """2 frames of 2048 x 2048: Cb = chroma column, Cr = chroma row -- every one of the 2^20 chroma pairs; Y seeded noise over
    0..1023, with frame 0's four positions of each 2 x 2 block forced to 0, 64, 940, 1023 (the extremes meet every pair)."""
    y = np.random.default_rng(20).integers(0, 1024, (2, 2048, 2048)).astype(np.uint16)
    y[0, 0::2, 0::2], y[0, 0::2, 1::2], y[0, 1::2, 0::2], y[0, 1::2, 1::2] = 0, 64, 940, 1023
    cb = np.broadcast_to(np.arange(1024, dtype=np.uint16)[None, None, :], (2, 1024, 1024))
    cr = np.broadcast_to(np.arange(1024, dtype=np.uint16)[None, :, None], (2, 1024, 1024))
    return y, cb, cr


@functools.lru_cache(maxsize=None)
def _ten_bit_frames(layout):
    geo = sref.geometry(layout, 2048, 2048, bits=10)  # nv12: P010 (noise in the low six bits); i420: yuv420p10le (in the high six)
    buf = sref.pack(*_ten_bit_planes(), geo, seed=4)
    word = buf[:, 0:8:2].astype(np.int64) | buf[:, 1:8:2].astype(np.int64) << 8
    assert (word & ~(1023 << geo[3])).any()  # the ignored bits do hold noise
    return geo, _dev(buf)


@functools.lru_cache(maxsize=1)
def _ten_bit_rgb(matrix, full):
    y, cb, cr = _ten_bit_planes()
    return sref.convert(y, sref.up2(cb), sref.up2(cr), matrix, full, 10)


@pytest.mark.parametrize("matrix,full,layout", [(m, f, lay) for (m, f) in sref.MODES for lay in ("nv12", "i420")])
def test_every_10_bit_chroma_pair_as_p010_and_yuv420p10le(matrix, full, layout):
    geo, d = _ten_bit_frames(layout)
    assert geo[3] == (6 if layout == "nv12" else 0)
    want = _ten_bit_rgb(matrix, full)
    got = resize.yuv420_to_rgb_u8(d, _pf(layout, matrix, full), surface=_surface(geo)).cpu().numpy()
    assert got.shape == want.shape == (2, 2048, 2048, 3)
    assert np.array_equal(got, want), int((got != want).sum())


# (H, W), layout, the geometry's keywords, size, filter, F, frame_step
RESIZES = [
    ((240, 320), "nv12", dict(pitch=384, rows=256, order="vu"), 256, "bilinear", 5, None),  # NV21
    ((1080, 1920), "nv12", dict(pitch=4096, rows=1088, bits=10), 256, "bilinear", 2, None),  # P010
    ((38, 46), "i420", dict(bits=10), 64, "lanczos", 5, 2),  # yuv420p10le
    ((6, 10), "i420", dict(pitch=16, order="vu"), (5, 7), "bicubic", 5, None),  # YV12
    ((64, 64), "nv12", dict(bits=10, shift=0, y_offset=6), (64, 20), "box", 5, None),  # horizontal only
    ((200, 32), "i420", dict(pitch=48, rows=208), (201, 32), "bicubic", 5, 2),  # vertical only
    ((8, 8), "nv12", dict(bits=10, order="vu", pitch=24), 8, "bilinear", 5, None),  # a copy: the conversion straight into dst
]


@pytest.mark.parametrize("case", RESIZES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1]}-{c[4]}")
def test_fused_resize_equals_pillow_restatement_of_the_converted_surfaces(case):
    (h, w), layout, kw, size, filt, F, step = case
    geo = sref.geometry(layout, h, w, **kw)
    buf = sref.pack(*sref.noise_planes(h, w, F, geo[2], h * 7 + w), geo, seed=6)
    matrix, full = ("bt709", True) if layout == "i420" else ("bt601", False)
    want = resize_frames(sref.to_rgb(buf, geo, matrix, full)[:: step or 1], size, filt)
    d, pf, sf = _dev(buf), _pf(layout, matrix, full), _surface(geo)
    got = resize.resize_u8(d, size, filt, frame_step=step, pixel_format=pf, surface=sf)
    assert tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    two = resize.resize_u8(resize.yuv420_to_rgb_u8(d, pf, surface=sf), size, filt, frame_step=step)  # the two-launch path, on the device
    assert torch.equal(got, two)
    buf2 = torch.full((3 + want.size + 16,), 7, device=DEV, dtype=torch.uint8)
    out = buf2[3 : 3 + want.size].view(want.shape)
    assert resize.resize_u8(d, size, filt, out=out, frame_step=step, pixel_format=pf, surface=sf) is out
    assert np.array_equal(out.cpu().numpy(), want) and bool((buf2[:3] == 7).all()) and bool((buf2[3 + want.size :] == 7).all())


@pytest.mark.parametrize("hw", [(38, 46), (240, 320)])
@pytest.mark.parametrize("layout", ("nv12", "i420"))
def test_compact_surface_equals_no_surface(layout, hw):
    h, w = hw
    x = _dev(ref.noise(h, w, 5, h + w))
    sf = resize.surface(layout, h, w)
    flat = x.view(5, -1)
    for step in (None, 2):
        assert torch.equal(resize.yuv420_to_rgb_u8(flat, layout, frame_step=step, surface=sf), resize.yuv420_to_rgb_u8(x, layout, frame_step=step))
        assert torch.equal(resize.resize_u8(flat, 64, "bicubic", frame_step=step, pixel_format=layout, surface=sf),
                           resize.resize_u8(x, 64, "bicubic", frame_step=step, pixel_format=layout))


@functools.lru_cache(maxsize=None)
def _model():
    from anomaly_detection_on_video_amd.i3d import I3Res50
    from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

    m = I3Res50()
    m.load_state_dict(synth_i3d_state_dict())
    return m.eval().to(DEV)


END_TO_END = [
    ("p010-resize", (240, 320), "nv12", dict(pitch=768, rows=256, bits=10), dict(resize=256)),
    ("nv21-resize-center-s8-d2", (240, 320), "nv12", dict(pitch=384, rows=256, order="vu"), dict(resize=256, crops="center", clip_stride=8, frame_step=2)),
    ("yuv420p10le-no-resize", (256, 340), "i420", dict(bits=10), dict()),
]


@pytest.mark.parametrize("hw,layout,geo_kw,kw", [c[1:] for c in END_TO_END], ids=[c[0] for c in END_TO_END])
def test_extract_video_frames_from_surfaces_equals_converted_frames(hw, layout, geo_kw, kw):
    """40 frames, from the host and from the device: the features of the frames converted beforehand by the restatement, bit for bit."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    geo = sref.geometry(layout, *hw, **geo_kw)
    buf = sref.pack(*sref.noise_planes(*hw, 40, geo[2], 3), geo, seed=8)
    want = extract_video_frames(m, torch.from_numpy(sref.to_rgb(buf, geo)), **kw)
    assert want.shape[-1] == 2048 and want.shape[0] >= (2 if "frame_step" in kw else 3)
    got = extract_video_frames(m, torch.from_numpy(buf), pixel_format=layout, surface=_surface(geo), **kw)
    assert np.array_equal(got, want)
    got_dev = extract_video_frames(m, _dev(buf), pixel_format=resize.PixelFormat(layout, "bt601", False), surface=_surface(geo), **kw)
    assert np.array_equal(got_dev, want)


def test_side_stream_interleaved_geometries():
    ga = sref.geometry("nv12", 240, 320, pitch=384, rows=256, order="vu")
    gb = sref.geometry("nv12", 1080, 1920, pitch=4096, rows=1088, bits=10)
    a = sref.pack(*sref.noise_planes(240, 320, 5, 8, 1), ga, seed=1)
    b = sref.pack(*sref.noise_planes(1080, 1920, 3, 10, 2), gb, seed=2)
    ra = resize_frames(sref.to_rgb(a, ga), 256, "bilinear")
    rb = resize_frames(sref.to_rgb(b, gb, "bt709"), 256, "bicubic")
    da, db = _dev(a), _dev(b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=DEV)
    outs = []
    with torch.cuda.stream(s):
        for _ in range(3):  # no synchronisation between the calls: tables, workspaces and launches are ordered on `s`
            outs.append((resize.resize_u8(da, 256, "bilinear", pixel_format="nv12", surface=_surface(ga)),
                         resize.resize_u8(db, 256, "bicubic", pixel_format=("nv12", "bt709"), surface=_surface(gb))))
    s.synchronize()
    for ya, yb in outs:
        assert np.array_equal(ya.cpu().numpy(), ra) and np.array_equal(yb.cpu().numpy(), rb)


def test_refusals():
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    sf = resize.surface("nv12", 8, 8, pitch=16)
    good = torch.zeros((2, sf.frame_bytes_min), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        resize.yuv420_to_rgb_u8(good.cpu(), "nv12", surface=sf)
    with pytest.raises(ValueError, match="pixel_format"):
        resize.resize_u8(good, 4, surface=sf)
    for fn in (lambda t: resize.yuv420_to_rgb_u8(t, "nv12", surface=sf), lambda t: resize.resize_u8(t, 4, pixel_format="nv12", surface=sf)):
        with pytest.raises(_lib.HipExtensionError, match="frame_bytes"):
            fn(good.view(2, -1, 8))
        with pytest.raises(_lib.HipExtensionError, match="contiguous"):
            fn(torch.zeros((2, 2 * sf.frame_bytes_min), dtype=torch.uint8, device=DEV)[:, ::2])  # not contiguous
        with pytest.raises(ValueError, match="beyond"):
            fn(good[:, :-1].contiguous())
    with pytest.raises(ValueError, match="contradicts"):
        resize.yuv420_to_rgb_u8(good, "i420", surface=sf)
    with pytest.raises(ValueError, match="frame_bytes"):
        extract_video_frames(_model(), torch.zeros((16, 12, 8), dtype=torch.uint8), pixel_format="nv12", surface=sf)
    with pytest.raises(ValueError, match="pixel_format"):
        extract_video_frames(_model(), good.cpu(), surface=sf)
    # an unaligned address at 10 bits through the raw C ABI: the error code, and nothing launched
    lib = _lib.load()
    s10 = resize.surface("nv12", 8, 8, bits=10)
    src = torch.zeros((s10.frame_bytes_min + 2,), dtype=torch.uint8, device=DEV)
    dst = torch.full((8, 8, 3), 9, dtype=torch.uint8, device=DEV)
    tail = (s10.bits, s10.shift, *s10[4:], *resize.yuv_coefficients("nv12", 10), _lib.stream(src))
    assert lib.advhip_yuv420_surface_to_rgb_u8(src.data_ptr() + 1, dst.data_ptr(), 1, 1, s10.frame_bytes_min, 8, 8, *tail) == -1
    assert b"even" in lib.advhip_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 9).all())
    assert lib.advhip_yuv420_surface_to_rgb_u8(src.data_ptr() + 2, dst.data_ptr(), 1, 1, s10.frame_bytes_min, 8, 8, *tail) == 0
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), sref.to_rgb(np.zeros((1, s10.frame_bytes_min), np.uint8), tuple(s10))[0])
