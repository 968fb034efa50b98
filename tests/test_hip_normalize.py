"""Normalisation modes from uint8 frames (per-channel mean / std, pixel and channel min-max) -- run with -m gpu.

The yardstick is tests/_normalize_ref.py: a numpy restatement of the reference's three normalisers that
tests/test_normalize_host.py pins to the reference's recorded outputs bit for bit, applied to the TenCrop geometry of
oracle.host_oracle.ten_crop_clips window by window.  Pixel comparisons are bit for bit with NaN == NaN (a constant crop or
channel gives 0 / 0 = NaN in the reference, and must here); feature comparisons are against forward_single on the dense pass's
rows at the same launch shape."""
import os

import numpy as np
import pytest
import torch

from _normalize_ref import crop_minmax_ref, tencrop_ref

pytestmark = pytest.mark.gpu

FPC = 16
MODES = {
    "std_channels": ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
    "pix_0_1": "pixel_minmax",
    "pix_01_07": ("pixel_minmax", 0.1, 0.7),   # the range at which a fused multiply-add changes about a fifth of the outputs
    "ch_m1_1": ("channel_minmax", -1.0, 1.0),
    "ch_01_07": ("channel_minmax", 0.1, 0.7),
    "ch_lists": ("channel_minmax", (0.0, -1.0, 0.1), (1.0, 1.0, 0.7)),
}
DEFAULT_SPELLINGS = [None, "standardize", ("standardize", 114.75, 57.375)]


def _dev():
    return torch.device("cuda:0")


def _frames(seed, shape, plant=True):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=shape, dtype=np.uint8)
    if plant and shape[0] > 4:
        f[2] = 93           # a constant frame: every crop of it is 0 / 0 in both min-max modes
        f[4, :, :, 1] = 17  # a constant channel: 0 / 0 in that channel of the channel mode only
    return f


_MODEL = {}


def _model():
    from anomaly_detection_on_video_amd.i3d import I3Res50
    from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict

    if "m" not in _MODEL:
        m = I3Res50()
        m.load_state_dict(synth_i3d_state_dict())
        _MODEL["m"] = m.eval().to(_dev())
    m = _MODEL["m"]
    m.fuse_pool, m.streams = True, 2
    return m


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def planes_of(dense):
    """(rows, C, T, cs, cs) -> the column-parity planes (rows, C, T, cs, 2, cs / 2 + 4) with their zero padding columns."""
    cs = dense.shape[-1]
    out = np.zeros(dense.shape[:-1] + (2, cs // 2 + 4), dtype=np.float32)
    out[..., 0, 2 : 2 + cs // 2] = dense[..., 0::2]
    out[..., 1, 2 : 2 + cs // 2] = dense[..., 1::2]
    return out


# ---- 1. the statistics kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,crop,pitch", [((5, 37, 45, 3), 32, 1), ((7, 40, 52, 3), 32, 2), ((7, 40, 52, 3), 32, 3),
                                              ((2, 256, 340, 3), 224, 1), ((3, 33, 35, 3), 31, 1), ((3, 20, 22, 2), 16, 1),
                                              ((2, 9, 11, 3), 2, 1)])
def test_crop_minmax_u8_against_numpy(shape, crop, pitch):
    """Odd row pitches (45 * 3, 35 * 3: window rows start at every byte alignment), frame pitches 2 and 3 over 7 frames, the
    reference's geometry, an odd crop (rows of 93 bytes: head, groups and tail all present), C = 2 (the byte path), and rows
    shorter than one 12-byte group."""
    from anomaly_detection_on_video_amd import ops

    frames = _frames(11 + pitch, shape, plant=False)
    got = ops.crop_minmax_u8(torch.from_numpy(frames).to(_dev()), crop, pitch)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (-(-shape[0] // pitch), 6, shape[3], 2)
    assert np.array_equal(got.cpu().numpy(), crop_minmax_ref(frames, crop, pitch))
    # a view that starts at an odd byte of its allocation: the alignment peel follows the address, not the index
    if pitch == 1:
        buf = torch.empty((frames.size + 3,), dtype=torch.uint8, device=_dev())
        for off in (1, 2, 3):
            v = buf[off : off + frames.size].view(shape)
            v.copy_(torch.from_numpy(frames))
            assert np.array_equal(ops.crop_minmax_u8(v, crop, 1).cpu().numpy(), crop_minmax_ref(frames, crop, 1)), off


def test_crop_minmax_u8_extremes_in_the_last_pixel_of_a_corner_window():
    """37 x 45 frames, crop 32: top-left rows 0..31 / cols 0..31, top-right cols 13..44, bottom rows 5..36, centre rows 2..33 / cols
    6..37 (Python-rounded halves of 5 and 13), the mirrored frame's centre crop cols 7..38.  A minimum in the last pixel of the
    last row of the bottom-right window ONLY, a maximum in the first pixel of the top-left window only, pixels just inside / just
    outside the top-left window's last row, and one column each that only the centre / only the mirrored centre holds: each
    window ends where it should, per channel."""
    from anomaly_detection_on_video_amd import ops

    H, W, cs = 37, 45, 32
    frames = np.full((2, H, W, 3), 128, dtype=np.uint8)
    frames[0, H - 1, W - 1, 1] = 1    # the frame's very last pixel: bottom-right only
    frames[0, 0, 0, 2] = 250          # the frame's first pixel: top-left only
    frames[0, 10, 38, 0] = 6          # column 38: the right-hand windows and the mirrored centre, not the centre
    frames[1, cs - 1, 12, 0] = 3      # last row of the top windows, left of the right-hand ones: top-left, bottom-left, both centres
    frames[1, cs, 0, 2] = 9           # one row below the top-left window, left of the centres: bottom-left only
    frames[1, 10, 6, 1] = 4           # column 6: the left-hand windows and the centre, not the mirrored centre
    got = ops.crop_minmax_u8(torch.from_numpy(frames).to(_dev()), cs).cpu().numpy()
    assert np.array_equal(got, crop_minmax_ref(frames, cs))
    assert [got[0, j, 1, 0] for j in range(6)] == [128, 128, 128, 1, 128, 128]
    assert [got[0, j, 2, 1] for j in range(6)] == [250, 128, 128, 128, 128, 128]
    assert [got[0, j, 0, 0] for j in range(6)] == [128, 6, 128, 6, 128, 6]
    assert [got[1, j, 0, 0] for j in range(6)] == [3, 128, 3, 128, 3, 3]
    assert [got[1, j, 2, 0] for j in range(6)] == [128, 128, 9, 128, 128, 128]
    assert [got[1, j, 1, 0] for j in range(6)] == [4, 128, 4, 128, 4, 128]


# ---- 2. both passes against the restatement -------------------------------------------------------------------------------------

# (F, clip_stride, frame_step): back-to-back clips with a short last window (LoopPad); overlapping windows; frame_step 2 at a
# stride it does not divide (statistics pitch 1) and at one it divides (pitch 2)
SAMPLINGS = [(37, None, None), (37, 8, None), (45, 5, 2), (45, 8, 2)]


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=lambda v: "F%s_s%s_d%s" % v)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_both_passes_equal_the_restatement(mode, sampling):
    from anomaly_detection_on_video_amd import mil_ops, ops

    F, s, d = sampling
    spec, crop = MODES[mode], 32
    frames = _frames(300 + F, (F, 37, 45, 3))
    fd = torch.from_numpy(frames).to(_dev())
    n = ops.n_windows(F, FPC, s, d)
    pitch = ops.crop_stats_pitch(FPC, s, d)
    assert pitch == (2 if (s, d) == (8, 2) else 1)
    minmax = ops.resolve_normalize(spec).kind != "standardize"
    for crops in (None, (4,), (0, 3, 5, 9)):
        nc = 10 if crops is None else len(crops)
        want = tencrop_ref(frames, spec, FPC, crop, s, d, crops)
        assert want.shape == (n * nc, 3, FPC, crop, crop)
        if minmax:
            assert np.isnan(want).any() and not np.isnan(want).all()  # the planted constants are inside what is compared
        got = mil_ops.tencrop_normalize_u8(fd, FPC, crop, clip_stride=s, crops=crops, frame_step=d, normalize=spec)
        assert same(got, want), (mode, sampling, crops)
        # planes: a range that starts and ends mid-clip, and the whole video
        for first, count in ((0, n * nc), (min(3, n * nc - 1), max(1, n * nc - 5))):
            if first + count > n * nc:
                continue
            xs = ops.tencrop_planes_u8(fd, first, count, FPC, crop, clip_stride=s, crops=crops, frame_step=d, normalize=spec)
            assert same(xs, planes_of(want[first : first + count])), (mode, sampling, crops, first, count)
    # a handed-in table gives the same bits; one at the wrong pitch or of another video is refused
    if minmax:
        stats = ops.crop_minmax_u8(fd, crop, pitch)
        assert same(mil_ops.tencrop_normalize_u8(fd, FPC, crop, clip_stride=s, frame_step=d, normalize=spec, crop_stats=stats),
                    tencrop_ref(frames, spec, FPC, crop, s, d))
        with pytest.raises(ValueError):
            mil_ops.tencrop_normalize_u8(fd, FPC, crop, clip_stride=s, frame_step=d, normalize=spec, crop_stats=stats[:-1])
        with pytest.raises(ValueError):
            ops.tencrop_planes_u8(fd, 0, 1, FPC, crop, clip_stride=s, frame_step=d, normalize=spec, crop_stats=ops.crop_minmax_u8(fd, crop, pitch + 1))


def test_passes_at_an_unvectorised_crop_and_the_reference_geometry():
    """crop 30 (not a multiple of 4: the scalar-store variant of the dense pass) and one window at 256 x 340 / 224."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    frames = _frames(41, (9, 33, 35, 3))
    fd = torch.from_numpy(frames).to(_dev())
    for spec in (MODES["pix_01_07"], MODES["ch_lists"], MODES["std_channels"]):
        want = tencrop_ref(frames, spec, 4, 30, 3, None, (1, 4, 7))
        assert same(mil_ops.tencrop_normalize_u8(fd, 4, 30, clip_stride=3, crops=(1, 4, 7), normalize=spec), want)
        assert same(ops.tencrop_planes_u8(fd, 1, 5, 4, 30, clip_stride=3, crops=(1, 4, 7), normalize=spec), planes_of(want[1:6]))
    frames = _frames(42, (3, 256, 340, 3), plant=False)
    fd = torch.from_numpy(frames).to(_dev())
    want = tencrop_ref(frames, MODES["pix_01_07"], 4, 224, None, None, (3, 9))
    assert same(mil_ops.tencrop_normalize_u8(fd, 4, 224, crops=(3, 9), normalize=MODES["pix_01_07"]), want)
    assert same(ops.tencrop_planes_u8(fd, 0, 2, 4, 224, crops=(3, 9), normalize=MODES["pix_01_07"]), planes_of(want))


# ---- 3. the default under its three spellings -----------------------------------------------------------------------------------

def test_default_spellings_are_the_call_without_the_argument():
    from anomaly_detection_on_video_amd import mil_ops, ops

    m = _model()
    frames = _frames(55, (37, 72, 90, 3))
    fd = torch.from_numpy(frames).to(_dev())
    dense = mil_ops.tencrop_normalize_u8(fd, FPC, 64, clip_stride=8)
    planes = ops.tencrop_planes_u8(fd, 3, 20, FPC, 64, clip_stride=8)
    fdw = ops.pad_windows_u8(fd, FPC, 8) if m.frames_need_whole_windows(64) else fd
    feats = m.forward_frames(fdw, 3, 20, FPC, 64, clip_stride=8)
    for spec in DEFAULT_SPELLINGS:
        assert torch.equal(mil_ops.tencrop_normalize_u8(fd, FPC, 64, clip_stride=8, normalize=spec), dense)
        assert torch.equal(ops.tencrop_planes_u8(fd, 3, 20, FPC, 64, clip_stride=8, normalize=spec), planes)
        assert torch.equal(m.forward_frames(fdw, 3, 20, FPC, 64, clip_stride=8, normalize=spec), feats)
        assert m.frames_need_whole_windows(64, spec) == m.frames_need_whole_windows(64)
    # ... and the same values through the `_modes` kernels, for the same per-channel constants written out
    assert torch.equal(mil_ops.tencrop_normalize_u8(fd, FPC, 64, clip_stride=8, normalize=("standardize", (114.75, 114.75, 114.5), 57.375))[:, :2], dense[:, :2])


# ---- 4. forward_frames over the whole backbone ----------------------------------------------------------------------------------

@pytest.fixture(params=["planes", "taps", "bytes"])
def form(request, monkeypatch):
    from anomaly_detection_on_video_amd import ops

    monkeypatch.setattr(ops, "U8_STEM_FORM", request.param)
    return request.param


@pytest.mark.parametrize("mode", ["std_channels", "pix_01_07", "ch_lists"])
def test_forward_frames_with_a_normalisation(form, mode):
    """crop 64, F = 37 (a short last window, never padded by the caller): rows [first, first + count) == forward_single of the
    dense pass's rows at the same launch shape, with and without a handed-in table, in every stem form (taps / bytes never run
    their stems with a normalisation) and on the separate-pass model."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    m = _model()
    spec, crop, F = MODES[mode], 64, 37
    frames = _frames(77, (F, 72, 90, 3), plant=False)
    fd = torch.from_numpy(frames).to(_dev())
    n = ops.n_windows(F, FPC) * 10
    assert n == 30 and m.frames_fused() and not m.frames_need_whole_windows(crop, spec)
    dense = mil_ops.tencrop_normalize_u8(fd, FPC, crop, normalize=spec)
    assert same(dense, tencrop_ref(frames, spec, FPC, crop))
    stats = None if mode == "std_channels" else ops.crop_minmax_u8(fd, crop)
    try:
        m.streams = 1
        for first, count in ((0, n), (7, 16)):
            want = m.forward_single(dense[first : first + count])
            assert torch.isfinite(want).all()
            got = m.forward_frames(fd, first, count, FPC, crop, normalize=spec)
            assert got.shape == (count, 2048, 1, 1, 1) and torch.equal(got, want), (form, mode, first, count)
            if stats is not None:
                assert torch.equal(m.forward_frames(fd, first, count, FPC, crop, normalize=spec, crop_stats=stats), want)
        with pytest.raises(ValueError):
            m.forward_frames(fd, n - 1, 2, FPC, crop, normalize=spec)
        if form == "planes":
            m.fuse_pool = False
            assert not m.frames_fused()
            assert torch.equal(m.forward_frames(fd, 7, 16, FPC, crop, normalize=spec), m.forward_single(dense[7:23]))
    finally:
        m.fuse_pool, m.streams = True, 2


# ---- 5. extract_video_frames ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["std_channels", "pix_01_07", "ch_lists"])
def test_extract_video_frames_with_a_normalisation(mode):
    """crop 64, F = 53: the step cut (clips_per_step 1 or 3) and where the frames live change nothing -- a frame's statistics are
    its own -- and the features are forward_single's of the restatement's pixels.  max_crop_clips = 2 makes every backbone launch
    one window's two crops whatever the step: the same launch shape on both sides (the backbone's split-K choice follows its
    batch), so the comparison is bit for bit."""
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    spec, F = MODES[mode], 53
    frames = _frames(88, (F, 72, 90, 3), plant=False)
    kw = dict(crop=64, crops="center_flip", normalize=spec, max_crop_clips=2)
    one = extract_video_frames(m, torch.from_numpy(frames), clips_per_step=1, **kw)
    assert one.shape == (4, 2, 2048) and np.isfinite(one).all()
    assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames), clips_per_step=3, **kw), one)
    assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames).to(_dev()), clips_per_step=3, **kw), one)
    assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames).to(_dev()), clips_per_step=1, **kw), one)
    assert not np.array_equal(one, extract_video_frames(m, torch.from_numpy(frames), clips_per_step=3, crop=64, crops="center_flip", max_crop_clips=2))
    dense = torch.from_numpy(tencrop_ref(frames, spec, FPC, 64, None, None, (4, 9))).to(_dev())
    try:
        m.streams = 1
        want = torch.cat([m.forward_single(dense[2 * w : 2 * w + 2]) for w in range(4)]).reshape(4, 2, 2048).cpu().numpy()
    finally:
        m.streams = 2
    assert np.array_equal(one, want)
    # overlapping windows of every second frame: the table's pitch follows the step's addressing
    got = extract_video_frames(m, torch.from_numpy(frames).to(_dev()), clips_per_step=2, clip_stride=8, frame_step=2, **kw)
    assert got.shape == (4, 2, 2048)
    assert np.array_equal(got, extract_video_frames(m, torch.from_numpy(frames), clips_per_step=3, clip_stride=8, frame_step=2, **kw))


def test_extract_video_frames_with_resize_and_a_normalisation():
    from anomaly_detection_on_video_amd.extract import extract_video_frames
    from anomaly_detection_on_video_amd.resize import resize_u8

    m = _model()
    frames = _frames(89, (37, 60, 80, 3), plant=False)
    kw = dict(crop=64, crops="center", normalize=("pixel_minmax", -1, 1), max_crop_clips=1)  # (one crop-clip per launch on both sides)
    got = extract_video_frames(m, torch.from_numpy(frames), clips_per_step=2, resize=72, **kw)
    resized = resize_u8(torch.from_numpy(frames).to(_dev()), 72)
    assert tuple(resized.shape[1:3]) == (72, 96)
    assert got.shape == (3, 1, 2048) and np.array_equal(got, extract_video_frames(m, resized, clips_per_step=2, **kw))
    assert np.array_equal(got, extract_video_frames(m, torch.from_numpy(frames).to(_dev()), clips_per_step=1, resize=72, **kw))


def test_long_video_segments_and_cache_names_with_a_normalisation(tmp_path):
    """Segments of 32 frames through the cache: stacked == the unsegmented call, the files carry the tag last, a second run reads
    every segment back, and a run with another (or no) normalisation reads none of them."""
    from anomaly_detection_on_video_amd import extract, ops

    m = _model()
    F = 53
    frames = torch.from_numpy(_frames(90, (F, 72, 90, 3), plant=False))
    reads = []

    def read(lo, hi):
        reads.append((lo, hi))
        return frames[lo:hi]

    out = str(tmp_path / "feat")
    kw = dict(crop=64, crops="center", clips_per_step=2)
    spec = ("pixel_minmax", -1, 1)
    tag = ops.normalize_tag(spec)
    assert tag.startswith("_npix-")
    whole = extract.extract_video_frames(m, frames, normalize=spec, **kw)
    seg = extract.extract_long_video_frames(m, "vid", F, read, out, seg_len=32, normalize=spec, **kw)
    assert seg.shape == (4, 1, 2048) and np.array_equal(seg, whole)
    assert reads == [(0, 32), (32, 53)]
    assert sorted(os.listdir(os.path.join(out, "vid"))) == [f"vid_c4{tag}_0.npy", f"vid_c4{tag}_1.npy"]
    run = lambda **k: extract.extract_frames([("vid", F, read)], m, out, long_video_frames=32, seg_len=32, **kw, **k)
    reads.clear()
    written = run(normalize=spec)
    assert written["vid"].endswith(f"vid_i3d_c4{tag}.npy") and reads == []  # every segment came from the cache it wrote itself
    assert np.array_equal(np.load(written["vid"]), whole)
    reads.clear()
    other = run(normalize="pixel_minmax")
    assert other["vid"].endswith("vid_i3d_c4_npix.npy") and reads == [(0, 32), (32, 53)]
    reads.clear()
    plain = run()
    assert plain["vid"].endswith("vid_i3d_c4.npy") and reads == [(0, 32), (32, 53)]
    assert not np.array_equal(np.load(plain["vid"]), whole)
    assert run(normalize=spec) == {}  # the reference's skip-if-exists rule, per name


# ---- 6. the scalar pair at channel counts other than 3 --------------------------------------------------------------------------

def scalar_pair_ref(frames, mean, std, frames_per_clip, crop, clip_stride, frame_step, crops):
    """tencrop_ref's windows and mirror with the scalar pair: (float32(px) - float32(mean)) / float32(std), any C."""
    from anomaly_detection_on_video_amd import ops
    from oracle.host_oracle import ten_crop_clips

    s, crops, d = ops.resolve_sampling(frames_per_clip, clip_stride, crops, frame_step)
    F = frames.shape[0]
    rows = []
    for w in range(ops.n_windows(F, frames_per_clip, s, d)):
        clip = frames[list(ops.window_frame_indices(F, w, frames_per_clip, s, d))]
        px = ten_crop_clips(clip, frames_per_clip, crop, mean=0.0, std=1.0)[0]  # (10, C, T, crop, crop): the pixels as floats
        assert px.dtype == np.float32
        rows.append(((px - np.float32(mean)) / np.float32(std))[list(crops)])
    return np.concatenate(rows, axis=0)


@pytest.mark.parametrize("frame_step", [None, 2])
@pytest.mark.parametrize("channels", [1, 2, 4])
def test_scalar_pair_passes_at_other_channel_counts(channels, frame_step):
    """The scalar pair takes any C (the per-channel triples do not): 9 frames, windows of 4 at stride 3 with a short last window
    (LoopPad) with and without frame_step, crops (1, 4, 7) -- a corner, the centre, a mirrored corner; crop 32 (16-byte stores) and
    30 (scalar stores); the default pair and another; planes over a range that starts and ends mid-clip.  Bit for bit."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    fpc, s, crops = 4, 3, (1, 4, 7)
    frames = _frames(600 + channels, (9, 33, 35, channels), plant=False)
    fd = torch.from_numpy(frames).to(_dev())
    n = ops.n_windows(9, fpc, s, frame_step) * len(crops)
    assert ops.window_frame_indices(9, n // 3 - 1, fpc, s, frame_step)[3] < ops.window_frame_indices(9, n // 3 - 1, fpc, s, frame_step)[2]  # LoopPad
    for crop in (32, 30):
        for pair in ({}, dict(mean=100.5, std=3.0)):
            want = scalar_pair_ref(frames, pair.get("mean", 114.75), pair.get("std", 57.375), fpc, crop, s, frame_step, crops)
            assert want.shape == (n, channels, fpc, crop, crop)
            got = mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=s, crops=crops, frame_step=frame_step, **pair)
            assert same(got, want), (crop, pair)
            for first, count in ((0, n), (1, n - 2)):
                xs = ops.tencrop_planes_u8(fd, first, count, fpc, crop, clip_stride=s, crops=crops, frame_step=frame_step, **pair)
                assert same(xs, planes_of(want[first : first + count])), (crop, pair, first, count)


def test_modes_passes_refuse_four_channels():
    """The `_modes` passes take their constants as triples: C = 4 is refused by the entry points, a four-entry parameter by
    resolve_normalize."""
    from anomaly_detection_on_video_amd import _lib, mil_ops, ops

    fd = torch.from_numpy(_frames(604, (9, 33, 35, 4), plant=False)).to(_dev())
    for spec in (MODES["std_channels"], "pixel_minmax", "channel_minmax"):
        with pytest.raises(_lib.HipExtensionError, match="triples"):
            mil_ops.tencrop_normalize_u8(fd, 4, 32, clip_stride=3, normalize=spec)
        with pytest.raises(_lib.HipExtensionError, match="triples"):
            ops.tencrop_planes_u8(fd, 0, 2, 4, 32, clip_stride=3, normalize=spec)
    with pytest.raises(ValueError, match="three entries"):
        ops.resolve_normalize(("standardize", (1.0, 2.0, 3.0, 4.0), 1.0))
