"""Crop subsets of TenCrop (crops=) on the uint8-frames path -- run with -m gpu.

The yardstick is never the subset code: it is the existing ten-crop call on the same frames.
  * pixel passes are elementwise: row q * nc + j of the subset call == row q * 10 + crops[j] of the ten-crop call;
  * a stem / backbone launch of `count` rows from subset row f: row i holds (clip q, crop c), and its yardstick is row i of the
    ten-crop call with first' = 10 q + c - i and the same count -- the same kernel, launch shape and position in the launch,
    only the addresses differ.  For an ascending set first' is always in range (asserted in `yardstick_rows`).
Every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

from anomaly_detection_on_video_amd.weights import synth_tensor

pytestmark = pytest.mark.gpu

TEN = tuple(range(10))
CROP_SETS = [(4,), (4, 9), (0, 1, 2, 3, 4), (5, 6, 7, 8, 9), (0, 3, 5, 9), TEN]


def _dev():
    return torch.device("cuda:0")


def _frames(seed, shape):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=shape, dtype=np.uint8)
    f[0, :3, :5] = 0
    f[-1, -3:, -5:] = 255
    return f


def subset_rows(n_clips, crops):
    """Ten-crop row of every subset row, in subset order."""
    return [q * 10 + c for q in range(n_clips) for c in crops]


def yardstick_rows(call_ten, n_clips, crops, first, count):
    """Rows [first, first + count) of a subset launch, each computed by the TEN-crop call `call_ten(first', count)` at the same
    position i of a launch of the same size."""
    nc = len(crops)
    assert 0 <= first and count > 0 and first + count <= n_clips * nc
    cache, rows = {}, []
    for i in range(count):
        q, c = divmod(first + i, nc)
        fp = 10 * q + crops[c] - i
        assert 0 <= fp and fp + count <= 10 * n_clips, (crops, first, count, i)
        if fp not in cache:
            cache[fp] = call_ten(fp, count)
        rows.append(cache[fp][i])
    return torch.stack(rows)


@pytest.fixture(params=["taps", "bytes", "planes"])
def form(request, monkeypatch):
    from anomaly_detection_on_video_amd import ops

    monkeypatch.setattr(ops, "U8_STEM_FORM", request.param)
    return request.param


def _stem(name="u8stem"):
    from anomaly_detection_on_video_amd import ops

    dev = _dev()
    k, s, p = (5, 7, 7), (2, 2, 2), (2, 3, 3)
    wt = synth_tensor(f"{name}.w", (64, 3) + k, scale=float(np.sqrt(6.0 / (3 * 5 * 7 * 7))))
    g = synth_tensor(f"{name}.g", (64,), scale=0.5, offset=1.0)
    be = synth_tensor(f"{name}.b", (64,), scale=0.25)
    mu = synth_tensor(f"{name}.m", (64,), scale=0.25)
    var = synth_tensor(f"{name}.v", (64,), scale=0.5, offset=1.0)
    return ops.pack_conv(wt.to(dev), g.to(dev), be.to(dev), mu.to(dev), var.to(dev), 1e-5, s, p, name=name)


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


# ---- 1. both passes, small and odd ---------------------------------------------------------------------------------------------
_TEN_PASS = {}


def _ten_pass(F, s):
    """The existing ten-crop passes (dense and planes) on the test's frames, computed once per (F, stride), left unchanged."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    if (F, s) not in _TEN_PASS:
        frames = _frames(F * 100 + s, (F, 37, 53, 3))  # margins 5 and 21: the centre offsets 2.5 and 10.5 round half to even
        fd = torch.from_numpy(frames).to(_dev())
        n = ops.n_windows(F, 16, s)
        _TEN_PASS[(F, s)] = (fd, mil_ops.tencrop_normalize_u8(fd, 16, 32, clip_stride=s), ops.tencrop_planes_u8(fd, 0, n * 10, 16, 32, clip_stride=s))
    return _TEN_PASS[(F, s)]


@pytest.mark.parametrize("s", [16, 8])
@pytest.mark.parametrize("F", [16, 17, 40])
@pytest.mark.parametrize("crops", CROP_SETS, ids=lambda c: "c" + "".join(map(str, c)))
def test_both_passes_equal_the_ten_crop_rows(crops, F, s):
    """Frames 37 x 53 (width no multiple of 4), crop 32: the dense pass over all rows, the planes pass over a range that starts
    and ends inside a clip's crops (where the set has more than one), a range one past the end refused."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    fpc, crop, nc = 16, 32, len(crops)
    fd, ten, ten_planes = _ten_pass(F, s)
    n = ops.n_windows(F, fpc, s)
    rows = subset_rows(n, crops)
    got = mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=s, crops=crops)
    assert got.shape == (n * nc, 3, fpc, crop, crop)
    assert torch.equal(got, ten[rows])
    first, count = (1, n * nc - 2) if n * nc >= 4 else (0, n * nc)
    planes = ops.tencrop_planes_u8(fd, first, count, fpc, crop, clip_stride=s, crops=crops)
    assert planes.shape == (count, 3, fpc, crop, 2, crop // 2 + 4)
    assert torch.equal(planes, ten_planes[rows[first : first + count]])
    with pytest.raises(ValueError):
        ops.tencrop_planes_u8(fd, first, n * nc - first + 1, fpc, crop, clip_stride=s, crops=crops)  # one past the end


@pytest.mark.parametrize("bad", [(4, 4), (9, 4), (10,), ()])
def test_passes_refuse_a_malformed_set(bad):
    from anomaly_detection_on_video_amd import mil_ops, ops

    fd = _ten_pass(16, 16)[0]
    with pytest.raises(ValueError):
        mil_ops.tencrop_normalize_u8(fd, 16, 32, crops=bad)
    with pytest.raises(ValueError):
        ops.tencrop_planes_u8(fd, 0, 1, 16, 32, crops=bad)
    with pytest.raises(ValueError):
        ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, _stem(), 0, 1, 16, 32, crops=bad)
    with pytest.raises(ValueError):
        _model().forward_frames(fd, 0, 1, 16, 32, crops=bad)


# ---- 2. reference geometry -----------------------------------------------------------------------------------------------------
def test_passes_at_the_reference_geometry_vs_oracle():
    """256 x 340 frames, crop 224, 17 frames (two clips, the second LoopPad-ed): the subset rows == the matching columns of
    oracle.host_oracle.ten_crop_clips (numpy restatement of TenCropVideoFrameDataset), array_equal."""
    from anomaly_detection_on_video_amd import mil_ops, ops
    from oracle import host_oracle

    fpc, crop = 16, 224
    frames = _frames(17000, (17, 256, 340, 3))
    fd = torch.from_numpy(frames).to(_dev())
    oracle = host_oracle.ten_crop_clips(frames)
    assert oracle.shape == (2, 10, 3, fpc, crop, crop)
    for crops in [(4,), (0, 3, 5, 9)]:
        nc = len(crops)
        got = mil_ops.tencrop_normalize_u8(fd, fpc, crop, crops=crops)
        assert got.shape == (2 * nc, 3, fpc, crop, crop)
        assert np.array_equal(got.cpu().numpy().reshape(2, nc, 3, fpc, crop, crop), oracle[:, list(crops)])
        planes = ops.tencrop_planes_u8(fd, 0, 2 * nc, fpc, crop, crops=crops)
        # the planes hold the same pixels: column 2 j + par of the crop at [par][2 + j], zero padding around
        cols = planes[..., 2 : 2 + crop // 2].transpose(-1, -2).reshape(2 * nc, 3, fpc, crop, crop)
        assert torch.equal(cols, got)
        assert not planes[..., :2].any() and not planes[..., 2 + crop // 2 :].any()


# ---- 3. the fused stem in each ADV_U8_STEM form --------------------------------------------------------------------------------
def test_stem_subset_rows_equal_the_ten_crop_call(form):
    """The fused uint8 stem in each form (the stem entry point runs the whole-pixel kernel under "planes"): every crop set over
    the whole range, a range cut inside a clip's crops and the last row alone; stride 8 on pad_windows_u8 frames for (4, 9);
    the identity set through the argument == the call without it."""
    from anomaly_detection_on_video_amd import ops

    pc = _stem()
    fpc, crop, F = 16, 32, 37
    frames = _frames(51, (F, 40, 52, 3))
    fd = ops.pad_windows_u8(torch.from_numpy(frames).to(_dev()), fpc, fpc)
    n = ops.n_windows(F, fpc)
    assert n == 3 and fd.shape[0] == n * fpc
    ten = lambda fp, count: ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, fp, count, fpc, crop)
    for crops in CROP_SETS:
        nc = len(crops)
        total = n * nc
        ranges = [(0, total), (total - 1, 1)]
        if total >= 4:
            ranges.append((1, total - 2))
        for first, count in ranges:
            got = ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, first, count, fpc, crop, crops=crops)
            assert torch.equal(got, yardstick_rows(ten, n, crops, first, count)), (form, crops, first, count)
        with pytest.raises(ValueError):
            ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, total - 1, 2, fpc, crop, crops=crops)  # one past the end
    want = ten(2, 15)
    assert torch.equal(ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, fpc, crop, crops=TEN), want)
    assert torch.equal(ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, fpc, crop, crops="ten"), want)
    assert torch.equal(ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, fpc, crop, crops=None), want)
    # overlapping windows: 37 frames at stride 8 = 4 windows, the last LoopPad-ed
    s, crops = 8, (4, 9)
    f8 = ops.pad_windows_u8(torch.from_numpy(frames).to(_dev()), fpc, s)
    n8 = ops.n_windows(F, fpc, s)
    assert n8 == 4 and f8.shape[0] == (n8 - 1) * s + fpc
    ten8 = lambda fp, count: ops.conv3d_u8_tencrop_bn_relu_maxpool233(f8, pc, fp, count, fpc, crop, clip_stride=s)
    for first, count in [(0, 8), (1, 6), (7, 1)]:
        got = ops.conv3d_u8_tencrop_bn_relu_maxpool233(f8, pc, first, count, fpc, crop, clip_stride=s, crops=crops)
        assert torch.equal(got, yardstick_rows(ten8, n8, crops, first, count)), (form, first, count)
    with pytest.raises(ValueError):
        ops.conv3d_u8_tencrop_bn_relu_maxpool233(f8, pc, 7, 2, fpc, crop, clip_stride=s, crops=crops)


# ---- 4. forward_frames, whole backbone -----------------------------------------------------------------------------------------
BACKBONE_CASES = [((4,), 0, 3), ((4, 9), 1, 5), ("five", 0, 15)]


def test_forward_frames_subset_rows_whole_backbone(form):
    """I3Res50.forward_frames(crops=C): every row == the row at the same position of a ten-crop forward_frames of the same
    count, in every stem form and on the separate-pass fallback; in the planes form also == forward_single of the dense pass's
    rows (one stream); ranges outside n_windows * nc raise."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    m = _model()
    fpc, crop, F = 16, 64, 37
    frames = _frames(71, (F, 72, 90, 3))
    fd = ops.pad_windows_u8(torch.from_numpy(frames).to(_dev()), fpc, fpc)
    n = 3
    assert m.frames_fused()
    ten = lambda fp, count: m.forward_frames(fd, fp, count, fpc, crop)
    for crops, first, count in BACKBONE_CASES:
        idx = ops.resolve_crops(crops)
        got = m.forward_frames(fd, first, count, fpc, crop, crops=crops)
        assert got.shape == (count, 2048, 1, 1, 1)
        assert torch.equal(got, yardstick_rows(ten, n, idx, first, count)), (form, crops)
        if form == "planes":
            try:
                m.streams = 1
                rows = subset_rows(n, idx)[first : first + count]
                dense = mil_ops.tencrop_normalize_u8(fd, fpc, crop)[rows]
                assert torch.equal(m.forward_frames(fd, first, count, fpc, crop, crops=crops), m.forward_single(dense)), crops
            finally:
                m.streams = 2
    for crops, first, count in [((4,), 1, 3), ((4, 9), 6, 1), ("five", 15, 1), ((4,), -1, 2), ((4, 9), 0, 0)]:
        with pytest.raises(ValueError):
            m.forward_frames(fd, first, count, fpc, crop, crops=crops)
    try:
        m.fuse_pool = False
        assert not m.frames_fused()
        short = torch.from_numpy(frames).to(_dev())  # the separate pass LoopPads by index: no appended frames needed
        ten_sep = lambda fp, count: m.forward_frames(short, fp, count, fpc, crop)
        for crops, first, count in BACKBONE_CASES:
            idx = ops.resolve_crops(crops)
            got = m.forward_frames(short, first, count, fpc, crop, crops=crops)
            assert torch.equal(got, yardstick_rows(ten_sep, n, idx, first, count)), ("fallback", crops)
        with pytest.raises(ValueError):
            m.forward_frames(short, 2, 2, fpc, crop, crops=(4,))
    finally:
        m.fuse_pool = True


# ---- 5. extract_video_frames ---------------------------------------------------------------------------------------------------
def _assemble(m, fr_dev_steps, crops, fpc, crop, max_cc=32):
    """What extract_video_frames must return, put together from forward_frames rows with the same step cuts."""
    nc = len(crops)
    rows = []
    for fr, n_clips in fr_dev_steps:
        n = n_clips * nc
        for i in range(0, n, max_cc):
            rows.append(m.forward_frames(fr, i, min(max_cc, n - i), fpc, crop, crops=crops).reshape(-1, 2048))
    return torch.cat(rows).reshape(-1, nc, 2048).cpu().numpy()


def test_extract_video_frames_center_crop():
    """crops="center", clips_per_step=3 on 53 frames (4 clips, the last 5 frames long: steps of 3 and 1 clips): (4, 1, 2048), not
    squeezed, == forward_frames rows put together by the test with the same step cuts -- from host frames, from device frames,
    and with resize=256 from decoded 240 x 320 frames."""
    from anomaly_detection_on_video_amd import ops, resize as resize_mod
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    fpc, crop, F = 16, 64, 53
    frames = _frames(93, (F, 72, 90, 3))
    fd = torch.from_numpy(frames).to(_dev())
    want = _assemble(m, [(ops.pad_windows_u8(fd[:48], fpc), 3), (ops.pad_windows_u8(fd[48:], fpc), 1)], (4,), fpc, crop)
    assert want.shape == (4, 1, 2048)
    for src in (torch.from_numpy(frames), fd):
        got = extract_video_frames(m, src, crop=crop, clips_per_step=3, crops="center")
        assert got.shape == (4, 1, 2048) and got.dtype == np.float32
        assert np.array_equal(got, want)
    decoded = _frames(94, (40, 240, 320, 3))  # 3 clips, one step
    dd = torch.from_numpy(decoded).to(_dev())
    want_r = _assemble(m, [(ops.pad_windows_u8(resize_mod.resize_u8(dd, 256, "bilinear"), fpc), 3)], (4,), fpc, 224)
    assert want_r.shape == (3, 1, 2048)
    for src in (torch.from_numpy(decoded), dd):
        got = extract_video_frames(m, src, resize=256, clips_per_step=3, crops="center")
        assert got.shape == (3, 1, 2048) and np.array_equal(got, want_r)
    # one clip: a subset keeps its axes (the ten-crop call keeps the reference's squeeze, below)
    assert extract_video_frames(m, fd[:16], crop=crop, crops=(4, 9)).shape == (1, 2, 2048)
    with pytest.raises(ValueError):
        extract_video_frames(m, fd, crop=crop, crops=(9, 4))


def test_extract_video_frames_ten_is_the_call_without_the_argument():
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    frames = torch.from_numpy(_frames(93, (53, 72, 90, 3)))
    plain = extract_video_frames(m, frames, crop=64)
    assert plain.shape == (4, 10, 2048)
    for crops in (None, "ten", TEN):
        assert np.array_equal(extract_video_frames(m, frames, crop=64, crops=crops), plain)
    one = extract_video_frames(m, frames[:16], crop=64)
    assert one.shape == (10, 2048)  # np.squeeze, as the reference
    for crops in (None, "ten", TEN):
        got = extract_video_frames(m, frames[:16], crop=64, crops=crops)
        assert got.shape == one.shape and np.array_equal(got, one)


def test_default_clips_per_step_follows_the_crop_count(monkeypatch):
    """No explicit clips_per_step: 3 for the ten crops, max(1, 30 // nc) for a subset (a step still launches about 30
    crop-clips) -- seen through the frames and the `count` that forward_frames is handed per step."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    calls = []
    real = m.forward_frames

    def spy(frames, first, count, *a, **kw):
        calls.append((frames.shape[0] // 16, first, count))
        return real(frames, first, count, *a, **kw)

    monkeypatch.setattr(m, "forward_frames", spy)
    frames = torch.from_numpy(_frames(96, (16 * 31, 72, 90, 3))).to(_dev())  # 31 clips
    cases = [  # (crops, clips_per_step passed, clips used, the (clips, first, count) of every step)
        ("five", None, 7, [(6, 0, 30), (1, 0, 5)]),
        ("center", None, 31, [(30, 0, 30), (1, 0, 1)]),
        ("center", 3, 7, [(3, 0, 3), (3, 0, 3), (1, 0, 1)]),
        ("center_flip", None, 16, [(15, 0, 30), (1, 0, 2)]),
        (None, None, 7, [(3, 0, 30), (3, 0, 30), (1, 0, 10)]),
        ("ten", None, 4, [(3, 0, 30), (1, 0, 10)]),
    ]
    for crops, passed, n_clips, want in cases:
        calls.clear()
        kw = {} if passed is None else {"clips_per_step": passed}
        extract_video_frames(m, frames[: 16 * n_clips], crop=64, crops=crops, **kw)
        assert calls == want, (crops, passed, calls)


# ---- 6. segment cache and names ------------------------------------------------------------------------------------------------
def test_long_video_segment_cache_and_names_carry_the_crop_set(tmp_path):
    """F = 117 at stride 8 with crops (4, 9) through the segment cache (segments of 48 frames = 6 windows = two whole steps of
    3): stacked segments == the whole-video call, the second run reads only the cache, another crop set reads none of the
    cached files, and runs without a subset keep the reference's names."""
    from anomaly_detection_on_video_amd import extract

    m = _model()
    F, s, crops = 117, 8, (4, 9)
    frames = torch.from_numpy(_frames(92, (F, 72, 90, 3)))
    reads = []

    def read(lo, hi):
        reads.append((lo, hi))
        return frames[lo:hi]

    out = str(tmp_path / "feat")
    whole = extract.extract_video_frames(m, frames, crop=64, clip_stride=s, crops=crops, clips_per_step=3)
    n = extract.n_windows(F, 16, s)
    assert whole.shape == (n, 2, 2048) and n == 14
    run = lambda **kw: extract.extract_frames([("vid", F, read)], m, out, long_video_frames=32, seg_len=48, crop=64, **kw)
    written = run(clip_stride=s, crops=crops, clips_per_step=3)
    assert written["vid"].endswith("vid_i3d_s8_c49.npy")
    assert np.array_equal(np.load(written["vid"]), whole)
    assert reads == [(0, 56), (48, 104), (96, 117)]
    seg_files = ["vid_s8_c49_0.npy", "vid_s8_c49_1.npy", "vid_s8_c49_2.npy"]
    assert sorted(os.listdir(os.path.join(out, "vid"))) == seg_files
    assert np.load(os.path.join(out, "vid", seg_files[0])).shape == (6, 2, 2048)
    # second run: the final file is gone, every segment comes from its cache
    os.remove(written["vid"])
    reads.clear()
    again = run(clip_stride=s, crops=crops, clips_per_step=3)
    assert reads == [] and np.array_equal(np.load(again["vid"]), whole)
    assert run(clip_stride=s, crops=crops, clips_per_step=3) == {}  # skip-if-exists
    # another crop set at the same stride: its own files, nothing cached is read
    reads.clear()
    centre = run(clip_stride=s, crops="center")
    assert centre["vid"].endswith("vid_i3d_s8_c4.npy") and reads == [(0, 56), (48, 104), (96, 117)]
    assert np.load(centre["vid"]).shape == (n, 1, 2048)
    assert np.array_equal(np.load(centre["vid"])[:6], np.load(os.path.join(out, "vid", "vid_s8_c4_0.npy")))
    # the same set at the clip length: no stride tag
    reads.clear()
    back = run(crops=crops)
    assert back["vid"].endswith("vid_i3d_c49.npy") and reads == [(0, 48), (48, 96), (96, 117)]
    assert np.load(back["vid"]).shape == (8, 2, 2048)
    # without a subset: the reference's names, whatever else lies in the folder
    reads.clear()
    ref = run()
    assert ref["vid"].endswith("vid_i3d.npy") and reads == [(0, 48), (48, 96), (96, 117)] and np.load(ref["vid"]).shape == (8, 10, 2048)
    names = sorted(os.listdir(os.path.join(out, "vid")))
    assert names == sorted(seg_files + [f"vid_s8_c4_{i}.npy" for i in range(3)] + [f"vid_c49_{i}.npy" for i in range(3)] +
                           [f"vid_{i}.npy" for i in range(3)])
    assert sorted(f for f in os.listdir(out) if f.endswith(".npy")) == ["vid_i3d.npy", "vid_i3d_c49.npy", "vid_i3d_s8_c4.npy", "vid_i3d_s8_c49.npy"]


# ---- 7. one ExtractScoreStream step --------------------------------------------------------------------------------------------
def test_stream_step_from_a_crop_subset():
    """One ExtractScoreStream step of a 3-clip video fed FrameCrops(..., crops=(4, 9)) into a stream built with ncrops = 2: the
    gathered rows are forward_frames' rows, the video's scores are score_video of those rows; the set is part of the key."""
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
    from anomaly_detection_on_video_amd.pipeline import ExtractScoreStream, FrameCrops
    from anomaly_detection_on_video_amd.weights import synth_module_state_dict

    dev = _dev()
    sc = MGFNForVideoAnomalyDetection(MGFNConfig())
    sc.load_state_dict(synth_module_state_dict(sc))
    sc = sc.eval().to(dev)
    m = _model()
    fpc, crops = 16, (4, 9)
    frames = _frames(97, (48, 72, 90, 3))
    host = torch.from_numpy(frames).pin_memory()
    st = ExtractScoreStream(m, sc, clips_per_video=3, ncrops=2, local_batch=6)
    h = st.step_async(host, prepare=lambda x: FrameCrops(x.to(dev, non_blocking=True), 0, 6, fpc, 64, crops=crops))
    st.drain()
    torch.cuda.synchronize()
    gathered, scored = h.result()
    try:
        m.streams = 1  # (the stream runs whole-batch launches per lane)
        want = m.forward_frames(torch.from_numpy(frames).to(dev), 0, 6, fpc, 64, crops=crops).reshape(6, -1)
    finally:
        m.streams = 2
    assert gathered.shape == (6, 2048) and torch.equal(gathered, want)
    assert [v for v, _ in scored] == [0] and scored[0][1].shape == (3,)
    assert torch.equal(scored[0][1], st.score_video(want.view(3, 2, 2048)))
    fd = torch.from_numpy(frames)
    assert FrameCrops(fd, 0, 6, fpc, 64, crops=crops).key() != FrameCrops(fd, 0, 6, fpc, 64, crops=(0, 9)).key()
    assert FrameCrops(fd, 0, 6, fpc, 64, crops=crops).key() != FrameCrops(fd, 0, 6, fpc, 64).key()
    assert FrameCrops(fd, 0, 6, fpc, 64, crops=None).key() == FrameCrops(fd, 0, 6, fpc, 64).key() == ("u8", 6, (72, 90), fpc, 64, fpc)
    with pytest.raises(ValueError):
        FrameCrops(fd, 0, 6, fpc, 64, crops=(4, 4))
