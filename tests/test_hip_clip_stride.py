"""Overlapping clip windows (clip_stride) on the device -- run with -m gpu.

The yardstick is never the strided code: it is the existing back-to-back path run on windows this file materialises itself
(`frames[w * s : w * s + fpc]`, the last one LoopPad-ed by index, src/gtransforms.py:119-132), and
oracle.host_oracle.ten_crop_clips for the pixels.  Same kernels, same K order, same launch shapes: every comparison is bit for bit."""
import os

import numpy as np
import pytest
import torch

from anomaly_detection_on_video_amd.weights import synth_tensor

pytestmark = pytest.mark.gpu

STRIDES = [1, 3, 8, 16]
LENGTHS = [16, 17, 31, 40]


def _dev():
    return torch.device("cuda:0")


def _frames(seed, shape):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=shape, dtype=np.uint8)
    f[0, :3, :5] = 0
    f[-1, -3:, -5:] = 255
    return f


def window_indices(F, fpc, s):
    """Frame indices of every window: the smallest n with (n - 1) * s + fpc >= F, window w = frames w * s + t % len_w."""
    n = 1
    while (n - 1) * s + fpc < F:
        n += 1
    out = []
    for w in range(n):
        length = min(fpc, F - w * s)
        assert length == fpc or w == n - 1
        out.append([w * s + t % length for t in range(fpc)])
    return out


def materialise(frames, fpc, s):
    """The video a user builds today: every window's frames, one after the other (n * fpc frames)."""
    idx = np.concatenate(window_indices(frames.shape[0], fpc, s))
    return frames[idx]


def frame_scores_np(scores, fpc, s, n_frames=None):
    x = np.asarray(scores, dtype=np.float32)
    n = x.size
    nf = (n - 1) * s + fpc if n_frames is None else n_frames
    out = np.empty((nf,), dtype=np.float32)
    for f in range(nf):
        ws = [w for w in range(n) if w * s <= f < w * s + fpc]
        acc = x[ws[0]]
        for w in ws[1:]:
            acc = np.float32(acc + x[w])
        out[f] = np.float32(acc / np.float32(len(ws)))
    return out


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


@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("F", LENGTHS)
def test_tencrop_passes_equal_the_existing_pass_per_window(F, s):
    """Both TenCrop passes (dense and column-parity planes) over overlapping windows == the existing pass on each materialised
    window; small frames with odd margins, and a planes range that starts and ends in the middle of a window's ten crops."""
    from anomaly_detection_on_video_amd import mil_ops, ops

    fpc, crop = 16, 32
    frames = _frames(F * 100 + s, (F, 37, 53, 3))
    fd = torch.from_numpy(frames).to(_dev())
    wins = window_indices(F, fpc, s)
    n = len(wins)
    assert ops.n_windows(F, fpc, s) == n
    got = mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=s)
    assert got.shape == (n * 10, 3, fpc, crop, crop)
    for w, idx in enumerate(wins):
        wd = torch.from_numpy(frames[idx]).to(_dev())
        assert torch.equal(got[w * 10 : (w + 1) * 10], mil_ops.tencrop_normalize_u8(wd, fpc, crop)), (F, s, w)
    mat = torch.from_numpy(materialise(frames, fpc, s)).to(_dev())
    first, count = (3, n * 10 - 7) if n > 1 else (3, 5)
    planes = ops.tencrop_planes_u8(fd, first, count, fpc, crop, clip_stride=s)
    assert torch.equal(planes, ops.tencrop_planes_u8(mat, first, count, fpc, crop))
    with pytest.raises(ValueError):
        ops.tencrop_planes_u8(fd, first, n * 10 - first + 1, fpc, crop, clip_stride=s)
    with pytest.raises(ValueError):
        mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=fpc + 1)
    with pytest.raises(ValueError):
        mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=0)


@pytest.mark.parametrize("s", STRIDES)
@pytest.mark.parametrize("F", LENGTHS)
def test_tencrop_passes_at_the_reference_geometry_vs_oracle(F, s):
    """256 x 340 frames, crop 224: every window of both passes == oracle.host_oracle.ten_crop_clips of the materialised window
    (numpy restatement of TenCropVideoFrameDataset), array_equal, and == the existing pass on it."""
    from anomaly_detection_on_video_amd import mil_ops, ops
    from oracle import host_oracle

    fpc, crop = 16, 224
    frames = _frames(F * 1000 + s, (F, 256, 340, 3))
    fd = torch.from_numpy(frames).to(_dev())
    wins = window_indices(F, fpc, s)
    n = len(wins)
    got = mil_ops.tencrop_normalize_u8(fd, fpc, crop, clip_stride=s)
    assert got.shape == (n * 10, 3, fpc, crop, crop)
    for w, idx in enumerate(wins):
        want = host_oracle.ten_crop_clips(frames[idx], fpc, crop)
        assert want.shape == (1, 10, 3, fpc, crop, crop)
        assert np.array_equal(got[w * 10 : (w + 1) * 10].cpu().numpy(), want[0]), (F, s, w)
        wd = torch.from_numpy(frames[idx]).to(_dev())
        assert torch.equal(got[w * 10 : (w + 1) * 10], mil_ops.tencrop_normalize_u8(wd, fpc, crop))
        planes = ops.tencrop_planes_u8(fd, w * 10, 10, fpc, crop, clip_stride=s)
        assert torch.equal(planes, ops.tencrop_planes_u8(wd, 0, 10, fpc, crop))
        # the planes hold the same pixels: column 2 j + par of the crop at [par][2 + j], zero padding around
        cols = planes[..., 2 : 2 + crop // 2].transpose(-1, -2).reshape(10, 3, fpc, crop, crop)
        assert torch.equal(cols, got[w * 10 : (w + 1) * 10])


@pytest.mark.parametrize("s", [1, 3, 8])
def test_stem_over_windows_equals_the_stem_on_materialised_windows(form, s):
    """The fused uint8 stem in each ADV_U8_STEM form (the stem entry point runs the whole-pixel kernel under "planes"): ranges
    that start and end inside a window's ten crops, a LoopPad-ed last window, and refusals."""
    from anomaly_detection_on_video_amd import ops

    pc = _stem()
    fpc, crop, F = 16, 32, 37
    frames = _frames(50 + s, (F, 40, 52, 3))
    fd = ops.pad_windows_u8(torch.from_numpy(frames).to(_dev()), fpc, s)
    wins = window_indices(F, fpc, s)
    n = len(wins)
    assert fd.shape[0] == (n - 1) * s + fpc
    assert np.array_equal(fd.cpu().numpy()[(n - 1) * s :], frames[wins[-1]])  # the appended frames are the last window's LoopPad
    mat = torch.from_numpy(materialise(frames, fpc, s)).to(_dev())
    for first, count in [(0, n * 10), (7, 11), (n * 10 - 13, 13), (13, 1)]:
        got = ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, first, count, fpc, crop, clip_stride=s)
        want = ops.conv3d_u8_tencrop_bn_relu_maxpool233(mat, pc, first, count, fpc, crop)
        assert torch.equal(got, want), (form, s, first, count)
    with pytest.raises(ValueError):
        ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, n * 10 - 3, 4, fpc, crop, clip_stride=s)  # past the last window
    with pytest.raises(ValueError):
        ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, -1, 4, fpc, crop, clip_stride=s)
    with pytest.raises(ValueError):
        ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 0, 4, fpc, crop, clip_stride=fpc + 1)
    if s > 1:
        with pytest.raises(ValueError):
            ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd[:-1], pc, 0, 4, fpc, crop, clip_stride=s)  # not whole windows


def test_stem_at_the_clip_length_is_the_existing_call(form):
    from anomaly_detection_on_video_amd import ops

    pc = _stem()
    fd = torch.from_numpy(_frames(5, (16, 40, 52, 3))).to(_dev())
    want = ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, 8, 32)
    assert torch.equal(ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, 8, 32, clip_stride=8), want)
    assert torch.equal(ops.conv3d_u8_tencrop_bn_relu_maxpool233(fd, pc, 2, 15, 8, 32, clip_stride=None), want)


@pytest.mark.parametrize("s", [3, 8])
def test_forward_frames_over_windows_whole_backbone(form, s):
    """I3Res50.forward_frames(clip_stride=s) == forward_frames on the materialised windows for the same [first, first + count)
    (same launch shapes), in every stem form and on the separate-pass fallback; ranges outside n_windows * 10 raise."""
    from anomaly_detection_on_video_amd import ops

    m = _model()
    fpc, crop, F = 16, 64, 37
    frames = _frames(70 + s, (F, 72, 90, 3))
    fd = ops.pad_windows_u8(torch.from_numpy(frames).to(_dev()), fpc, s)
    n = len(window_indices(F, fpc, s))
    mat = torch.from_numpy(materialise(frames, fpc, s)).to(_dev())
    assert m.frames_fused()
    for first, count in [(4, 23), (n * 10 - 9, 9)]:
        got = m.forward_frames(fd, first, count, fpc, crop, clip_stride=s)
        assert got.shape == (count, 2048, 1, 1, 1)
        assert torch.equal(got, m.forward_frames(mat, first, count, fpc, crop)), (form, s, first, count)
    for first, count in [(n * 10 - 3, 4), (-1, 3), (0, 0)]:
        with pytest.raises(ValueError):
            m.forward_frames(fd, first, count, fpc, crop, clip_stride=s)
    try:
        m.fuse_pool = False
        assert not m.frames_fused()
        short = torch.from_numpy(frames).to(_dev())  # the separate pass LoopPads by index: no appended frames needed
        assert torch.equal(m.forward_frames(short, 6, 17, fpc, crop, clip_stride=s), m.forward_frames(mat, 6, 17, fpc, crop))
        with pytest.raises(ValueError):
            m.forward_frames(short, n * 10 - 3, 4, fpc, crop, clip_stride=s)
    finally:
        m.fuse_pool = True


@pytest.mark.parametrize("fuse_pool", [True, False])
def test_extract_video_frames_with_a_stride(fuse_pool):
    """extract_video_frames(clip_stride=8) from host frames, from device frames and with resize=256 from decoded 240 x 320
    frames == the existing function on the materialised video; clip_stride = 16 / None == the call without the argument."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    try:
        m.fuse_pool = fuse_pool
        assert m.frames_fused() == fuse_pool
        fpc, s, F = 16, 8, 53  # 6 windows, the last 13 frames long: two steps of three windows
        frames = _frames(90, (F, 72, 90, 3))
        mat = materialise(frames, fpc, s)
        assert mat.shape[0] == 6 * fpc
        want = extract_video_frames(m, torch.from_numpy(mat), crop=64)
        assert want.shape == (6, 10, 2048)
        assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames), crop=64, clip_stride=s), want)
        assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames).to(_dev()), crop=64, clip_stride=s), want)
        plain = extract_video_frames(m, torch.from_numpy(frames), crop=64)
        assert plain.shape == (4, 10, 2048)
        assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames), crop=64, clip_stride=16), plain)
        assert np.array_equal(extract_video_frames(m, torch.from_numpy(frames), crop=64, clip_stride=None), plain)
        with pytest.raises(ValueError):
            extract_video_frames(m, torch.from_numpy(frames), crop=64, clip_stride=17)
        if fuse_pool:  # decoded frames, resized on the device per step (the overlap frames twice: the same bytes)
            decoded = _frames(91, (40, 240, 320, 3))
            dmat = materialise(decoded, fpc, s)
            want_r = extract_video_frames(m, torch.from_numpy(dmat), resize=256)
            assert want_r.shape == (4, 10, 2048)
            assert np.array_equal(extract_video_frames(m, torch.from_numpy(decoded), resize=256, clip_stride=s), want_r)
            assert np.array_equal(extract_video_frames(m, torch.from_numpy(decoded).to(_dev()), resize=256, clip_stride=s), want_r)
    finally:
        m.fuse_pool = True


def test_long_video_segments_own_their_windows_and_cache_per_stride(tmp_path):
    """A long video at stride 8 through the segment cache (segments of 48 frames = 6 windows = two whole steps of 3, so every
    launch has the whole-video run's shape): stacked segments == the whole-video result, the second run reads the cache, a
    run at another stride does not pick the files up, and the back-to-back names stay the reference's."""
    from anomaly_detection_on_video_amd import extract

    m = _model()
    F, s = 117, 8
    frames = torch.from_numpy(_frames(92, (F, 72, 90, 3)))
    reads = []

    def read(lo, hi):
        reads.append((lo, hi))
        return frames[lo:hi]

    out = str(tmp_path / "feat")
    whole = extract.extract_video_frames(m, frames, crop=64, clip_stride=s)
    n = extract.n_windows(F, 16, s)
    assert whole.shape == (n, 10, 2048) and n == 14
    run = lambda **kw: extract.extract_frames([("vid", F, read)], m, out, long_video_frames=32, seg_len=48, crop=64, **kw)
    written = run(clip_stride=s)
    assert written["vid"].endswith("vid_i3d_s8.npy")
    assert np.array_equal(np.load(written["vid"]), whole)
    assert reads == [(0, 56), (48, 104), (96, 117)]  # each segment reads fpc - s = 8 frames past its end
    assert sorted(os.listdir(os.path.join(out, "vid"))) == ["vid_s8_0.npy", "vid_s8_1.npy", "vid_s8_2.npy"]
    # second run: the final file is gone, every segment comes from its cache
    os.remove(written["vid"])
    reads.clear()
    again = run(clip_stride=s)
    assert reads == [] and np.array_equal(np.load(again["vid"]), whole)
    assert run(clip_stride=s) == {}  # skip-if-exists
    # another stride: its own files, nothing of stride 8 is read
    reads.clear()
    back = run()
    assert back["vid"].endswith("vid_i3d.npy") and reads == [(0, 48), (48, 96), (96, 117)]
    assert np.load(back["vid"]).shape == (8, 10, 2048)
    assert sorted(os.listdir(os.path.join(out, "vid"))) == ["vid_0.npy", "vid_1.npy", "vid_2.npy", "vid_s8_0.npy", "vid_s8_1.npy", "vid_s8_2.npy"]
    reads.clear()
    four = run(clip_stride=4)
    assert four["vid"].endswith("vid_i3d_s4.npy") and len(reads) == 3
    assert np.load(four["vid"]).shape == (extract.n_windows(F, 16, 4), 10, 2048)
    with pytest.raises(ValueError):
        extract.extract_long_video_frames(m, "other", F, read, out, seg_len=48, crop=64, clip_stride=5)


@pytest.mark.parametrize("s", STRIDES)
def test_frame_scores_kernel_equals_the_numpy_rule(s):
    from anomaly_detection_on_video_amd import mil_ops

    rng = np.random.default_rng(40 + s)
    for n in (1, 2, 7, 300):
        x = rng.random(n).astype(np.float32)
        xd = torch.from_numpy(x).to(_dev())
        covered = (n - 1) * s + 16
        got = mil_ops.frame_scores(xd, 16, s)
        assert got.shape == (covered,) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy(), frame_scores_np(x, 16, s))
        nf = covered - min(11, covered - 1)
        assert np.array_equal(mil_ops.frame_scores(xd, 16, s, nf).cpu().numpy(), frame_scores_np(x, 16, s, nf))
        if s == 16:
            assert np.array_equal(got.cpu().numpy(), np.repeat(x, 16))
            assert np.array_equal(mil_ops.frame_scores(xd).cpu().numpy(), np.repeat(x, 16))
        with pytest.raises(ValueError):
            mil_ops.frame_scores(xd, 16, s, covered + 1)
    with pytest.raises(ValueError):
        mil_ops.frame_scores(torch.zeros(4, device=_dev()), 16, 17)


def test_stream_step_from_strided_frames_equals_the_step_from_materialised_frames():
    """One ExtractScoreStream step fed FrameCrops(..., clip_stride=8) == the step fed the materialised frames, bit for bit; the
    stride is part of the table key."""
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
    from anomaly_detection_on_video_amd.pipeline import ExtractScoreStream, FrameCrops
    from anomaly_detection_on_video_amd.weights import synth_module_state_dict

    dev = _dev()
    sc = MGFNForVideoAnomalyDetection(MGFNConfig())
    sc.load_state_dict(synth_module_state_dict(sc))
    sc = sc.eval().to(dev)
    m = _model()
    fpc, s = 16, 8
    frames = _frames(95, (32, 72, 90, 3))  # 3 whole windows at stride 8
    mat = materialise(frames, fpc, s)
    fd, md = torch.from_numpy(frames).pin_memory(), torch.from_numpy(mat).pin_memory()
    a = ExtractScoreStream(m, sc, clips_per_video=3, ncrops=10, local_batch=20)
    ha = a.step_async(fd, prepare=lambda h: FrameCrops(h.to(dev, non_blocking=True), 7, 20, fpc, 64, clip_stride=s))
    a.drain()
    b = ExtractScoreStream(m, sc, clips_per_video=3, ncrops=10, local_batch=20)
    hb = b.step_async(md, prepare=lambda h: FrameCrops(h.to(dev, non_blocking=True), 7, 20, fpc, 64))
    b.drain()
    torch.cuda.synchronize()
    assert torch.equal(ha.result()[0], hb.result()[0])
    assert FrameCrops(md, 0, 10, fpc, 64).key() != FrameCrops(md, 0, 10, fpc, 64, clip_stride=s).key()
    assert FrameCrops(md, 0, 10, fpc, 64).key() == FrameCrops(md, 0, 10, fpc, 64, clip_stride=fpc).key()
    with pytest.raises(ValueError):
        FrameCrops(md, 0, 10, fpc, 64, clip_stride=0)
