"""GPU tests of the live frame rings (csrc/live.hip, mil_ops.frame_ring_push / frame_ring_windows, live.LiveFrames,
LiveScorer.step_camera_frames): ring, counts and windows byte for byte against the numpy model of tests/_live_frames_ref.py at
every access width, what must not be written, misaligned operands, push through resize_u8, the due tuple, reset, the whole path
from frames to scores against the offline windows of the same frames (equal, not close), the ATen audit of a steady-state step,
and every refusal."""
import itertools

import numpy as np
import pytest
import torch

from _live_frames_ref import FrameRingRef, scripted_counts, scripted_pushes, strides
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_module_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CAM = 6
FILL = 0xA5
# bytes one workgroup copies at access widths 1 / 4 / 16: FRAME_CHUNK = 256 lanes x 4 accesses of csrc/live.hip (mil_ops.FRAME_RING_CHUNK)
CHUNK = {1: 1024, 4: 4096, 16: 16384}
# (FH, FW): the issue's smallest frame of each width, and one per width that spans two chunks and ends inside the second
FRAMES = {(2, 3): 1, (2, 2): 4, (4, 4): 16, (7, 49): 1, (4, 343): 4, (16, 343): 16}
SAMPLING = [(1, 1), (4, 1), (1, 3), (4, 3)]  # (frames_per_clip, frame_step)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def test_the_frame_sizes_take_the_paths_they_are_meant_for():
    from anomaly_detection_on_video_amd import mil_ops

    assert all(v == k * mil_ops.FRAME_RING_CHUNK for k, v in CHUNK.items())
    for (fh, fw), width in FRAMES.items():
        fb = fh * fw * 3
        assert (16 if fb % 16 == 0 else 4 if fb % 4 == 0 else 1) == width, (fh, fw)
        if fb > 48:
            assert CHUNK[width] < fb < 2 * CHUNK[width] and fb % CHUNK[width], (fh, fw)


# ---- 1. push and windows: bytes only ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fpc,d", SAMPLING)
@pytest.mark.parametrize("hw", list(FRAMES))
def test_push_and_windows_byte_for_byte(hw, fpc, d):
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd.live import LiveFrames

    R, shape = fpc * d, hw + (3,)
    for s in strides(R):
        lf = LiveFrames(N_CAM, frame_hw=hw, frames_per_clip=fpc, frame_step=d, clip_stride=s, device=DEV)
        assert (lf.span, lf.clip_stride, lf.frame_step) == (R, s, d) and lf.ring.data_ptr() % 16 == 0
        ref = FrameRingRef(N_CAM, shape, fpc, d, s)
        for cams, frames in scripted_pushes(R, shape):  # (every step but the first few is a push to a subset)
            due = lf.push(cams, _dev(frames))
            assert due == ref.push(cams, frames), (s, cams)
            assert np.array_equal(_np(lf.ring), ref.ring), (s, cams)  # the pushed frames, and no byte of a camera outside the push
            assert lf.counts.tolist() == list(lf.counts_host) == ref.counts.tolist()
        assert ref.counts.tolist() == scripted_counts(R)
    full = [c for c in range(N_CAM) if ref.has_window(c)]
    assert len(full) >= 3
    ring_before = lf.ring.clone()
    for n in range(1, len(full) + 1):
        for sub in itertools.combinations(full, n):
            for cams in {sub, sub[::-1], sub[1:] + sub[:1]}:  # ascending, descending, rotated
                got = lf.windows(cams)
                assert tuple(got.shape) == (len(cams) * fpc,) + shape
                assert np.array_equal(_np(got), ref.windows(list(cams))), cams
                dst = torch.full_like(got, FILL)  # the launch alone, into a buffer of the caller's: the same bytes, twice
                for _ in range(2):
                    mil_ops.frame_ring_windows(lf.ring, lf.counts, _dev(np.array(cams, dtype=np.int32)), dst, fpc, d)
                    assert torch.equal(dst, got)
    assert torch.equal(lf.ring, ring_before)


# ---- 2. what must not be written ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fpc,d", [(4, 1), (4, 3)])
@pytest.mark.parametrize("hw", [(2, 3), (2, 2), (4, 4), (16, 343)])
def test_rows_without_a_window_and_bad_ids_write_nothing(hw, fpc, d):
    from anomaly_detection_on_video_amd import mil_ops

    R, shape = fpc * d, hw + (3,)
    ref = FrameRingRef(N_CAM, shape, fpc, d)
    ring = torch.zeros((N_CAM, R) + shape, dtype=torch.uint8, device=DEV)
    counts = torch.zeros((N_CAM,), dtype=torch.int64, device=DEV)
    for cams, frames in scripted_pushes(R, shape, seed=2):
        mil_ops.frame_ring_push(_dev(frames), _dev(np.array(cams, dtype=np.int32)), ring, counts)
        ref.push(cams, frames)
    assert np.array_equal(_np(ring), ref.ring) and counts.tolist() == scripted_counts(R)
    listed = [5, -1, 0, 3, 1, N_CAM, 2, 4]  # below span: 0, 1, 2; outside the range: -1, N_CAM
    dst = torch.full((len(listed) * fpc,) + shape, FILL, dtype=torch.uint8, device=DEV)
    mil_ops.frame_ring_windows(ring, counts, _dev(np.array(listed, dtype=np.int32)), dst, fpc, d)
    got, want = _np(dst), ref.windows(listed, fill=FILL)
    assert np.array_equal(got, want)
    for v, c in enumerate(listed):
        if not ref.has_window(c):
            assert (got[v * fpc:(v + 1) * fpc] == FILL).all(), c  # the pattern is still there
    ring_before, counts_before = ring.clone(), counts.clone()
    bad = _dev(np.array([-1, N_CAM], dtype=np.int32))
    mil_ops.frame_ring_push(torch.full((2,) + shape, 77, dtype=torch.uint8, device=DEV), bad, ring, counts)
    assert torch.equal(ring, ring_before) and torch.equal(counts, counts_before)
    # one good id beside a bad one: only the good camera's slot and count move
    mixed = _dev(np.array([N_CAM, 2], dtype=np.int32))
    frames = np.full((2,) + shape, 78, dtype=np.uint8)
    mil_ops.frame_ring_push(_dev(frames), mixed, ring, counts)
    ref.push([2], frames[1:])
    assert np.array_equal(_np(ring), ref.ring) and counts.tolist() == ref.counts.tolist()


# ---- 3. misaligned operands -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(4, 4), (16, 343)])
def test_misaligned_operands_take_the_narrower_path(hw):
    """The frame size allows 16-byte accesses; frames / dst one byte or four bytes into a larger buffer do not: the host picks
    single bytes / dwords, and the bytes are the aligned call's."""
    from anomaly_detection_on_video_amd import mil_ops

    fpc, d, shape = 4, 1, hw + (3,)
    fb = int(np.prod(shape))
    assert fb % 16 == 0
    ref = FrameRingRef(N_CAM, shape, fpc, d)
    steps = scripted_pushes(fpc * d, shape, seed=3)
    for cams, frames in steps:
        ref.push(cams, frames)
    listed = [5, 3, 4]
    ids = _dev(np.array(listed, dtype=np.int32))
    want = ref.windows(listed)
    for off in (0, 1, 4):
        ring = torch.zeros((N_CAM, fpc * d) + shape, dtype=torch.uint8, device=DEV)
        counts = torch.zeros((N_CAM,), dtype=torch.int64, device=DEV)
        for cams, frames in steps:
            buf = torch.full((off + frames.size + 16,), FILL, dtype=torch.uint8, device=DEV)
            view = buf[off: off + frames.size].view(frames.shape)
            view.copy_(_dev(frames))
            assert view.data_ptr() % 16 == (off if off else 0) and view.is_contiguous()
            mil_ops.frame_ring_push(view, _dev(np.array(cams, dtype=np.int32)), ring, counts)
        assert np.array_equal(_np(ring), ref.ring), off
        buf = torch.full((off + want.size + 16,), FILL, dtype=torch.uint8, device=DEV)
        dst = buf[off: off + want.size].view(want.shape)
        mil_ops.frame_ring_windows(ring, counts, ids, dst, fpc, d)
        assert np.array_equal(_np(dst), want), off
        assert bool((buf[:off] == FILL).all()) and bool((buf[off + want.size:] == FILL).all())  # guard bytes untouched


# ---- 4. push with resize ------------------------------------------------------------------------------------------------------------
def _push_resized(frame_hw, frames, **kw):
    """Two pushes of two cameras through resize_u8; every ring slot must hold resize_u8's bytes of its frame."""
    from anomaly_detection_on_video_amd import resize
    from anomaly_detection_on_video_amd.live import LiveFrames

    lf = LiveFrames(3, frame_hw=frame_hw, frames_per_clip=2, device=DEV)
    cams = [2, 0]
    for step in range(2):
        x = frames[2 * step: 2 * step + 2]
        want = resize.resize_u8(x if x.is_cuda else x.to(DEV), kw["resize"], kw.get("resample", "bilinear"), pixel_format=kw.get("pixel_format"),
                                surface=kw.get("surface"))
        assert tuple(want.shape) == (2,) + frame_hw + (3,)
        due = lf.push(cams, x, **kw)
        assert due == ((2, 0) if step == 1 else ())
        for i, c in enumerate(cams):
            assert torch.equal(lf.ring[c, step], want[i]), (step, c)
    assert not lf.ring[1].any() and lf.counts.tolist() == list(lf.counts_host) == [2, 0, 2]
    return lf


def test_push_with_resize_packed_rgb():
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.integers(0, 256, size=(4, 19, 23, 3), dtype=np.uint8))
    _push_resized((5, 61), x.to(DEV), resize=(5, 61), resample="bicubic")  # (a small case of tests/test_hip_resize.py)
    _push_resized((5, 61), x, resize=(5, 61), resample="bicubic")          # host frames: copied on the current stream
    y = torch.from_numpy(rng.integers(0, 256, size=(4, 45, 37, 3), dtype=np.uint8)).to(DEV)
    lf = _push_resized((77, 64), y, resize=64, resample="lanczos")          # an int: the short side
    before, counts = lf.ring.clone(), lf.counts_host
    with pytest.raises(HipExtensionError, match=r"LiveFrames.push: resize=\(5, 61\) of 45 x 37 frames gives \(5, 61\), the rings hold \(77, 64\) frames"):
        lf.push([0, 1], y[:2], resize=(5, 61))
    with pytest.raises(HipExtensionError, match=r"LiveFrames.push: resize=32 of 45 x 37 frames gives \(38, 32\), the rings hold \(77, 64\)"):
        lf.push([0, 1], y[:2], resize=32)
    with pytest.raises(HipExtensionError, match=r"LiveFrames.push: frames must be \(2, 77, 64, 3\) \(frames at ring size"):
        lf.push([0, 1], y[:2])
    assert torch.equal(lf.ring, before) and lf.counts_host == counts and lf.counts.tolist() == list(counts)  # a refused push moves nothing


def test_push_with_resize_nv12_and_pitched_surface():
    from anomaly_detection_on_video_amd import resize

    rng = np.random.default_rng(8)
    h, w = 38, 46
    nv12 = torch.from_numpy(rng.integers(0, 256, size=(4, 3 * h // 2, w), dtype=np.uint8)).to(DEV)
    _push_resized((16, 20), nv12, resize=(16, 20), pixel_format="nv12")
    sf = resize.surface("nv12", h, w, pitch=64, rows=40)
    surf = torch.from_numpy(rng.integers(0, 256, size=(4, 64 * 40 * 3 // 2 + 5), dtype=np.uint8)).to(DEV)
    _push_resized((16, 20), surf, resize=(16, 20), pixel_format=("nv12", "bt709"), surface=sf)
    _push_resized((h, w), surf, resize=(h, w), pixel_format="nv12", surface=sf)  # already at ring size: converted only


# ---- 5. the due tuple, counts_host, reset ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fpc,d,s", [(4, 1, 2), (2, 3, 4), (4, 1, 4)])
def test_due_tuple_and_counts_follow_the_model_at_different_rates(fpc, d, s):
    from anomaly_detection_on_video_amd.live import LiveFrames

    hw, n_cam = (4, 4), 4
    shape, R = hw + (3,), fpc * d
    lf = LiveFrames(n_cam, frame_hw=hw, frames_per_clip=fpc, frame_step=d, clip_stride=s, device=DEV)
    ref = FrameRingRef(n_cam, shape, fpc, d, s)
    rng = np.random.default_rng(50 + R + s)
    series = [[] for _ in range(n_cam)]
    dues = 0
    for step in range(4 * R + 5):
        cams = [c for c, every in ((3, 1), (0, 2), (1, 3)) if step % every == 0]  # camera 3 every step, 0 every 2nd, 1 every 3rd, 2 never
        frames = rng.integers(0, 256, size=(len(cams),) + shape, dtype=np.uint8)
        for i, c in enumerate(cams):
            series[c].append(frames[i])
        due = lf.push(cams, _dev(frames))
        assert due == ref.push(cams, frames) and lf.counts_host == tuple(ref.counts.tolist())
        if due:
            dues += 1
            got = _np(lf.windows(due))
            assert np.array_equal(got, ref.windows(list(due)))
            for v, c in enumerate(due):  # window w of the camera's series, by slicing
                w = (len(series[c]) - R) // s
                assert np.array_equal(got[v * fpc:(v + 1) * fpc], np.stack(series[c])[w * s: w * s + R: d])
    assert dues > 4 and lf.counts.tolist() == ref.counts.tolist() and lf.counts_host[2] == 0
    # reset: camera 3 starts over, camera 0 keeps its frames
    lf.reset([3])
    ref.reset([3])
    assert lf.counts.tolist() == list(lf.counts_host) == ref.counts.tolist() and lf.counts_host[3] == 0
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    new = []
    for k in range(1, R + 1):
        with pytest.raises(HipExtensionError, match=rf"LiveFrames.windows: cameras \[3\] have fewer than span = {R} frames"):
            lf.windows([0, 3])
        f = rng.integers(0, 256, size=(1,) + shape, dtype=np.uint8)
        new.append(f[0])
        due = lf.push([3], _dev(f))
        assert due == ref.push([3], f) == ((3,) if k == R else ())
    assert np.array_equal(_np(lf.windows([3])), np.stack(new)[::d])  # only frames pushed after the reset


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scorer():
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    m.load_state_dict(synth_module_state_dict(m), strict=True)
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def backbone():
    from anomaly_detection_on_video_amd.i3d import I3Res50

    m = I3Res50()
    m.load_state_dict(synth_i3d_state_dict())
    return m.eval().to(DEV)


def _bits(t):
    return _np(t).view(np.int32)


@pytest.mark.parametrize("fpc,d,s,n_frames", [(16, 1, 8, 32), (8, 2, 8, 32)])
def test_step_camera_frames_is_the_offline_windows_pushed_and_scored(scorer, backbone, fpc, d, s, n_frames):
    """Cameras 2 and 0 of 3; camera 0 starts 3 frames late.  At every due moment the scores equal forward_frames on the windows
    cut by slicing from the cameras' linear frame series, pushed and scored on a second LiveScorer: bit for bit."""
    from anomaly_detection_on_video_amd.live import LiveFrames, LiveScorer

    CH, W, late, hw = 2048, 5, 3, (256, 340)
    R = fpc * d
    rng = np.random.default_rng(60 + d)
    series = {c: torch.from_numpy(rng.integers(0, 256, size=(n_frames,) + hw + (3,), dtype=np.uint8)).to(DEV) for c in (2, 0)}
    lf = LiveFrames(3, frame_hw=hw, frames_per_clip=fpc, frame_step=d, clip_stride=s, device=DEV)
    ref = FrameRingRef(3, (1,), fpc, d, s)  # (the model's due rule and counts; its frames are not used)
    a = LiveScorer(scorer, 3, window=W, ncrops=2, channels=CH, device=DEV)
    b = LiveScorer(scorer, 3, window=W, ncrops=2, channels=CH, device=DEV)
    pushed = {2: 0, 0: 0}
    n_due = n_none = 0
    for step in range(n_frames + late):
        cams = [c for c in (2, 0) if (step >= late or c == 2) and pushed[c] < n_frames]
        frames = torch.stack([series[c][pushed[c]] for c in cams])
        for c in cams:
            pushed[c] += 1
        want_due = ref.push(cams, np.zeros((len(cams), 1), dtype=np.uint8))
        got = a.step_camera_frames(backbone, lf, cams, frames, crops="center_flip")
        if not want_due:
            assert got is None
            n_none += 1
            continue
        n_due += 1
        clips = torch.cat([series[c][((pushed[c] - R) // s) * s: ((pushed[c] - R) // s) * s + R: d] for c in want_due])
        feats = backbone.forward_frames(clips, 0, len(want_due) * 2, frames_per_clip=fpc, crops="center_flip")
        b.push(want_due, feats.reshape(len(want_due), 2, CH))
        want = b.score(want_due)
        assert got.cams == want.cams == want_due and got.lens == want.lens
        assert np.array_equal(_bits(got.scores), _bits(want.scores)) and np.array_equal(_bits(got.latest), _bits(want.latest)), step
    per_cam = (n_frames - R) // s + 1
    assert n_due + n_none == n_frames + late and a.counts_host == b.counts_host == (per_cam, 0, per_cam)
    assert n_due > per_cam  # (the late camera's clips came due at moments of their own)
    assert torch.equal(a.ring, b.ring) and torch.equal(a.counts, b.counts) and torch.equal(a.latest.nan_to_num(-1), b.latest.nan_to_num(-1))
    assert lf.counts_host == (n_frames, 0, n_frames) and lf.counts.tolist() == [n_frames, 0, n_frames]


# ---- 7. the steady state dispatches nothing ------------------------------------------------------------------------------------------------
def test_steady_state_push_and_windows_dispatch_no_torch_arithmetic():
    from anomaly_detection_on_video_amd.live import LiveFrames
    from test_hip_strict import AtenAudit

    hw, fpc, cams = (8, 10), 4, (0, 2, 3)
    lf = LiveFrames(4, frame_hw=hw, frames_per_clip=fpc, clip_stride=1, device=DEV)
    rng = np.random.default_rng(70)
    frames = [_dev(rng.integers(0, 256, size=(3,) + hw + (3,), dtype=np.uint8)) for _ in range(fpc + 2)]
    for f in frames[:fpc + 1]:
        due = lf.push(cams, f)
    warm = lf.windows(due).clone()  # (the id vector of this camera set)
    with AtenAudit() as audit:
        due = lf.push(cams, frames[fpc + 1])
        clips = lf.windows(due)
    assert due == cams
    assert audit.arithmetic() == {}, f"torch arithmetic on the live frame step: {audit.arithmetic()}"
    assert "_to_copy" not in audit.ops and "copy_" not in audit.ops, audit.ops
    assert torch.equal(clips.view(3, fpc, *hw, 3)[:, :-1], warm.view(3, fpc, *hw, 3)[:, 1:])  # the windows moved on by one frame
    assert torch.equal(clips.view(3, fpc, *hw, 3)[:, -1], frames[fpc + 1])
    assert lf.counts.tolist() == list(lf.counts_host) == [fpc + 2, 0, fpc + 2, fpc + 2]


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_live_frames_refusals():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames

    hw = (4, 4)
    lf = LiveFrames(4, frame_hw=hw, frames_per_clip=2, device=DEV)
    ok = torch.zeros((2,) + hw + (3,), dtype=torch.uint8, device=DEV)
    for cams, what in (([1, 1], r"duplicate camera ids \[1\]: one frame per camera and call"), ([0, 4], r"camera id 4 is out of range \[0, 4\)"),
                       ([-1, 0], "camera id -1 is out of range"), ([], "an empty list of cameras"), ((), "an empty list of cameras"),
                       ([0, 1.5], "camera id 1.5 is not a host integer"), (3, "cams must be a sequence of camera ids, got int")):
        with pytest.raises(HipExtensionError, match="LiveFrames.push: " + what):
            lf.push(cams, ok)
        with pytest.raises(HipExtensionError, match="LiveFrames.windows: " + what):
            lf.windows(cams)
        with pytest.raises(HipExtensionError, match="LiveFrames.reset: " + what):
            lf.reset(cams)
    for frames, what in ((ok[:1], "frames must be a torch.uint8 tensor with 2 leading rows"), (ok.float(), "frames must be a torch.uint8 tensor with 2 leading rows"),
                         (ok.cpu().numpy(), "frames must be a torch.uint8 tensor with 2 leading rows"),
                         (ok[:, :3], r"frames must be \(2, 4, 4, 3\) \(frames at ring size")):
        with pytest.raises(HipExtensionError, match="LiveFrames.push: " + what):
            lf.push([0, 1], frames)
    with pytest.raises(HipExtensionError, match="LiveFrames.push: pixel_format / surface describe frames to be converted: give resize="):
        lf.push([0, 1], ok, pixel_format="nv12")
    with pytest.raises(HipExtensionError, match="frame_ring_push: frames must be contiguous"):
        lf.push([0, 1], torch.zeros((4, 2, 4, 3), dtype=torch.uint8, device=DEV).transpose(0, 1))
    with pytest.raises(HipExtensionError, match=r"LiveFrames.windows: cameras \[0, 1\] have fewer than span = 2 frames"):
        lf.windows([0, 1])
    assert lf.counts.tolist() == list(lf.counts_host) == [0] * 4 and not lf.ring.any()  # a refused call moves nothing
    assert lf.push([0, 1], ok.cpu()) == () and lf.push([1, 0], ok) == (1, 0)  # host frames at ring size are taken
    with pytest.raises(HipExtensionError, match=r"LiveFrames.windows: cameras \[2\] have fewer than span = 2 frames"):
        lf.windows([0, 2])
    assert tuple(lf.windows([1]).shape) == (2, 4, 4, 3)


def test_launch_wrapper_refusals():
    from anomaly_detection_on_video_amd import _lib, mil_ops
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    R, fpc, d, shape = 4, 2, 2, (4, 4, 3)
    ring = torch.zeros((N_CAM, R) + shape, dtype=torch.uint8, device=DEV)
    counts = torch.zeros((N_CAM,), dtype=torch.int64, device=DEV)
    frames = torch.ones((2,) + shape, dtype=torch.uint8, device=DEV)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    dst = torch.zeros((2 * fpc,) + shape, dtype=torch.uint8, device=DEV)
    push, win = mil_ops.frame_ring_push, mil_ops.frame_ring_windows
    cases = [
        (lambda: push(frames.cpu(), ids, ring, counts), "frame_ring_push: frames is on 'cpu'"),
        (lambda: push(frames, ids.cpu(), ring, counts), "frame_ring_push: cam_ids is on 'cpu'"),
        (lambda: push(frames, ids, ring.cpu(), counts), "frame_ring_push: ring is on 'cpu'"),
        (lambda: push(frames, ids, ring, counts.cpu()), "frame_ring_push: counts is on 'cpu'"),
        (lambda: push(frames.float(), ids, ring, counts), "frame_ring_push: frames must be torch.uint8, got torch.float32"),
        (lambda: push(frames, ids.long(), ring, counts), "frame_ring_push: cam_ids must be torch.int32, got torch.int64"),
        (lambda: push(frames, ids, ring.int(), counts), "frame_ring_push: ring must be torch.uint8, got torch.int32"),
        (lambda: push(frames, ids, ring, counts.int()), "frame_ring_push: counts must be torch.int64, got torch.int32"),
        (lambda: push(frames[:, :3], ids, ring, counts), r"frame_ring_push: frames must be \(\*, 4, 4, 3\), got \(2, 3, 4, 3\)"),
        (lambda: push(torch.ones((4, 2, 4, 3), dtype=torch.uint8, device=DEV).transpose(0, 1), ids, ring, counts), "frame_ring_push: frames must be contiguous"),
        (lambda: push(frames.view(2, 48), ids, ring, counts), r"frame_ring_push: frames must be \(\*, 4, 4, 3\), got \(2, 48\)"),
        (lambda: push(frames, ids[:1], ring, counts), r"frame_ring_push: cam_ids must be \(2,\), got \(1,\)"),
        (lambda: push(frames, ids, ring, counts[:5]), r"frame_ring_push: counts must be \(6,\), got \(5,\)"),
        (lambda: push(frames, ids, ring[:, :, :, :3], counts), "frame_ring_push: ring must be contiguous"),
        (lambda: push(frames, ids, ring[0, 0, 0], counts), r"frame_ring_push: ring must be a torch.uint8 tensor \(n_cam, R, frame_bytes\)"),
        (lambda: push(frames, ids, None, counts), r"frame_ring_push: ring must be a torch.uint8 tensor \(n_cam, R, frame_bytes\)"),
        (lambda: win(ring, counts, ids, dst.cpu(), fpc, d), "frame_ring_windows: dst is on 'cpu'"),
        (lambda: win(ring, counts, ids, dst.short(), fpc, d), "frame_ring_windows: dst must be torch.uint8, got torch.int16"),
        (lambda: win(ring, counts, ids, dst[:3], fpc, d), r"frame_ring_windows: dst must be \(4, 4, 4, 3\), got \(3, 4, 4, 3\)"),
        (lambda: win(ring, counts, ids, torch.zeros((2 * fpc, 4, 3, 4), dtype=torch.uint8, device=DEV).transpose(2, 3), fpc, d),
         "frame_ring_windows: dst must be contiguous"),
        (lambda: win(ring, counts[:3], ids, dst, fpc, d), r"frame_ring_windows: counts must be \(6,\)"),
        (lambda: win(ring, counts, ids.long(), dst, fpc, d), "frame_ring_windows: cam_ids must be torch.int32"),
        (lambda: win(ring, counts, ids.view(1, 2), dst, fpc, d), r"frame_ring_windows: cam_ids must be \(\*,\), got \(1, 2\)"),
        (lambda: win(ring, counts, ids, dst, 0, d), "frame_ring_windows: frames_per_clip 0 is not a positive integer"),
        (lambda: win(ring, counts, ids, dst, fpc, 1.0), "frame_ring_windows: frame_step 1.0 is not a positive integer"),
        # R != frames_per_clip * frame_step: the entry point's own refusal
        (lambda: win(ring, counts, ids, dst, fpc, 1), r"frame_ring_windows failed \(code -1\): frame_ring_windows: R=4 is not frames_per_clip \* frame_step = 2 \* 1"),
        (lambda: win(ring, counts, ids, torch.zeros((2,) + shape, dtype=torch.uint8, device=DEV), 1, 2), r"R=4 is not frames_per_clip \* frame_step = 1 \* 2"),
    ]
    if torch.cuda.device_count() > 1:
        cases.append((lambda: push(frames, ids.to("cuda:1"), ring, counts), "frame_ring_push: cam_ids is on cuda:1, the arguments before it are on cuda:0"))
    for call, what in cases:
        with pytest.raises(HipExtensionError, match=what):
            call()
    assert not ring.any() and not counts.any() and not dst.any()  # nothing was launched
    lib = _lib.load()
    assert lib.advhip_frame_ring_windows_u8(ring.data_ptr(), counts.data_ptr(), ids.data_ptr(), dst.data_ptr(), 2, N_CAM, R, 48, 4, 2, None) == -1
    assert "R=4 is not frames_per_clip * frame_step = 4 * 2" in lib.advhip_last_error().decode()


def test_step_camera_frames_refusals(scorer):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames, LiveScorer

    hw = (4, 4)
    lf = LiveFrames(3, frame_hw=hw, frames_per_clip=2, device=DEV)
    live = LiveScorer(scorer, 3, window=5, ncrops=2, channels=2048, device=DEV)
    ok = torch.zeros((2,) + hw + (3,), dtype=torch.uint8, device=DEV)
    what = "LiveScorer.step_camera_frames: "
    for kw, msg in ((dict(frames_per_clip=2), "frames_per_clip belong to the LiveFrames"), (dict(clip_stride=1, frame_step=1), "frame_step, clip_stride belong to the LiveFrames"),
                    (dict(crops="center"), "1 crops, the rings hold 2"), (dict(), "10 crops, the rings hold 2"),
                    (dict(crops="center_flip", size=3), r"unknown arguments \['size'\]")):
        with pytest.raises(HipExtensionError, match=what + msg):
            live.step_camera_frames(None, lf, [0, 1], ok, **kw)
    with pytest.raises(HipExtensionError, match=what + "live_frames must be a LiveFrames, got NoneType"):
        live.step_camera_frames(None, None, [0, 1], ok, crops="center_flip")
    with pytest.raises(HipExtensionError, match=what + "the LiveFrames holds 4 cameras on cuda:0, the LiveScorer 3 on cuda:0"):
        live.step_camera_frames(None, LiveFrames(4, frame_hw=hw, frames_per_clip=2, device=DEV), [0, 1], ok, crops="center_flip")
    with pytest.raises(HipExtensionError, match=r"LiveFrames.push: duplicate camera ids \[1\]"):
        live.step_camera_frames(None, lf, [1, 1], ok, crops="center_flip")
    assert lf.counts_host == (0, 0, 0) and live.counts_host == (0, 0, 0)  # every refusal came before the push
    assert live.step_camera_frames(None, lf, [0, 1], ok, crops="center_flip") is None  # nothing due: the backbone is not touched
    assert lf.counts_host == (1, 1, 0)
