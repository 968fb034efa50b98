"""Host tests of the live frame rings: the numpy model the GPU tests compare with (tests/_live_frames_ref.py) against plain
slicing of the frame series -- the due moments and the bytes of every window --, LiveFrames' refusals that need no GPU, and the
two entry points' refusals before any launch."""
import numpy as np
import pytest

from _live_frames_ref import FrameRingRef, scripted_counts, scripted_pushes, strides


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("fpc", [1, 2, 4])
def test_model_is_slicing_of_the_frame_series(fpc, d):
    span = fpc * d
    rng = np.random.default_rng(100 * fpc + d)
    for s in strides(span):
        for F in range(0, 3 * span + 3):
            frames = rng.integers(0, 256, size=(F, 2, 3), dtype=np.uint8)
            ref = FrameRingRef(2, (2, 3), fpc, d, s)  # (camera 0 stays empty)
            due_at, w = [], 0
            for k in range(1, F + 1):
                due = ref.push([1], frames[k - 1:k])
                assert due in ((), (1,))
                if due:
                    due_at.append(k)
                    want = frames[w * s: w * s + span: d]
                    assert want.shape[0] == fpc
                    assert np.array_equal(ref.windows([1]), want), (fpc, d, s, F, w)
                    w += 1
            n = (F - span) // s + 1 if F >= span else 0
            assert due_at == [span + i * s for i in range(n)], (fpc, d, s, F)
            assert not ref.has_window(0) and ref.has_window(1) == (F >= span)


@pytest.mark.parametrize("R", [1, 4, 12])
def test_scripted_pushes_reach_the_scripted_counts(R):
    ref = FrameRingRef(6, (2, 2, 3), R)
    for cams, frames in scripted_pushes(R, (2, 2, 3)):
        ref.push(cams, frames)
    assert ref.counts.tolist() == scripted_counts(R)
    fill = ref.windows([0, 6, -1])
    assert (fill == 0xA5).all()  # no window: an empty camera, ids outside the range


def test_live_frames_refusals_that_need_no_gpu():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames

    for kw, what in ((dict(n_cameras=0), "n_cameras = 0 is not an integer >= 1"), (dict(n_cameras=2.5), "n_cameras = 2.5 is not an integer"),
                     (dict(n_cameras=2, frame_hw=(0, 4)), r"frame_hw\[0\] = 0 is not an integer >= 1"),
                     (dict(n_cameras=2, frame_hw=8), "frame_hw = 8 is not a pair"),
                     (dict(n_cameras=2, frames_per_clip=0), "frames_per_clip = 0 is not an integer >= 1"),
                     (dict(n_cameras=4096, frames_per_clip=16), "4096 cameras x 16 frames per clip is above the 65535 frame rows"),
                     (dict(n_cameras=2, device="cpu"), "device 'cpu': the rings live on the GPU")):
        with pytest.raises(HipExtensionError, match="LiveFrames: " + what):
            LiveFrames(**kw)
    # the sampling arguments' ranges and messages are the package's own (ops.resolve_sampling)
    with pytest.raises(ValueError, match=r"clip_stride 17 outside \[1, frames_per_clip = 16\]"):
        LiveFrames(2, clip_stride=17, device="cpu")
    with pytest.raises(ValueError, match=r"clip_stride 0 outside \[1, frames_per_clip \* frame_step = 8\]"):
        LiveFrames(2, frames_per_clip=4, frame_step=2, clip_stride=0, device="cpu")
    with pytest.raises(ValueError, match="frame_step 0: an integer >= 1"):
        LiveFrames(2, frame_step=0, device="cpu")


def test_entry_points_refuse_null_pointers_and_bad_sizes_before_any_launch():
    """Pure host-side validation: every call returns ADVHIP_EINVAL with a message, with or without a GPU."""
    import __graft_entry__
    from anomaly_detection_on_video_amd import _lib

    __graft_entry__.build()
    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is refused first
    push, win = lib.advhip_frame_ring_push_u8, lib.advhip_frame_ring_windows_u8
    cases = [
        (push, (None, p, p, p, 1, 1, 4, 48, None), "frame_ring_push: null pointer"),
        (push, (p, None, p, p, 1, 1, 4, 48, None), "frame_ring_push: null pointer"),
        (push, (p, p, None, p, 1, 1, 4, 48, None), "frame_ring_push: null pointer"),
        (push, (p, p, p, None, 1, 1, 4, 48, None), "frame_ring_push: null pointer"),
        (push, (p, p, p, p, 0, 1, 4, 48, None), "frame_ring_push: bad shape"),
        (push, (p, p, p, p, 1, 0, 4, 48, None), "frame_ring_push: bad shape"),
        (push, (p, p, p, p, 1, 1, 0, 48, None), "frame_ring_push: bad shape"),
        (push, (p, p, p, p, 1, 1, 4, 0, None), "frame_ring_push: bad shape"),
        (push, (p, p, p, p, 65536, 70000, 4, 48, None), "frame_ring_push: 65536 rows of 48 bytes are outside the launch grid"),
        (win, (None, p, p, p, 1, 1, 4, 48, 4, 1, None), "frame_ring_windows: null pointer"),
        (win, (p, p, p, None, 1, 1, 4, 48, 4, 1, None), "frame_ring_windows: null pointer"),
        (win, (p, p, p, p, 0, 1, 4, 48, 4, 1, None), "frame_ring_windows: bad shape"),
        (win, (p, p, p, p, 1, 1, 4, -1, 4, 1, None), "frame_ring_windows: bad shape"),
        (win, (p, p, p, p, 1, 1, 4, 48, 4, 0, None), "frame_ring_windows: bad shape"),
        (win, (p, p, p, p, 1, 1, 4, 48, 2, 1, None), "frame_ring_windows: R=4 is not frames_per_clip * frame_step = 2 * 1"),
        (win, (p, p, p, p, 1, 1, 6, 48, 4, 2, None), "frame_ring_windows: R=6 is not frames_per_clip * frame_step = 4 * 2"),
        (win, (p, p, p, p, 4096, 1, 16, 48, 16, 1, None), "frame_ring_windows: 65536 rows of 48 bytes are outside the launch grid"),
    ]
    for fn, args, what in cases:
        assert fn(*args) == -1 and what in lib.advhip_last_error().decode(), (what, lib.advhip_last_error())
