"""Host tests of live scoring: the slot rule (LiveScorer.window_order) and the numpy ring model the GPU tests compare with
(tests/_live_ref.py), each against a brute-force list of the clips pushed."""
import numpy as np
import pytest

from _live_ref import RingRef, scripted_counts, scripted_pushes

WINDOWS = (1, 5, 8)


@pytest.mark.parametrize("W", WINDOWS)
def test_window_order_is_the_last_clips_oldest_first(W):
    from anomaly_detection_on_video_amd.live import LiveScorer

    for count in scripted_counts(W):
        holds = {}  # slot -> the number of the clip that lies there
        for k in range(count):
            holds[k % W] = k
        want = tuple(slot for slot, _ in sorted(holds.items(), key=lambda kv: kv[1]))
        got = LiveScorer.window_order(count, W)
        assert got == want, (count, W)
        assert len(got) == min(count, W)
        assert sorted(holds[s] for s in got) == list(range(max(0, count - W), count))
    assert LiveScorer.window_order(0, W) == ()
    with pytest.raises(ValueError):
        LiveScorer.window_order(-1, W)
    with pytest.raises(ValueError):
        LiveScorer.window_order(3, 0)


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("C", [5, 130])
def test_ring_model_against_a_list_of_the_pushed_clips(W, C):
    from anomaly_detection_on_video_amd.live import LiveScorer

    ncrops, n_cam = 3, 6
    ref = RingRef(n_cam, ncrops, W, C)
    pushed = [[] for _ in range(n_cam)]  # per camera: every clip (ncrops, C + 1) in the order it came
    for cams, feats in scripted_pushes(W, ncrops, C):
        ref.push(cams, feats)
        for i, c in enumerate(cams):
            mag = np.sqrt(np.add.reduce(feats[i] * feats[i], axis=-1))
            pushed[c].append(np.concatenate([feats[i], mag[:, None]], axis=1))
    assert ref.counts.tolist() == scripted_counts(W) == [len(p) for p in pushed]
    cams = list(range(n_cam))
    for tmax in sorted({W, max(1, W - 2)}):
        got = ref.windows(cams, tmax)
        assert ref.lens(cams, tmax) == [min(len(p), W, tmax) for p in pushed]
        for c in cams:
            n = min(len(pushed[c]), W, tmax)
            if n:
                want = np.stack(pushed[c][-n:], axis=1)  # (ncrops, n, C + 1)
                assert np.array_equal(got[c, :, :n].view(np.int32), want.view(np.int32)), (c, tmax)
                # the slots the model read are the ones the stated rule names
                slots = LiveScorer.window_order(len(pushed[c]), W)[-n:]
                assert np.array_equal(ref.ring[c][:, list(slots)].view(np.int32), want.view(np.int32))
            assert np.isnan(got[c, :, n:]).all()


def test_entry_points_refuse_null_pointers_and_bad_sizes_before_any_launch():
    """Pure host-side validation: every call returns ADVHIP_EINVAL with a message, with or without a GPU."""
    import __graft_entry__
    from anomaly_detection_on_video_amd import _lib

    __graft_entry__.build()
    lib = _lib.load()
    p = 4096  # never dereferenced: every call below is refused first
    cases = [
        (lib.advhip_ring_push_f32, (None, p, p, p, 1, 1, 1, 1, 8, None), "ring_push: null pointer"),
        (lib.advhip_ring_push_f32, (p, p, p, None, 1, 1, 1, 1, 8, None), "ring_push: null pointer"),
        (lib.advhip_ring_push_f32, (p, p, p, p, 0, 1, 1, 1, 8, None), "ring_push: bad shape"),
        (lib.advhip_ring_push_f32, (p, p, p, p, 1, 1, 1, 0, 8, None), "ring_push: bad shape"),
        (lib.advhip_ring_push_f32, (p, p, p, p, 1, 1, 1, 1, 8193, None), "ring_push: C=8193 above 8192"),
        (lib.advhip_ring_windows_f32, (p, None, p, p, 1, 1, 1, 1, 1, 9, None), "ring_windows: null pointer"),
        (lib.advhip_ring_windows_f32, (p, p, p, p, 1, 1, 1, 1, 0, 9, None), "ring_windows: bad shape"),
        (lib.advhip_ring_windows_f32, (p, p, p, p, 1 << 20, 1, 1 << 10, 1, 2, 9, None), "ring_windows: 2147483648 rows is outside the launch grid"),
        (lib.advhip_crop_mean_last_f32, (p, p, None, p, 1, 1, 1, None), "crop_mean_last: null pointer"),
        (lib.advhip_crop_mean_last_f32, (p, p, p, p, 1, -1, 1, None), "crop_mean_last: bad shape"),
    ]
    for fn, args, what in cases:
        assert fn(*args) == -1 and what in lib.advhip_last_error().decode(), (what, lib.advhip_last_error())
    assert lib.advhip_abi_version() == 2  # the three entry points are an addition
