"""Host tests of the event rule (no GPU): hand-written known answers for the sequential reference tests/_events_ref.py, the
vectorised events.find_events_host against it on 300 seeded random ragged batches, resolve_event_spec's refusals by name, and
the two C entry points' argument validation (ADVHIP_EINVAL before anything is launched)."""
import ctypes as C

import numpy as np
import pytest

import _events_ref as ref
from anomaly_detection_on_video_amd import events

NAN = float("nan")


def _ev(x, low, high, **kw):
    ev_int, ev_f, counts, _ = ref.events_ref(np.asarray(x, np.float32), [len(x)], low, high, **kw)
    return [tuple(int(i) for i in r[1:]) for r in ev_int], ev_f, counts


def test_reference_known_answers():
    # a weak-only candidate (frames 1-2 never reach high) and a strong one
    rows, ev_f, counts = _ev([0.1, 0.75, 0.8, 0.1, 0.72, 0.95, 0.1], 0.7, 0.9)
    assert rows == [(4, 6, 5)] and counts.tolist() == [1]
    assert ev_f[0, 0] == np.float32(0.95) and ev_f[0, 1] == np.float32((float(np.float32(0.72)) + float(np.float32(0.95))) / 2)
    # too short: two strong frames, min_len 3; kept at min_len 2
    x = [0.0, 0.95, 0.95, 0.0]
    assert _ev(x, 0.7, 0.9, min_len=3)[0] == [] and _ev(x, 0.7, 0.9, min_len=2)[0] == [(1, 3, 1)]
    # two runs two frames apart: one candidate at merge_gap 2, two at 1 (of which the weak one is dropped)
    x = [0.95, 0.8, 0.1, 0.2, 0.75, 0.0]
    assert _ev(x, 0.7, 0.9, merge_gap=2)[0] == [(0, 5, 0)]
    assert _ev(x, 0.7, 0.9, merge_gap=1)[0] == [(0, 2, 0)]
    # merging chains: three runs, each one frame from the next
    assert _ev([0.95, 0.0, 0.8, 0.0, 0.8], 0.7, 0.9, merge_gap=1)[0] == [(0, 5, 0)]
    # a plateau peak: the first of the equal frames
    assert _ev([0.8, 0.95, 0.95, 0.95, 0.8], 0.7, 0.9)[0] == [(0, 5, 1)]
    # a NaN in a merged gap: NaN mean, the peak ignores it
    rows, ev_f, _ = _ev([0.95, NAN, 0.8], 0.7, 0.9, merge_gap=1)
    assert rows == [(0, 3, 0)] and np.isnan(ev_f[0, 1]) and ev_f[0, 0] == np.float32(0.95)
    # a NaN frame is not active: without merging it splits the run
    assert _ev([0.95, NAN, 0.8], 0.7, 0.9)[0] == [(0, 1, 0)]
    # smoothing: window 3 on a spike, clipped at both ends
    y = ref.smooth_ref(np.array([0, 3, 0, 0], np.float32), 3)
    assert y.tolist() == [1.5, 1.0, 1.0, 0.0]
    # w = 1 keeps the bits but -0.0; the window never leaves the video
    y = ref.smooth_ref(np.array([-0.0, 1e-45, np.inf], np.float32), 1)
    assert y.view(np.int32).tolist() == np.array([0.0, 1e-45, np.inf], np.float32).view(np.int32).tolist()
    ev_int, _, counts, ys = ref.events_ref(np.array([1, 1, 0, 0], np.float32), [2, 2], 0.5, 0.5, smooth=3)
    assert ys.tolist() == [1, 1, 0, 0] and ev_int.tolist() == [[0, 0, 2, 0]] and counts.tolist() == [1, 0]


def test_fast_reference_smoothing_is_the_sequential_one():
    rng = np.random.default_rng(5)
    for n, w in ((1, 1), (1, 9), (7, 3), (40, 9), (40, 81), (300, 255)):
        x = rng.standard_normal(n).astype(np.float32)
        if n > 5:
            x[2], x[4] = np.nan, -0.0
        a, b = ref.smooth_ref(x, w), ref.smooth_ref_fast(x, w)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (n, w)


def test_host_rule_equals_the_reference_on_random_batches():
    rng = np.random.default_rng(20240)
    kept = 0
    for case in range(300):
        x, lengths = ref.random_batch(rng, int(rng.integers(1, 6)), 120)
        spec = events.EventSpec(0.7, 0.9, int(rng.choice([1, 3, 5, 9])), int(rng.integers(0, 6)), int(rng.integers(1, 8)))
        if case % 25 == 0 and x.size > 3:
            x[int(rng.integers(0, x.size))] = np.nan
        got = events.find_events_host(x, lengths, spec)
        ev_int, ev_f, counts, _ = ref.events_ref(x, lengths, spec.low, spec.high, spec.smooth, spec.merge_gap, spec.min_len)
        ref.assert_events_equal(got.ev_int, got.ev_f, got.counts, ev_int, ev_f, counts, f"case {case} {spec} lengths {lengths}")
        assert got.ev_int.dtype == np.int32 and got.ev_f.dtype == np.float32 and len(got) == ev_int.shape[0]
        kept += len(got)
    assert kept > 300  # the distribution exercises the rule (about 1 400 events)


def test_events_object_on_the_host():
    x = np.array([0.95, 0.0, 0.95, 0.95, 0.0, 0.95], np.float32)
    ev = events.find_events_host(x, [2, 0, 4], (0.7, 0.9))
    assert len(ev) == 3 and ev.counts.tolist() == [1, 0, 2] and ev.numpy() is ev
    assert ev.video.tolist() == [0, 2, 2] and ev.start.tolist() == [0, 0, 3] and ev.end.tolist() == [1, 2, 4]
    assert len(ev.per_video(1)) == 0 and ev.per_video(2).start.tolist() == [0, 3]
    sec = ev.to_seconds(2.0)
    assert sec["start"].tolist() == [0.0, 0.0, 1.5] and sec["end"].tolist() == [0.5, 1.0, 2.0] and sec["video"].tolist() == [0, 2, 2]
    with pytest.raises(IndexError):
        ev.per_video(3)
    with pytest.raises(ValueError, match="sum to"):
        events.find_events_host(x, [2, 3], (0.7, 0.9))
    assert len(events.find_events_host(np.zeros(0, np.float32), [0, 0], (0.7, 0.9))) == 0


@pytest.mark.parametrize("spec, name", [
    ({"low": NAN, "high": 1.0}, "low"), ({"low": 0.1, "high": float("inf")}, "high"), ({"low": 0.9, "high": 0.7}, "low"),
    ({"high": 0.7}, "low"), ({"low": 0.7}, "high"), ({"low": "a", "high": 1.0}, "low"), ({"low": 0.1, "high": 1e39}, "high"),
    ({"low": 0.1, "high": 0.2, "smooth": 4}, "smooth"), ({"low": 0.1, "high": 0.2, "smooth": 1025}, "smooth"),
    ({"low": 0.1, "high": 0.2, "smooth": 0}, "smooth"), ({"low": 0.1, "high": 0.2, "smooth": 3.0}, "smooth"),
    ({"low": 0.1, "high": 0.2, "merge_gap": -1}, "merge_gap"), ({"low": 0.1, "high": 0.2, "min_len": 0}, "min_len"),
    ({"low": 0.1, "high": 0.2, "gap": 1}, "gap"), ((0.1,), "tuple"), (0.5, "mapping"),
])
def test_resolve_event_spec_refuses_by_name(spec, name):
    with pytest.raises(ValueError, match=name):
        events.resolve_event_spec(spec)


def test_resolve_event_spec_accepts():
    assert events.resolve_event_spec(None) is None
    want = events.EventSpec(0.5, 0.5, 3, 2, 4)
    assert events.resolve_event_spec({"low": 0.5, "high": 0.5, "smooth": 3, "merge_gap": 2, "min_len": 4}) == want
    assert events.resolve_event_spec((0.5, 0.5, 3, 2, 4)) == want and events.resolve_event_spec(want) == want
    assert events.resolve_event_spec([0, 1]) == events.EventSpec(0.0, 1.0, 1, 0, 1)


def test_capi_refuses_bad_arguments_without_gpu():
    """Every call below fails validation, so nothing is launched and no pointer is dereferenced."""
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    p = C.c_void_p(4096)  # stands for a device pointer
    ws = lib.advhip_score_events_ws_bytes(1000, 3)
    assert ws > 0 and lib.advhip_score_events_ws_bytes(1, 1) > 0

    def smooth(scores=p, offsets=p, v=3, n=1000, window=5, out=C.c_void_p(8192)):
        return lib.advhip_smooth_scores_f32(scores, offsets, v, n, window, out, None)

    for kw, text in (({"scores": None}, b"null"), ({"offsets": None}, b"null"), ({"out": None}, b"null"), ({"n": 0}, b"N"),
                     ({"n": 1 << 31}, b"N"), ({"v": 0}, b"V"), ({"window": 4}, b"window"), ({"window": 1025}, b"window"),
                     ({"window": 0}, b"window"), ({"window": -3}, b"window"), ({"out": p}, b"out")):
        assert smooth(**kw) == -1, kw
        assert text in lib.advhip_last_error(), (kw, lib.advhip_last_error())

    def score(y=p, offsets=p, v=3, n=1000, low=0.5, high=0.7, gap=0, min_len=1, ev_int=p, ev_f=p, cap=500, counts=p, meta=p, w=p,
              wbytes=ws):
        return lib.advhip_score_events(y, offsets, v, n, low, high, gap, min_len, ev_int, ev_f, cap, counts, meta, w, wbytes, None)

    for kw, text in (({"y": None}, b"null"), ({"offsets": None}, b"null"), ({"ev_int": None}, b"null"), ({"ev_f": None}, b"null"),
                     ({"counts": None}, b"null"), ({"meta": None}, b"null"), ({"w": None}, b"null"), ({"n": 0}, b"N"),
                     ({"n": 1 << 31}, b"N"), ({"v": 0}, b"V"), ({"low": 0.8}, b"low"), ({"low": NAN}, b"finite"),
                     ({"high": float("inf")}, b"finite"), ({"gap": -1}, b"merge_gap"), ({"min_len": 0}, b"min_len"),
                     ({"cap": 0}, b"cap"), ({"wbytes": ws - 1}, b"workspace"), ({"w": C.c_void_p(4100)}, b"aligned")):
        assert score(**kw) == -1, kw
        assert text in lib.advhip_last_error(), (kw, lib.advhip_last_error())
    assert lib.advhip_score_events_ws_bytes(0, 1) == -1 and lib.advhip_score_events_ws_bytes(5, 0) == -1
    assert lib.advhip_score_events_ws_bytes(1 << 31, 1) == -1
    assert lib.advhip_abi_version() == 2
