"""Host tests of live events: the sequential tracker the GPU tests compare with (tests/_live_events_ref.py) against the offline
rule (tests/_events_ref.py, events.find_events_host) and the emission rule (events.live_emission_count), the new entry point's
refusals and declaration, and the refusals of LiveEventTracker / LiveScorer(events=) that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO
from _events_ref import assert_events_equal, events_ref
from _live_events_ref import LiveRef, rows

SYMBOL = "advhip_live_events_update_f32"
_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "int": C.c_int}


def _series(rng, n):
    """Noise around the thresholds in runs of a few samples, with exact threshold values, zeros of both signs and NaNs."""
    x = np.repeat(rng.uniform(0.0, 1.0, size=n // 3 + 1), 3)[:n] + rng.uniform(-0.15, 0.15, size=n)
    x = x.astype(np.float32)
    for value, p in ((0.5, 0.05), (0.8, 0.05), (0.0, 0.03), (-0.0, 0.03), (np.nan, 0.04)):
        x[rng.random(n) < p] = value
    return x


@pytest.mark.parametrize("seed", range(6))
def test_reference_tracker_is_the_offline_rule_and_emits_when_stated(seed):
    from anomaly_detection_on_video_amd.events import EventSpec, find_events_host, live_emission_count

    rng = np.random.default_rng(100 + seed)
    total = 0
    for _ in range(60):
        n = int(rng.integers(0, 81))
        spec = EventSpec(0.5, 0.8, int(rng.choice([1, 3, 9, 31])), int(rng.choice([0, 1, 2, 5])), int(rng.choice([1, 2, 4])))
        if rng.random() < 0.2:
            spec = EventSpec(0.0, 0.0, spec.smooth, spec.merge_gap, spec.min_len)  # (-0.0 >= 0.0: zeros of both signs are active and strong)
        x = _series(rng, n)
        ref = LiveRef(spec.low, spec.high, spec.smooth, spec.merge_gap, spec.min_len)
        for k in range(n):
            before = len(ref.events)
            ref.update(x[k])
            assert len(ref.events) - before <= 1  # at most one event per update
            assert ref.samples == k + 1
        running = len(ref.events)
        ref.finish()
        assert ref.samples == 0 and ref.generation == 1 and ref.alert == 0 and ref.open_start == -1
        got_int, got_f = rows(ref.events)
        assert (got_int[:, 0] == 0).all()
        got_int = got_int.copy()
        got_int[:, 0] = 0  # generation -> video 0
        want_int, want_f, want_counts, _ = events_ref(x, [n], spec.low, spec.high, spec.smooth, spec.merge_gap, spec.min_len)
        what = f"seed {seed} n {n} {spec}"
        # integers, peak bits and mean bits: the ascending float64 sum is video_events_ref's
        assert np.array_equal(got_int, want_int), f"{what}\n{got_int}\nvs\n{want_int}"
        assert np.array_equal(got_f.view(np.int32), want_f.view(np.int32)), f"{what}\n{got_f}\nvs\n{want_f}"
        host = find_events_host(x, [n], spec)
        assert_events_equal(got_int, got_f, [len(ref.events)], host.ev_int, host.ev_f, host.counts, what)
        for (_, s, e, *_), at in zip(ref.events[:running], ref.emit_at[:running]):
            assert at == live_emission_count(e, spec) == e + spec.merge_gap + (spec.smooth - 1) // 2 + 1, what
            assert at <= n
        for (_, s, e, *_), at in zip(ref.events[running:], ref.emit_at[running:]):
            assert at is None and live_emission_count(e, spec) > n, what  # what finish closed was not due yet
        total += len(ref.events)
    assert total > 20  # the series do hold events


def test_reference_alert_and_open_start_describe_the_open_candidate():
    ref = LiveRef(0.5, 0.8, smooth=1, merge_gap=1, min_len=2)
    seen = []
    for v in (0.1, 0.6, 0.9, 0.2, 0.6, 0.1, 0.1, 0.9):
        ref.update(v)
        seen.append((ref.alert, ref.open_start))
    #        x   0.1      0.6      0.9     0.2     0.6     0.1     0.1 (closes)  0.9
    assert seen == [(0, -1), (0, 1), (1, 1), (1, 1), (1, 1), (1, 1), (0, -1), (0, 7)]
    assert [e[:4] for e in ref.events] == [(0, 1, 5, 2)] and ref.emit_at == [7]
    ref.reset()
    assert ref.generation == 1 and ref.samples == 0 and len(ref.events) == 1  # the open candidate at 7 is dropped
    delayed = LiveRef(0.5, 0.8, smooth=3)
    for k, v in enumerate((0.9, 0.9, 0.9)):
        delayed.update(v)
        assert delayed.open_start == (-1 if k == 0 else 0)  # y[0] is final with the second sample: one sample behind


def test_live_emission_count():
    from anomaly_detection_on_video_amd.events import EventSpec, live_emission_count

    assert live_emission_count(5, EventSpec(0.5, 0.8)) == 6
    assert live_emission_count(5, EventSpec(0.5, 0.8, smooth=9, merge_gap=2)) == 5 + 2 + 4 + 1
    assert live_emission_count(1, (0.5, 0.8, 1023, 7, 3)) == 1 + 7 + 511 + 1
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="end"):
            live_emission_count(bad, EventSpec(0.5, 0.8))
    with pytest.raises(ValueError, match="no event spec"):
        live_emission_count(5, None)
    with pytest.raises(ValueError, match="smooth=4"):
        live_emission_count(5, (0.5, 0.8, 4))


def test_entry_point_refuses_before_any_launch():
    """Pure host-side validation: every call returns ADVHIP_EINVAL with a message, with or without a GPU."""
    import __graft_entry__
    from anomaly_detection_on_video_amd import _lib

    __graft_entry__.build()
    lib = _lib.load()
    fn = lib.advhip_live_events_update_f32
    p = 4096  # never dereferenced: every call below is refused first
    ok = dict(ptrs=[p] * 12, nb=1, n_cam=1, K=1, smooth=1, low=0.5, high=0.8, merge_gap=0, min_len=1, by_camera=0, mode=0)

    def call(**kw):
        a = {**ok, **kw}
        return fn(*a["ptrs"], a["nb"], a["n_cam"], a["K"], a["smooth"], a["low"], a["high"], a["merge_gap"], a["min_len"], a["by_camera"], a["mode"], None)

    cases = [(dict(ptrs=[p] * i + [None] + [p] * (11 - i)), "live_events: null pointer") for i in range(12)]
    cases += [
        (dict(nb=0), "live_events: bad shape (nb = 0"), (dict(n_cam=0), "live_events: bad shape"), (dict(K=0), "live_events: bad shape"),
        (dict(nb=-1), "live_events: bad shape"),
        (dict(smooth=0), "live_events: smooth = 0 is not an odd window in [1, 1023]"), (dict(smooth=4), "live_events: smooth = 4 is not an odd window"),
        (dict(smooth=1025), "live_events: smooth = 1025 is not an odd window"), (dict(smooth=-1), "live_events: smooth = -1 is not an odd window"),
        (dict(merge_gap=-1), "live_events: merge_gap = -1 is negative"), (dict(min_len=0), "live_events: min_len = 0 below 1"),
        (dict(low=float("nan")), "must be finite"), (dict(high=float("inf")), "must be finite"), (dict(low=float("-inf")), "must be finite"),
        (dict(low=0.9, high=0.8), "live_events: low = 0.9 above high = 0.8"),
        (dict(by_camera=2), "live_events: by_camera = 2 is not 0 or 1"), (dict(mode=3), "live_events: mode = 3 is not update (0), finish (1) or reset (2)"),
        (dict(mode=-1), "live_events: mode = -1"),
    ]
    for kw, what in cases:
        assert call(**kw) == -1 and what in lib.advhip_last_error().decode(), (kw, what, lib.advhip_last_error())
    assert lib.advhip_abi_version() == 2  # the entry point is an addition


def test_header_lib_and_exported_symbol_agree():
    import __graft_entry__
    from anomaly_detection_on_video_amd import _lib

    __graft_entry__.build()
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + SYMBOL + r"\s*\(([^)]*)\)\s*;", code)
    assert m, f"{SYMBOL} is not declared in include/advhip.h"
    args = [C.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in (a.strip() for a in m.group(2).split(","))]
    assert _lib.SIGNATURES[SYMBOL] == (_CTYPE[m.group(1)], args), f"{SYMBOL}: include/advhip.h and _lib.SIGNATURES disagree"
    assert hasattr(_lib.load(), SYMBOL)
    names = [a.replace("*", " ").split()[-1] for a in m.group(2).split(",")]
    assert names[:12] == ["scores", "cam_ids"] + [n for n in __import__("anomaly_detection_on_video_amd.mil_ops", fromlist=["x"]).LIVE_EVENTS_STATE]
    for macro, value in (("CAND_INTS", _lib.LIVE_EVENTS_CAND_INTS), ("UPDATE", _lib.LIVE_EVENTS_UPDATE), ("FINISH", _lib.LIVE_EVENTS_FINISH),
                         ("RESET", _lib.LIVE_EVENTS_RESET)):
        assert re.search(rf"#define ADVHIP_LIVE_EVENTS_{macro} {value}\b", code), macro


def test_tracker_refusals_that_need_no_device():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.events import EventSpec, LiveEventTracker

    spec = EventSpec(0.5, 0.8, 3, 1, 2)
    for bad, what in ((None, "no event spec"), ((0.9, 0.8), "low=0.9 is above high=0.8"), ((0.5, 0.8, 4), "smooth=4 is not an odd window"),
                      ((0.5, 0.8, 1025), "smooth=1025"), ((0.5, float("nan")), "high=nan is not a finite number"),
                      ((0.5, 0.8, 1, -1), "merge_gap=-1"), ((0.5, 0.8, 1, 0, 0), "min_len=0"), ("0.5", "expected a mapping")):
        with pytest.raises(HipExtensionError, match="LiveEventTracker: .*" + re.escape(what)):
            LiveEventTracker(bad, 4)
    for n in (0, -1, 1.5, True, "3"):
        with pytest.raises(HipExtensionError, match="LiveEventTracker: n_cameras = "):
            LiveEventTracker(spec, n)
    for k in (0, 2.0, False):
        with pytest.raises(HipExtensionError, match="LiveEventTracker: log = "):
            LiveEventTracker(spec, 4, log=k)
    with pytest.raises(HipExtensionError, match="LiveEventTracker: device 'cpu': the state lives on the GPU"):
        LiveEventTracker(spec, 4, device="cpu")


def test_live_scorer_events_argument_refusals_that_need_no_device():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveScorer

    for bad, what in (((0.9, 0.8), "low=0.9 is above high=0.8"), ({"low": 0.5, "high": 0.8, "window": 3}, "unknown key"), ((0.5, 0.8, 2), "smooth=2")):
        with pytest.raises(HipExtensionError, match="LiveScorer: .*" + re.escape(what)):
            LiveScorer(None, 4, window=5, ncrops=3, events=bad, device="cpu")
    for k in (0, -2, 1.5, True):
        with pytest.raises(HipExtensionError, match="LiveScorer: event_log = "):
            LiveScorer(None, 4, window=5, ncrops=3, events=(0.5, 0.8), event_log=k, device="cpu")
    with pytest.raises(HipExtensionError, match="LiveScorer: device 'cpu'"):  # (events=None: as before)
        LiveScorer(None, 4, window=5, ncrops=3, device="cpu")
