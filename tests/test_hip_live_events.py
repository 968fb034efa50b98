"""GPU tests of live events (csrc/live_events.hip, mil_ops.live_events_update, events.LiveEventTracker, LiveScorer(events=)): the
kernel fed one sample at a time against the sequential tracker of tests/_live_events_ref.py after EVERY update -- emitted counts,
log rows (integers, peak bits, mean bits), alert, open_start, generation -- at the edges of the ring, the gap rule and the log;
what a launch may not touch, two runs, the two ways of passing scores; the whole series against events.find_events_host; every
refusal; and LiveScorer feeding its newest clip scores."""
import numpy as np
import pytest
import torch

from _events_ref import assert_events_equal
from _live_events_ref import LiveRef, rows
from anomaly_detection_on_video_amd.weights import synth_module_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_CAM, K = 5, 4
NAN = float("nan")


def _bytes(state):
    return {k: v.cpu().numpy().tobytes() for k, v in state.items()}


class Pair:
    """A LiveEventTracker and one LiveRef per camera, fed the same samples and compared after every call."""

    def __init__(self, spec, n_cam=N_CAM, log=K, by_camera=False):
        from anomaly_detection_on_video_amd.events import LiveEventTracker, resolve_event_spec

        self.spec = s = resolve_event_spec(spec)
        self.tracker = LiveEventTracker(s, n_cam, log=log, device=DEV)
        self.refs = [LiveRef(s.low, s.high, s.smooth, s.merge_gap, s.min_len) for _ in range(n_cam)]
        self.by_camera, self.n_cam, self.log = by_camera, n_cam, log
        self.series = [[] for _ in range(n_cam)]  # per camera, since its last finish / reset

    def update(self, cams, values):
        if self.by_camera:  # (the entries of unlisted cameras are never read: poison them)
            full = np.full(self.n_cam, 1e30, dtype=np.float32)
            full[list(cams)] = np.asarray(values, dtype=np.float32)
            scores = torch.from_numpy(full).to(DEV)
        else:
            scores = torch.from_numpy(np.asarray(values, dtype=np.float32)).to(DEV)
        self.tracker.update(cams, scores, by_camera=self.by_camera)
        for c, v in zip(cams, values):
            self.refs[c].update(v)
            self.series[c].append(np.float32(v))
        self.check(("update", tuple(cams)))

    def finish(self, cams):
        self.tracker.finish(cams)
        for c in cams:
            self.refs[c].finish()
            self.series[c] = []
        self.check(("finish", tuple(cams)))

    def reset(self, cams):
        self.tracker.reset(cams)
        for c in cams:
            self.refs[c].reset()
            self.series[c] = []
        self.check(("reset", tuple(cams)))

    def check(self, what=""):
        st = {k: self.tracker.state[k].cpu().numpy() for k in ("emitted", "samples", "alert", "open_start", "cand_int", "log_int", "log_f")}
        for c, ref in enumerate(self.refs):
            at = (what, "camera", c, "samples", ref.samples)
            assert st["emitted"][c] == len(ref.events), at
            assert st["samples"][c] == ref.samples == self.tracker.samples_host[c], at
            assert st["alert"][c] == ref.alert and st["open_start"][c] == ref.open_start == st["cand_int"][c, 0], at
            assert st["cand_int"][c, 4] == ref.generation, at
            first = max(0, len(ref.events) - self.log)
            want_int, want_f = rows(ref.events[first:])
            slots = [j % self.log for j in range(first, len(ref.events))]
            assert np.array_equal(st["log_int"][c, slots], want_int), (at, st["log_int"][c], want_int)
            assert np.array_equal(st["log_f"][c, slots].view(np.int32), want_f.view(np.int32)), (at, st["log_f"][c], want_f)

    def feed(self, series, rates=None, seed=0):
        """series[c]: the samples of camera c; at step k the cameras with samples left and k % rates[c] == 0 are fed in one launch,
        in an order that changes from step to step."""
        rates = rates or [1] * len(series)
        left = [list(s) for s in series]
        rng, k = np.random.default_rng(seed), 0
        while any(left):
            cams = [c for c in range(len(series)) if left[c] and k % rates[c] == 0]
            k += 1
            if cams:
                cams = [cams[i] for i in rng.permutation(len(cams))]
                self.update(cams, [left[c].pop(0) for c in cams])


def _noise(rng, n, block=3, nan=0.03):
    """Runs of `block` samples around the thresholds 0.5 / 0.8, some exactly on them, a share of `nan` NaN."""
    x = (np.repeat(rng.uniform(0.0, 1.0, size=n // block + 1), block)[:n] + rng.uniform(-0.15, 0.15, size=n)).astype(np.float32)
    for value, p in ((0.5, 0.05), (0.8, 0.05), (np.nan, nan)):
        x[rng.random(n) < p] = value
    return x


# ---- the kernel against the sequential tracker, every update -------------------------------------------------------------------
@pytest.mark.parametrize("smooth", [1, 3, 1023])
def test_kernel_follows_the_reference_tracker_at_every_update(smooth):
    """Lengths h - 1, h and h + 1 (nothing / one y final before finish), and lengths that cross multiples of `smooth` (the ring
    wraps); finish closes what is open.  smooth = 1023: levels held about as long as the window, so that its mean crosses the
    thresholds, and a single NaN (a share of NaN samples would leave no window without one)."""
    h = (smooth - 1) // 2
    rng = np.random.default_rng(smooth)
    if smooth == 1023:
        lens, block, rates, nan = [2 * smooth + 60, max(h - 1, 0), h, h + 1, smooth + 40], 600, [1, 1, 1, 1, 1], 0.0
    else:
        lens, block, rates, nan = [50 * smooth + 4, max(h - 1, 0), h, h + 1, 150], 3, [1, 2, 1, 3, 2], 0.03
    series = [_noise(rng, n, block, nan) for n in lens]
    series[4][100] = np.nan
    pair = Pair((0.5, 0.8, smooth, 2, 2))
    pair.feed(series, rates, seed=smooth)
    assert pair.tracker.samples_host == tuple(lens)
    pair.finish([4, 0])
    pair.finish([1, 2, 3])
    assert pair.tracker.samples_host == (0,) * N_CAM
    assert sum(len(r.events) for r in pair.refs) >= 2
    if smooth < 1023:
        assert max(len(r.events) for r in pair.refs) > K  # the log wrapped


def test_scripted_edges_of_the_rule():
    """merge_gap = 2, min_len = 2, smooth = 1: every position below is the sample's own."""
    hi, mid, lo = 0.9, 0.6, 0.1
    series = [
        # gaps of exactly merge_gap (one event [0, 6)) and of merge_gap + 1 (a second event [9, 11))
        [hi, hi, lo, lo, hi, hi, lo, lo, lo, hi, hi, lo, lo, lo],
        # no strong sample; below min_len; a NaN sample on its own; a NaN inside a gap (the event's mean is NaN)
        [mid, mid, mid, lo, lo, lo, hi, lo, lo, lo, NAN, lo, hi, hi, NAN, hi, lo, lo, lo],
        # a strong sample only after the candidate is long enough: alert rises there; thresholds met exactly
        [0.5, 0.5, 0.5, 0.8, lo, lo, lo],
        # six events into K = 4
        [hi, hi, lo, lo, lo] * 6,
        # an event still open when the camera is finished
        [lo, hi, hi, hi],
    ]
    pair = Pair((0.5, 0.8, 1, 2, 2))
    pair.feed(series, rates=[1, 2, 1, 1, 3])
    got = [[e[1:4] for e in r.events] for r in pair.refs]
    assert got[0] == [(0, 6, 0), (9, 11, 9)] and got[1] == [(12, 16, 12)] and got[2] == [(0, 4, 3)] and got[4] == []
    assert got[3] == [(5 * j, 5 * j + 2, 5 * j) for j in range(6)]
    assert np.isnan(pair.refs[1].events[0][5]) and not np.isnan(pair.refs[0].events[0][5])
    assert pair.tracker.alert.tolist() == [0, 0, 0, 0, 1] and pair.tracker.open_start.tolist() == [-1, -1, -1, -1, 1]

    d = pair.tracker.drain()
    ev = d.events.numpy()
    assert d.lost.tolist() == [0, 0, 0, 2, 0] and ev.counts.tolist() == [2, 1, 1, 4, 0]
    assert ev.video.tolist() == [0, 0, 1, 2, 3, 3, 3, 3]
    assert ev.start.tolist() == [0, 9, 12, 0, 10, 15, 20, 25]  # camera 3: the newest four, oldest first
    assert d.generation.tolist() == [0] * 8
    for c in range(N_CAM):  # every drained row is the reference's, bit for bit
        want_int, want_f = rows(pair.refs[c].events[-K:])
        mine = ev.per_video(c)
        assert np.array_equal(mine.ev_int[:, 1:], want_int[:, 1:]) and np.array_equal(mine.ev_f.view(np.int32), want_f.view(np.int32))
    again = pair.tracker.drain()
    assert len(again.events) == 0 and again.lost.tolist() == [0] * 5 and again.events.counts.tolist() == [0] * 5

    pair.finish([4, 1])            # camera 4's open event [1, 4) is closed and emitted; camera 1 has nothing open
    assert [e[:4] for e in pair.refs[4].events] == [(0, 1, 4, 1)]
    pair.finish([4])               # finish at n = 0: nothing but the generation moves
    pair.reset([0])
    pair.update([0, 4, 2], [hi, hi, hi])  # camera 2 goes on at position 7, cameras 0 and 4 at 0
    pair.update([4, 0], [hi, hi])
    pair.reset([0])                # the open candidate is dropped
    pair.finish([4, 2])
    assert [e[:4] for e in pair.refs[4].events[1:]] == [(2, 0, 2, 0)] and [r.generation for r in pair.refs] == [2, 1, 1, 0, 3]
    assert len(pair.refs[0].events) == 2 and len(pair.refs[2].events) == 1  # (camera 2: one sample at 7 is below min_len)
    d = pair.tracker.drain()
    assert d.events.numpy().video.tolist() == [4, 4] and d.generation.tolist() == [0, 2] and d.lost.tolist() == [0] * 5


def test_signed_zero_peaks_and_nan_inside_a_window():
    """low = high = 0: zeros of both signs are active and strong (-0.0 >= 0.0).  A sum from +0.0 turns a -0.0 sample into +0.0
    (the rule's own statement at smooth = 1); a y of -0.0 comes from a window sum that underflows in the division.  The peak is
    the first of the equal zeros, with its sign."""
    neg, pos, tiny = -0.0, 0.0, -float(np.float32(1e-45))  # (the smallest fp32 subnormal: / 2 and / 3 round to -0.0)
    pair = Pair((0.0, 0.0, 1, 0, 1))
    pair.feed([[neg, pos, -1.0], [pos, neg, -1.0], [neg, neg, -1.0], [neg, 1.0, pos, -1.0], [-1.0, NAN, neg]])
    pair.finish(range(N_CAM))
    peaks = [np.float32(r.events[0][4]) for r in pair.refs]
    assert [bool(np.signbit(p)) for p in peaks] == [False] * 5 and [e.events[0][3] for e in pair.refs] == [0, 0, 0, 1, 2]
    pair = Pair((0.0, 0.0, 3, 0, 1))
    # y = -0.0, -0.0, +0.0, < 0 ...  and  +0.0, -0.0, -0.0, < 0 ...: both one event [0, 3) with its peak at 0, -0.0 in the first only
    pair.feed([[tiny, pos, pos, pos, -1.0, -1.0, -1.0], [pos, pos, tiny, pos, -1.0, -1.0, -1.0], [tiny], [tiny, tiny], [-1.0, tiny, -1.0]])
    pair.finish(range(N_CAM))
    assert [r.events[0][1:4] for r in pair.refs[:2]] == [(0, 3, 0), (0, 3, 0)]
    assert [bool(np.signbit(np.float32(r.events[0][4]))) for r in pair.refs[:2]] == [True, False]
    assert all(float(r.events[0][4]) == 0.0 for r in pair.refs[:2])
    # smooth = 3: one NaN sample poisons the three windows that hold it, and only those
    pair = Pair((0.5, 0.8, 3, 1, 1))
    pair.feed([[0.9, 0.9, 0.9, NAN, 0.9, 0.9, 0.9, 0.9, 0.1, 0.1, 0.1, 0.1]] * 2 + [[NAN, 0.9, 0.9], [0.9, NAN], [NAN]], rates=[1, 2, 1, 1, 1])
    pair.finish(range(N_CAM))
    assert [e[1:3] for e in pair.refs[0].events] == [(0, 2), (5, 8)]  # y[2..4] are NaN: a gap of 3 > merge_gap


# ---- what a launch touches; repeatability; the two ways of passing scores ------------------------------------------------------
def test_unlisted_cameras_two_runs_and_by_camera():
    rng = np.random.default_rng(7)
    series = [_noise(rng, n) for n in (30, 17, 25, 30, 9)]
    runs = []
    for by_camera in (False, False, True):
        pair = Pair((0.5, 0.8, 5, 1, 2), by_camera=by_camera)
        pair.feed(series, rates=[1, 2, 1, 1, 3], seed=3)
        before = {k: v.clone() for k, v in pair.tracker.state.items()}
        pair.update([3, 0], [0.95, 0.05])  # cameras 1, 2 and 4 are not listed: not a bit of theirs moves
        for k, v in pair.tracker.state.items():
            assert np.array_equal(v[[1, 2, 4]].cpu().numpy().view(np.uint8), before[k][[1, 2, 4]].cpu().numpy().view(np.uint8)), k
        assert not torch.equal(pair.tracker.samples, before["samples"])
        before = {k: v.clone() for k, v in pair.tracker.state.items()}
        pair.finish([2, 3])  # the same for the finish form
        for k, v in pair.tracker.state.items():
            assert np.array_equal(v[[0, 1, 4]].cpu().numpy().view(np.uint8), before[k][[0, 1, 4]].cpu().numpy().view(np.uint8)), k
        runs.append(_bytes(pair.tracker.state))
    assert runs[0] == runs[1], "two runs differ"
    assert runs[0] == runs[2], "by_camera = 0 and 1 differ"


def test_ids_outside_the_cameras_write_nothing():
    from anomaly_detection_on_video_amd import _lib, mil_ops

    state = mil_ops.live_events_state(N_CAM, 3, K, DEV)
    ids = torch.tensor([1, 3], dtype=torch.int32, device=DEV)
    for v in (0.9, 0.9, 0.9, 0.1, 0.1):
        mil_ops.live_events_update(torch.full((2,), v, device=DEV), ids, state, 0.5, 0.8, 3, 0, 1)
    assert state["emitted"].tolist() == [0, 1, 0, 1, 0] and state["samples"].tolist() == [0, 5, 0, 5, 0]
    before = _bytes(state)
    bad = torch.tensor([-1, N_CAM, 1 << 30], dtype=torch.int32, device=DEV)
    for mode, scores in ((_lib.LIVE_EVENTS_UPDATE, torch.ones((3,), device=DEV)), (_lib.LIVE_EVENTS_FINISH, None), (_lib.LIVE_EVENTS_RESET, None)):
        mil_ops.live_events_update(scores, bad, state, 0.5, 0.8, 3, 0, 1, mode=mode)
    assert _bytes(state) == before
    # a camera whose counters no tracker leaves behind is not touched either
    state["samples"][1] = (1 << 31) - 1
    state["emitted"][3] = -1
    before = _bytes(state)
    mil_ops.live_events_update(torch.ones((2,), device=DEV), ids, state, 0.5, 0.8, 3, 0, 1)
    assert _bytes(state) == before


# ---- the whole series against the offline rule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(0.5, 0.8, 1, 0, 1), (0.5, 0.8, 3, 1, 2), (0.5, 0.8, 9, 5, 4), (0.5, 0.8, 31, 2, 1)])
def test_whole_series_against_find_events_host(spec):
    from anomaly_detection_on_video_amd.events import LiveEventTracker, find_events_host, live_emission_count, resolve_event_spec

    spec = resolve_event_spec(spec)
    rng = np.random.default_rng(spec.smooth)
    lens = [150, 0, 97, 1, 64]
    series = [_noise(rng, n, block=max(3, spec.smooth // 2)) for n in lens]
    tracker = LiveEventTracker(spec, N_CAM, log=64, device=DEV)
    seen, due = np.zeros(N_CAM, dtype=np.int64), [[] for _ in range(N_CAM)]
    for k in range(max(lens)):
        cams = tuple(c for c in range(N_CAM) if k < lens[c])
        tracker.update(cams, torch.from_numpy(np.asarray([series[c][k] for c in cams], dtype=np.float32)).to(DEV))
        emitted = tracker.emitted.cpu().numpy().copy()
        for c in np.flatnonzero(emitted > seen):
            assert emitted[c] == seen[c] + 1  # at most one per update
            due[c].append(k + 1)              # the sample count that emitted it
        seen = emitted
    tracker.finish(range(N_CAM))
    d = tracker.drain()
    assert d.lost.tolist() == [0] * N_CAM and (d.generation == 0).all()
    got = d.events.numpy()
    want = find_events_host(np.concatenate(series), lens, spec)
    assert_events_equal(got.ev_int, got.ev_f, got.counts, want.ev_int, want.ev_f, want.counts, str(spec))
    assert len(got) >= 3
    for c in range(N_CAM):  # the emission rule: every event emitted while running came at the stated count
        ends = got.per_video(c).end.tolist()
        assert due[c] == [live_emission_count(e, spec) for e in ends[:len(due[c])]]
        assert all(live_emission_count(e, spec) > lens[c] for e in ends[len(due[c]):])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_tracker_refusals():
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.events import LiveEventTracker

    t = LiveEventTracker((0.5, 0.8, 3), 4, log=2, device=DEV)
    ok = torch.rand((2,), device=DEV)
    for cams, what in (([1, 1], r"duplicate camera ids \[1\]"), ([0, 4], r"camera id 4 is out of range \[0, 4\)"), ([-1, 0], "camera id -1 is out of range"),
                       ([], "an empty list of cameras"), ([0, 1.5], "camera id 1.5 is not a host integer"), ([0, "1"], "camera id '1' is not a host integer"),
                       (torch.tensor([0, 1]), "cams must be a sequence of host integers, got a Tensor"),
                       (torch.tensor([0, 1], device=DEV), ".*got a Tensor"), (np.array([0, 1]), ".*got a ndarray"), (3, "cams must be a sequence of camera ids, got int")):
        for call, name in ((lambda: t.update(cams, ok), "update"), (lambda: t.finish(cams), "finish"), (lambda: t.reset(cams), "reset")):
            with pytest.raises(HipExtensionError, match=f"LiveEventTracker.{name}: " + what):
                call()
    for scores, what in ((ok.cpu(), "scores is on 'cpu'"), (ok.double(), "scores must be torch.float32"), (torch.rand((3,), device=DEV), r"scores must be \(2,\), got \(3,\)"),
                         (torch.rand((2, 2), device=DEV)[:, 0], "scores must be contiguous"), ([0.5, 0.5], "scores must be a torch.float32 tensor")):
        with pytest.raises(HipExtensionError, match="live_events_update: " + what):
            t.update([0, 1], scores)
    with pytest.raises(HipExtensionError, match=r"live_events_update: scores must be \(4,\), got \(2,\)"):
        t.update([0, 1], ok, by_camera=True)
    assert t.samples_host == (0,) * 4 and not t.samples.any() and not t.emitted.any()  # a refused call moves nothing
    t.cameras.host[2] = (1 << 31) - 1
    with pytest.raises(HipExtensionError, match=r"LiveEventTracker.update: cameras \[2\] have fed 2\^31 - 1 samples"):
        t.update([0, 2], ok)
    assert t.samples_host[0] == 0
    ids = t.cameras.ids(t.cameras.check((0, 1), "x"))
    t.update((0, 1), ok)
    # the id tensor of a repeated camera set is reused
    assert t.cameras.ids(t.cameras.check((0, 1), "x")) is ids and t.cameras.ids(t.cameras.check([0, 1], "x")) is ids


def test_launch_wrapper_refusals():
    from anomaly_detection_on_video_amd import _lib, mil_ops
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    state = mil_ops.live_events_state(N_CAM, 3, K, DEV)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    sc = torch.rand((2,), device=DEV)
    before = _bytes(state)

    def call(scores=sc, cam_ids=ids, smooth=3, low=0.5, high=0.8, merge_gap=0, min_len=1, by_camera=False, mode=0, **swap):
        return mil_ops.live_events_update(scores, cam_ids, {**state, **swap}, low, high, smooth, merge_gap, min_len, by_camera, mode)

    cases = [
        (lambda: call(ring=state["ring"].cpu()), "ring is on 'cpu'"), (lambda: call(ring=state["ring"].double()), "ring must be torch.float32"),
        (lambda: call(smooth=5), r"ring must be \(n_cam, smooth = 5\), got \(5, 3\)"),
        (lambda: call(ring=torch.zeros((3, N_CAM), device=DEV).t()), "ring must be contiguous"),
        (lambda: call(samples=state["samples"].int()), "samples must be torch.int64, got torch.int32"),
        (lambda: call(samples=state["samples"][:4]), r"samples must be \(5,\), got \(4,\)"),
        (lambda: call(cand_int=state["cand_int"].long()), "cand_int must be torch.int32"),
        (lambda: call(cand_int=state["cand_int"][:, :4]), r"cand_int must be \(5, 5\), got \(5, 4\)"),
        (lambda: call(cand_int=torch.zeros((5, N_CAM), dtype=torch.int32, device=DEV).t()), "cand_int must be contiguous"),
        (lambda: call(cand_peak=state["cand_peak"].cpu()), "cand_peak is on 'cpu'"),
        (lambda: call(cand_sum=state["cand_sum"].float()), "cand_sum must be torch.float64, got torch.float32"),
        (lambda: call(alert=state["alert"].long()), "alert must be torch.int32"), (lambda: call(open_start=state["open_start"][:3]), r"open_start must be \(5,\)"),
        (lambda: call(log_int=state["log_int"].long()), "log_int must be torch.int32"),
        (lambda: call(log_int=torch.zeros((N_CAM, K, 6), dtype=torch.int32, device=DEV)), r"log_int must be \(5, \*, 4\), got \(5, 4, 6\)"),
        (lambda: call(log_f=torch.zeros((N_CAM, K + 1, 2), device=DEV)), r"log_f must be \(5, 4, 2\), got \(5, 5, 2\)"),
        (lambda: call(emitted=state["emitted"].int()), "emitted must be torch.int64"),
        (lambda: call(cam_ids=ids.long()), "cam_ids must be torch.int32, got torch.int64"), (lambda: call(cam_ids=ids.cpu()), "cam_ids is on 'cpu'"),
        (lambda: call(cam_ids=[0, 1]), "cam_ids must be a torch.int32 tensor"),
        (lambda: call(scores=sc.cpu()), "scores is on 'cpu'"), (lambda: call(scores=sc.half()), "scores must be torch.float32, got torch.float16"),
        (lambda: call(scores=None), "scores must be a torch.float32 tensor"), (lambda: call(by_camera=True), r"scores must be \(5,\), got \(2,\)"),
        (lambda: call(mode=_lib.LIVE_EVENTS_FINISH), "finish and reset feed no sample: scores must be None"),
        (lambda: call(mode=3), "mode 3 is not LIVE_EVENTS_UPDATE"), (lambda: call(merge_gap=-1), "merge_gap -1 is not an integer"),
        (lambda: call(min_len=0), "min_len 0 is not an integer"), (lambda: call(min_len=1.5), "min_len 1.5 is not an integer"),
        (lambda: mil_ops.live_events_update(sc, ids, {k: v for k, v in state.items() if k != "alert"}, 0.5, 0.8, 3), "state must be a dict of the tensors"),
        # what the entry point itself refuses
        (lambda: call(low=0.9), "low = 0.9 above high = 0.8"), (lambda: call(high=float("inf")), "must be finite"),
        (lambda: call(smooth=4, ring=torch.zeros((N_CAM, 4), device=DEV)), "smooth = 4 is not an odd window"),
    ]
    if torch.cuda.device_count() > 1:
        cases.append((lambda: call(cam_ids=ids.to("cuda:1")), "cam_ids is on cuda:1, the arguments before it are on cuda:0"))
    for fn, what in cases:
        with pytest.raises(HipExtensionError, match="live_events_update.*" + what):
            fn()
    assert _bytes(state) == before  # nothing was launched


# ---- LiveScorer(events=) -------------------------------------------------------------------------------------------------------
NCROPS, CH, W, CAMS = 3, 2048, 5, 3


@pytest.fixture(scope="module")
def scorer():
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    m.load_state_dict(synth_module_state_dict(m), strict=True)
    return m.eval().to(DEV)


def _script(steps=40):
    """[(cams, feats)]: mostly every camera, some steps a subset in another order; the features' scale wanders so that the scores do."""
    g = torch.Generator().manual_seed(21)
    out = []
    for k in range(steps):
        cams = [2, 0] if k % 7 == 3 else [1] if k % 11 == 5 else [0, 1, 2]
        scale = 1.0 + 0.8 * torch.sin(torch.tensor(0.45 * k)) + 0.5 * torch.rand((len(cams), 1, 1), generator=g)
        out.append((cams, (torch.rand((len(cams), NCROPS, CH), generator=g) * scale).to(DEV)))
    return out


@pytest.fixture(scope="module")
def plain_run(scorer):
    """The script through LiveScorer without events: per step the scores' bits, per camera the series of `latest`."""
    from anomaly_detection_on_video_amd.live import LiveScorer

    live = LiveScorer(scorer, CAMS, window=W, ncrops=NCROPS, channels=CH, device=DEV)
    assert live.events is None
    bits, series = [], [[] for _ in range(CAMS)]
    for cams, feats in _script():
        live.push(cams, feats)
        s = live.score(cams)
        bits.append((s.scores.cpu().numpy().tobytes(), s.latest.cpu().numpy().tobytes()))
        latest = live.latest.cpu().numpy()
        for c in cams:
            series[c].append(latest[c])
    return bits, [np.asarray(x, dtype=np.float32) for x in series]


def test_live_scorer_events_are_the_offline_events_of_the_latest_series(scorer, plain_run):
    from anomaly_detection_on_video_amd.events import EventSpec, LiveEventTracker, find_events_host
    from anomaly_detection_on_video_amd.live import LiveScorer

    bits, series = plain_run
    allx = np.concatenate(series)
    assert np.isfinite(allx).all() and np.unique(allx).size > 10
    spec = EventSpec(float(np.quantile(allx, 0.5)), float(np.quantile(allx, 0.8)), smooth=3, merge_gap=1, min_len=2)
    live = LiveScorer(scorer, CAMS, window=W, ncrops=NCROPS, channels=CH, device=DEV, events=spec, event_log=16)
    assert isinstance(live.events, LiveEventTracker) and live.events.log == 16 and live.events.spec == spec
    for k, (cams, feats) in enumerate(_script()):
        live.push(cams, feats)
        s = live.score(cams)
        assert (s.scores.cpu().numpy().tobytes(), s.latest.cpu().numpy().tobytes()) == bits[k], f"step {k}: events= changed the scores"
        assert live.events.samples_host == live.counts_host
        if k == 20:  # scored again without a push: nothing is fed
            emitted = live.events.emitted.clone()
            live.score([0, 1, 2])
            live.score()
            assert live.events.samples_host == live.counts_host and torch.equal(live.events.emitted, emitted)
    assert live.events.samples.tolist() == list(live.counts_host) == [len(x) for x in series]
    live.events.finish(range(CAMS))
    d = live.events.drain()
    got, want = d.events.numpy(), find_events_host(allx, [len(x) for x in series], spec)
    assert_events_equal(got.ev_int, got.ev_f, got.counts, want.ev_int, want.ev_f, want.counts, "LiveScorer")
    assert len(got) >= 2 and d.lost.tolist() == [0] * CAMS
    live.reset([0, 1, 2])  # (finish alone leaves the rings' counts ahead of the series: the two are reset together)
    assert live.events.samples_host == live.counts_host == (0, 0, 0)


def test_live_scorer_refuses_a_camera_two_clips_ahead_and_resets_with_the_tracker(scorer):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveScorer

    live = LiveScorer(scorer, CAMS, window=W, ncrops=NCROPS, channels=CH, device=DEV, events=(0.0, 0.0, 1, 0, 1))
    f = torch.rand((CAMS, NCROPS, CH), device=DEV)
    live.push([0, 1, 2], f)
    live.push([1], f[:1])
    before = (live.latest.clone(), live.events.samples.clone())
    with pytest.raises(HipExtensionError, match=r"LiveScorer.score: cameras \[1\] are more than one clip ahead of their event series"):
        live.score()
    with pytest.raises(HipExtensionError, match=r"cameras \[1\] are more than one clip ahead"):
        live.score([1, 2])
    assert torch.equal(live.latest.isnan(), before[0].isnan()) and torch.equal(live.events.samples, before[1])  # nothing was launched
    live.score([2, 0])  # the others go on; only they are fed
    assert live.events.samples_host == (1, 0, 1)
    live.reset([1])
    assert live.counts_host == (1, 0, 1) and live.events.state["cand_int"][:, 4].tolist() == [0, 1, 0]
    live.push([1], f[:1])
    live.score()
    assert live.events.samples_host == live.counts_host == (1, 1, 1)
    assert live.events.alert.tolist() == [1, 1, 1] and live.events.open_start.tolist() == [0, 0, 0]  # (scores lie in [0, 1]: all >= 0)
    live.reset([0, 2])  # the open candidates are dropped, nothing is emitted
    assert live.events.alert.tolist() == [0, 1, 0] and not live.events.emitted.any()
    assert live.events.state["cand_int"][:, 4].tolist() == [1, 1, 1]


def test_steady_state_step_with_events_dispatches_no_torch_arithmetic(scorer):
    from anomaly_detection_on_video_amd.live import LiveScorer
    from test_hip_strict import AtenAudit

    cams = [0, 2, 3]
    live = LiveScorer(scorer, 4, window=W, ncrops=NCROPS, channels=CH, device=DEV, events=(0.2, 0.6, 9, 1, 2))
    g = torch.Generator().manual_seed(11)
    feats = [torch.rand((3, NCROPS, CH), generator=g).to(DEV) for _ in range(W + 2)]
    for f in feats[:W + 1]:
        live.push(cams, f)
        warm = live.score(cams)  # (lazily built operands; the id and length vectors of this camera set)
    with AtenAudit() as audit:
        live.push(cams, feats[W + 1])
        s = live.score(cams)
    assert audit.arithmetic() == {}, f"torch arithmetic on the live step: {audit.arithmetic()}"
    assert "_to_copy" not in audit.ops and "copy_" not in audit.ops, audit.ops
    assert s.lens == (W,) * 3 and not torch.equal(s.scores, warm.scores)
    assert live.events.samples.tolist() == list(live.events.samples_host) == [W + 2, 0, W + 2, W + 2]
