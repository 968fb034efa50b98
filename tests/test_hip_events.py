"""GPU tests of the event kernels (csrc/events.hip) through mil_ops.smooth_scores / mil_ops.score_events, events.find_events,
metrics.FrameAucPlan.events and the runner's `data.events`: the smoothing bit for bit, the event list against the sequential
reference tests/_events_ref.py (integers, peaks and counts exact; means within one fp32 ulp: scores are non-negative and
L <= 2^20, so any order of the float64 sum is within L * 2^-53 <= 2^-33 relative, far below half an fp32 ulp, and the two
rounded results are equal or adjacent), boundary cases with known answers, two large cases, reproducibility, refusals."""
import numpy as np
import pytest
import torch

import _events_ref as ref
from anomaly_detection_on_video_amd import events, metrics, mil_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LENGTHS = [1, 2, 255, 0, 256, 257, 1023, 1024, 1025, 4097]  # one ragged batch: tile edges, more than one block, an empty video


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)  # (a copy: the shared fixtures are read-only)


@pytest.fixture(scope="module")
def ragged():
    """Scores in [0, 1.6] with a NaN, +inf next to -inf and -0.0 in known places (read-only)."""
    rng = np.random.default_rng(11)
    x, _ = ref.random_batch(rng, 1, sum(LENGTHS))
    while x.size != sum(LENGTHS):
        x = np.concatenate([x, ref.random_batch(rng, 1, sum(LENGTHS) - x.size)[0]])
    o = _offsets(LENGTHS)
    x[o[2] + 100] = np.nan       # inside the 255-frame video
    x[o[5] + 7] = np.inf         # the 257-frame video: +inf next to -inf
    x[o[5] + 8] = -np.inf
    x[o[4] + 3] = -0.0           # the 256-frame video
    x[o[0]] = -0.0               # the one-frame video
    x.setflags(write=False)
    return x, o


def _run(x, lengths, spec):
    ev = events.find_events(_dev(x), lengths, spec)
    h = ev.numpy()
    assert ev.ev_int.is_cuda and ev.ev_int.dtype == torch.int32 and ev.ev_f.dtype == torch.float32 and ev.counts.dtype == torch.int32
    return h


def _check(x, lengths, spec, what=""):
    spec = events.resolve_event_spec(spec)
    h = _run(x, lengths, spec)
    ev_int, ev_f, counts, _ = ref.events_ref(x, lengths, spec.low, spec.high, spec.smooth, spec.merge_gap, spec.min_len, fast_smooth=True)
    ref.assert_events_equal(h.ev_int, h.ev_f, h.counts, ev_int, ev_f, counts, what or str(spec))
    return h


@pytest.mark.parametrize("w", [1, 3, 255, 1023])
def test_smoothing_is_exact(ragged, w):
    x, o = ragged
    want = np.concatenate([ref.smooth_ref_fast(x[o[i]:o[i + 1]], w) for i in range(len(LENGTHS))])
    got = mil_ops.smooth_scores(_dev(x), _dev(o), w)
    assert torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(want.view(np.int32))), f"window {w}"
    if w == 1:  # the input's bits, but -0.0
        fixed = np.where(x == 0, np.float32(0), x)
        assert np.array_equal(want.view(np.int32), fixed.view(np.int32))
    out = torch.empty(x.size, device=DEV)
    assert mil_ops.smooth_scores(_dev(x), _dev(o), w, out=out) is out and torch.equal(out.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("spec", [(0.7, 0.9), (0.7, 0.9, 5, 3, 4), (0.5, 0.5, 255, 0, 1), (0.6, 1.0, 9, 40, 30), (0.8, 0.8, 1023, 2, 1)])
def test_events_equal_the_reference_on_the_ragged_batch(ragged, spec):
    x, _ = ragged
    h = _check(x, LENGTHS, spec)
    print(spec, "events", len(h), "counts", h.counts.tolist())


def test_events_equal_the_reference_on_random_batches():
    rng = np.random.default_rng(77)
    total = 0
    for case in range(20):
        x, lengths = ref.random_batch(rng, int(rng.integers(1, 7)), 400)
        if x.size == 0:
            x, lengths = np.zeros(3, np.float32), lengths + [3]
        if case % 4 == 0:
            x[int(rng.integers(0, x.size))] = np.nan
        spec = (0.7, 0.9, int(rng.choice([1, 3, 5, 9])), int(rng.integers(0, 6)), int(rng.integers(1, 8)))
        total += len(_check(x, lengths, spec, f"case {case}"))
    assert total > 20


def test_boundaries():
    lengths = [5, 0, 1, 300, 2]
    n = sum(lengths)
    # every frame active, an unbounded gap: one event per non-empty video, none across a boundary
    h = _check(np.full(n, 0.9, np.float32), lengths, (0.5, 0.8, 1, 10 ** 9, 1))
    assert h.video.tolist() == [0, 2, 3, 4] and h.start.tolist() == [0] * 4 and h.end.tolist() == [5, 1, 300, 2]
    assert h.counts.tolist() == [1, 0, 1, 1, 1] and h.peak_frame.tolist() == [0] * 4  # a constant curve: the peak is at the start
    # ... also with two active ends only, far apart inside each video
    x = np.zeros(n, np.float32)
    o = _offsets(lengths)
    x[o[:-1][np.array(lengths) > 0]] = 0.9
    x[o[1:][np.array(lengths) > 0] - 1] = 0.9
    h = _check(x, lengths, (0.5, 0.8, 1, 10 ** 9, 1))
    assert h.end.tolist() == [5, 1, 300, 2]
    # 64 videos of one frame, every other one active
    x = np.where(np.arange(64) % 2 == 0, 0.9, 0.1).astype(np.float32)
    h = _check(x, [1] * 64, (0.5, 0.8, 3, 4, 1))
    assert len(h) == 32 and h.counts.tolist() == [1, 0] * 32
    # no active frame
    h = _check(np.full(n, 0.1, np.float32), lengths, (0.5, 0.8))
    assert len(h) == 0 and h.counts.tolist() == [0] * 5 and h.ev_int.shape == (0, 4) and h.ev_f.shape == (0, 2)
    # alternating frames, no merging: the capacity bound sum(ceil(L / 2))
    lengths = [7, 1, 0, 2, 1025, 2048]
    x = np.concatenate([np.where(np.arange(l) % 2 == 0, 0.9, 0.1) for l in lengths]).astype(np.float32)
    h = _check(x, lengths, (0.5, 0.8))
    assert len(h) == sum((l + 1) // 2 for l in lengths) and h.counts.tolist() == [(l + 1) // 2 for l in lengths]
    # low == high, -0.0 >= 0.0, min_len one above and equal to an event's length
    x = np.array([0.1, 0.8, 0.8, 0.8, 0.1, -0.0, -1.0], np.float32)
    assert _check(x, [7], (0.8, 0.8, 1, 0, 3)).ev_int.tolist() == [[0, 1, 4, 1]]
    assert len(_check(x, [7], (0.8, 0.8, 1, 0, 4))) == 0
    assert _check(x, [7], (0.0, 0.0)).ev_int.tolist() == [[0, 0, 6, 1]]


def test_large_cases():
    # one event of 300 000 frames inside a 300 001-frame video: the candidate's looped reduction
    n = 300_001
    rng = np.random.default_rng(3)
    x = (0.8 + 0.2 * rng.random(n)).astype(np.float32)
    x[-1] = 0.1
    x[123_457] = x[200_000] = 1.25  # the peak, twice
    h = _run(x, [n], (0.5, 0.9))
    want = events.find_events_host(x, [n], (0.5, 0.9))
    ref.assert_events_equal(h.ev_int, h.ev_f, h.counts, want.ev_int, want.ev_f, want.counts, "300 000-frame event")
    assert h.ev_int.tolist() == [[0, 0, 300_000, 123_457]] and h.peak.tolist() == [1.25]
    exact = np.float32(x[:-1].astype(np.float64).sum() / 300_000)
    assert abs(int(h.mean.view(np.int32)[0]) - int(exact.view(np.int32))) <= 1
    # N = 1024 * 1024 + 5 positions in 3 videos: the third level of the scans
    lengths = [700_000, 5, 1024 * 1024 - 700_000]
    n = sum(lengths)
    x = (0.55 * (1 + np.sin(np.arange(n) / 977.0))).astype(np.float32)  # humps about 6 000 frames apart
    x[700_000 - 2:700_000 + 7] = 1.0  # active across both inner boundaries
    spec = (0.7, 0.8, 5, 100, 2)
    h = _run(x, lengths, spec)
    want = events.find_events_host(x, lengths, spec)
    ref.assert_events_equal(h.ev_int, h.ev_f, h.counts, want.ev_int, want.ev_f, want.counts, "2^20 + 5 positions")
    assert len(h) > 150 and h.counts[1] == 1 and h.ev_int[h.video == 1].tolist()[0][:3] == [1, 0, 5]
    assert (h.end[h.video == 0] <= 700_000).all() and int(h.end[h.video == 0][-1]) == 700_000


def test_two_runs_give_the_same_bits(ragged):
    x, o = ragged
    xd, od = _dev(x), _dev(o)
    ws = mil_ops.score_events_workspace(x.size, len(LENGTHS), DEV)
    runs = []
    for _ in range(2):
        ws.fill_(0xAB)  # the workspace is scratch only
        y = mil_ops.smooth_scores(xd, od, 5)
        ev_int, ev_f, counts = mil_ops.score_events(y, od, 0.7, 0.9, 3, 2, workspace=ws, offsets_host=o)
        runs.append((y.view(torch.int32).clone(), ev_int.clone(), ev_f.view(torch.int32).clone(), counts.clone()))
    assert len(runs[0][1]) > 10
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _plan(windows, stride, seed=0, fpc=16):
    rng = np.random.default_rng(seed)
    span = fpc
    frames = [(n - 1) * (stride or span) + span for n in windows]
    frames[-1] -= 0 if stride is None else 3  # per-frame mode: the last video's labels end inside its last window
    labels = [(rng.random(f) > 0.5).astype(np.float32) for f in frames]
    plan = metrics.FrameAucPlan(labels, windows, fpc, stride, device=DEV)
    scores = [np.clip(rng.random(n) * 1.2, 0, 1).astype(np.float32) for n in windows]
    for i, s in enumerate(scores):
        plan.slot(i).copy_(_dev(s))
    return plan, scores, frames


@pytest.mark.parametrize("stride", [None, 8])
def test_plan_events_equal_the_host_rule(stride):
    windows = [3, 40, 17]
    plan, scores, frames = _plan(windows, stride)
    spec = events.EventSpec(0.5, 0.8, 5, 6, 4)
    before = plan.compute()
    ev = plan.events(spec)
    again = plan.events((0.5, 0.8, 5, 6, 4))  # the cached buffers
    assert plan.compute() == before
    host_frames = [metrics.frame_scores(s, 16, stride, f) for s, f in zip(scores, frames)]
    want = events.find_events_host(np.concatenate(host_frames), frames, spec)
    for got in (ev.numpy(), again.numpy()):
        ref.assert_events_equal(got.ev_int, got.ev_f, got.counts, want.ev_int, want.ev_f, want.counts, f"stride {stride}")
    assert len(want) >= 2 and ev.video.is_cuda
    # the one-video path on the same window scores
    for i, n in enumerate(windows):
        one = events.video_events(plan.slot(i), spec, 16, stride, n_frames=frames[i]).numpy()
        mine = ev.numpy().per_video(i)
        assert np.array_equal(one.ev_int[:, 1:], mine.ev_int[:, 1:]) and np.array_equal(one.ev_f.view(np.int32), mine.ev_f.view(np.int32))
        assert one.counts.tolist() == [len(mine)] and (one.video == 0).all()
    dev_one = ev.per_video(1)
    assert dev_one.start.is_cuda and len(dev_one) == int(want.counts[1])


def test_wrapper_refusals(ragged):
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    x, o = ragged
    xd, od = _dev(x), _dev(o)
    with pytest.raises(HipExtensionError, match="cpu"):
        mil_ops.smooth_scores(torch.from_numpy(np.array(x)), od, 3)
    with pytest.raises(HipExtensionError, match="cpu"):
        mil_ops.score_events(xd, torch.from_numpy(o), 0.5, 0.7)
    with pytest.raises(ValueError, match="fp32"):
        mil_ops.smooth_scores(xd.double(), od, 3)
    with pytest.raises(ValueError, match="int64"):
        mil_ops.score_events(xd, od.int(), 0.5, 0.7)
    with pytest.raises(ValueError, match="window"):
        mil_ops.smooth_scores(xd, od, 4)
    with pytest.raises(ValueError, match="not be the scores"):
        mil_ops.smooth_scores(xd, od, 3, out=xd)
    short = o.copy()
    short[-1] -= 1
    with pytest.raises(ValueError, match="non-decreasing from 0 to N"):
        mil_ops.score_events(xd, _dev(short), 0.5, 0.7)  # (read back from the device)
    with pytest.raises(ValueError, match="non-decreasing from 0 to N"):
        mil_ops.score_events(xd, od, 0.5, 0.7, offsets_host=short)
    down = o.copy()
    down[3] = down[2] - 1
    with pytest.raises(ValueError, match="decreasing step"):
        mil_ops.score_events(xd, od, 0.5, 0.7, offsets_host=down)
    with pytest.raises(ValueError, match="low"):
        mil_ops.score_events(xd, od, 0.9, 0.7)
    with pytest.raises(ValueError, match="min_len"):
        mil_ops.score_events(xd, od, 0.5, 0.7, 0, 0)
    with pytest.raises(ValueError, match="workspace"):
        mil_ops.score_events(xd, od, 0.5, 0.7, workspace=torch.empty(8, device=DEV))
    with pytest.raises(HipExtensionError, match="workspace"):
        mil_ops.score_events(xd, od, 0.5, 0.7, workspace=torch.empty(64, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError, match="sum to"):
        events.find_events(xd, LENGTHS[:-1], (0.5, 0.7))


def _train(tmp_path, data_dir, tag, monkeypatch, extra=()):
    import run
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    seen = {"runner": None, "scores": []}
    real_end = VideoAnomalyDetectionRunner.on_validation_epoch_end

    def on_validation_epoch_end(self):
        seen["runner"] = self
        seen["scores"].append(self.auc_plan.scores.cpu().numpy().copy())
        return real_end(self)

    with monkeypatch.context() as mp:
        mp.setattr(VideoAnomalyDetectionRunner, "on_validation_epoch_end", on_validation_epoch_end)
        torch.manual_seed(0)
        trainer = run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=2",
                            "data.resident=true", "data.device_metrics=true", f"trainer.callbacks.model_checkpoint.dirpath={tmp_path / ('ckpt_' + tag)}",
                            f"trainer.logger.jsonl.path={tmp_path / (tag + '.jsonl')}", *extra])
    return trainer, seen


def test_runner_lists_events_when_asked(tmp_path, monkeypatch):
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips

    data_dir = write_synthetic_feature_zips(str(tmp_path / "feat"), n_normal=4, n_abnormal=6, n_test=5, seed=3)
    t_off, s_off = _train(tmp_path, data_dir, "off", monkeypatch)
    # thresholds from the scores of the run without the key (the two runs compute the same scores): the median and the upper quartile
    low, high = (float(np.quantile(s_off["scores"][-1], q)) for q in (0.5, 0.75))
    spec = events.EventSpec(low, high, 3, 1, 2)
    t_on, s_on = _train(tmp_path, data_dir, "on", monkeypatch,
                        extra=(f"data.events={{low: {low!r}, high: {high!r}, smooth: 3, merge_gap: 1, min_len: 2}}",))
    runner = s_on["runner"]
    assert runner.event_spec == spec and s_off["runner"].event_spec is None and s_off["runner"].last_events is None
    keys = lambda t: [sorted(h) for h in t.history]
    valid_on = [h for h in t_on.history if "valid/rec_auc" in h]
    assert len(valid_on) == 2 and all("valid/n_events" in h for h in valid_on)
    assert not any("valid/n_events" in h for h in t_off.history)
    assert [[k for k in ks if k != "valid/n_events"] for ks in keys(t_on)] == keys(t_off)  # nothing else changes
    assert [h.get("valid/rec_auc") for h in t_on.history] == [h.get("valid/rec_auc") for h in t_off.history]
    plan = runner.auc_plan
    for h, scores in zip(valid_on, s_on["scores"]):
        want = events.find_events_host(np.repeat(scores, plan.items.span), plan.items.frames, spec)
        print("valid/n_events", h["valid/n_events"], "host", len(want))
        assert h["valid/n_events"] == len(want)
    assert np.array_equal(s_on["scores"][-1], s_off["scores"][-1]) and len(want) > 0
    last = runner.last_events.numpy()
    ref.assert_events_equal(last.ev_int, last.ev_f, last.counts, want.ev_int, want.ev_f, want.counts, "runner.last_events")


def test_runner_refuses_events_without_device_metrics(tmp_path):
    import os

    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner
    from conftest import REPO

    def runner(*overrides):
        cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={tmp_path}", *overrides])
        return VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data).to(DEV), cfg

    r, cfg = runner("data.resident=true", "data.events={low: 0.5, high: 0.7}")
    assert cfg.data.events == {"low": 0.5, "high": 0.7}
    with pytest.raises(ValueError, match=r"data\.events needs data\.device_metrics=true"):
        r.setup("fit")
    r, _ = runner("data.resident=true", "data.device_metrics=true", "data.events={low: 0.9, high: 0.7}")
    with pytest.raises(ValueError, match="low=0.9 is above high=0.7"):
        r.setup("fit")
    assert not hasattr(r, "valid_dataset")  # refused before anything is loaded
    r, cfg = runner()
    assert cfg.data.events is None
