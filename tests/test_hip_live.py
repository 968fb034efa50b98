"""GPU tests of live scoring (csrc/live.hip, mil_ops.ring_push / ring_windows / crop_mean_last, live.LiveScorer): the ring and its
windows bit for bit against the numpy model of tests/_live_ref.py, the scores against MGFNForVideoAnomalyDetection.score_padded on
a batch built with torch.cat from the pushed features (exact) and against the per-camera pass, what cannot leak (history, NaN),
the ATen audit of a steady-state step, every refusal, and step_frames."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from _live_ref import RingRef, scripted_counts, scripted_pushes
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_module_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3  # the project's parity contract (tests/test_hip_val_batch.py)
NCROPS, N_CAM, CH = 3, 6, 2048


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32) if torch.is_tensor(t) else np.asarray(t).view(np.int32)


@pytest.fixture(scope="module")
def scorer():
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    m.load_state_dict(synth_module_state_dict(m), strict=True)
    return m.eval().to(DEV)


# ---- push and windows: bits only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 5, 8])
@pytest.mark.parametrize("C", [5, 13, 130, 2048])
def test_push_and_windows_bit_for_bit(C, W):
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd.live import LiveScorer

    live = LiveScorer(None, N_CAM, window=W, ncrops=NCROPS, channels=C, device=DEV)
    ref = RingRef(N_CAM, NCROPS, W, C)
    for cams, feats in scripted_pushes(W, NCROPS, C):  # (every step but the first few is a push to a subset)
        live.push(cams, torch.from_numpy(feats).to(DEV))
        ref.push(cams, feats)
    # the whole ring: the pushed rows and their magnitudes, and no byte of a camera outside a push
    assert np.array_equal(_bits(live.ring), _bits(ref.ring))
    assert live.counts.tolist() == list(live.counts_host) == ref.counts.tolist() == scripted_counts(W)
    ring_before = live.ring.clone()
    for cams in (list(range(N_CAM)), [5, 0, 3], [2]):
        ids = torch.tensor(cams, dtype=torch.int32, device=DEV)
        for tmax in sorted({W, max(1, W - 2)}):
            dst = torch.full((len(cams), NCROPS, tmax, C + 1), float("nan"), device=DEV)
            again = dst.clone()
            mil_ops.ring_windows(live.ring, live.counts, ids, dst)
            want = ref.windows(cams, tmax)
            assert np.array_equal(_bits(dst), _bits(want)), (cams, tmax)
            for v, n in enumerate(ref.lens(cams, tmax)):
                assert torch.isnan(dst[v, :, n:]).all()  # the tails; a camera at count 0 is all tail
            mil_ops.ring_windows(live.ring, live.counts, ids, again)  # two runs, the same bits
            assert np.array_equal(_bits(again), _bits(dst))
    assert torch.equal(live.ring, ring_before)
    # ids outside [0, n_cam), given on the device: no byte of the state changes
    counts_before = live.counts.clone()
    bad = torch.tensor([-1, N_CAM], dtype=torch.int32, device=DEV)
    mil_ops.ring_push(torch.ones((2, NCROPS, C), device=DEV), bad, live.ring, live.counts)
    assert np.array_equal(_bits(live.ring), _bits(ring_before)) and torch.equal(live.counts, counts_before)
    dst = torch.full((2, NCROPS, W, C + 1), float("nan"), device=DEV)
    mil_ops.ring_windows(live.ring, live.counts, bad, dst)
    assert torch.isnan(dst).all()


def test_crop_mean_last_writes_only_the_listed_cameras():
    from anomaly_detection_on_video_amd import mil_ops

    nb, tmax = 3, 7
    rows = torch.rand((nb * NCROPS, tmax, 1), device=DEV)
    lens = torch.tensor([7, 1, 4], dtype=torch.int32, device=DEV)
    ids = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
    offs = torch.tensor([0, tmax, 2 * tmax], dtype=torch.int64, device=DEV)
    dense = mil_ops.crop_mean_scatter(rows, lens, offs, torch.zeros((nb * tmax,), device=DEV), nb, NCROPS).view(nb, tmax)
    latest = torch.full((N_CAM,), -1.0, device=DEV)
    mil_ops.crop_mean_last(rows, lens, ids, latest, NCROPS)
    assert latest.tolist() == [float(dense[1, 0]), -1.0, float(dense[2, 3]), -1.0, float(dense[0, 6]), -1.0]


# ---- scores --------------------------------------------------------------------------------------------------------------------
class _Run:
    """A LiveScorer after the scripted pushes, with every camera's clips kept in the order they came."""

    def __init__(self, scorer, W):
        from anomaly_detection_on_video_amd.live import LiveScorer

        self.W = W
        self.live = LiveScorer(scorer, N_CAM, window=W, ncrops=NCROPS, channels=CH, device=DEV)
        self.pushed = [[] for _ in range(N_CAM)]
        for cams, feats in scripted_pushes(W, NCROPS, CH, seed=1, spread=0.5):
            feats = torch.from_numpy(np.abs(feats)).to(DEV)  # (non-negative, as pooled ReLU features are)
            self.live.push(cams, feats)
            for i, c in enumerate(cams):
                self.pushed[c].append(feats[i])

    def explicit(self, cams, fill=0.0):
        """(padded batch, lens) of the listed cameras' windows from the pushed features: torch.cat, and add_magnitude_np for the
        last channel (code of the parent commit, numpy's bits)."""
        from anomaly_detection_on_video_amd import mil_ops

        lens = [min(len(self.pushed[c]), self.W) for c in cams]
        video = torch.full((len(cams), NCROPS, max(lens), CH + 1), fill, device=DEV)
        for v, (c, n) in enumerate(zip(cams, lens)):
            clips = torch.cat([f.unsqueeze(0) for f in self.pushed[c][-n:]])  # (n, ncrops, C)
            video[v, :, :n] = mil_ops.add_magnitude_np(clips, transpose=True)
        return video, lens


_RUNS = {}


def _run(scorer, W):
    if W not in _RUNS:
        _RUNS[W] = _Run(scorer, W)
    return _RUNS[W]


@pytest.fixture(scope="module", params=[1, 5, 8])
def run(request, scorer):
    return _run(scorer, request.param)


@pytest.fixture(scope="module", params=[5, 8])
def run_topk(request, scorer):
    """The runs whose windows the per-camera pass takes: scorer(video=...) selects its top k = 3 clips and refuses T < 3, so at
    W = 1 that reference does not exist (there score_padded on the explicit batch is the check)."""
    return _run(scorer, request.param)


def _cam_sets(W):
    sets = [None, [4, 5], [5, 1, 3]]       # everything that has a clip (mixed lengths); two cameras after wrap-around; any order
    if W > 2:
        sets.append([1, 2])                # Tmax = W - 1 < W
    return sets


def test_scores_equal_score_padded_on_the_explicit_batch(run, scorer):
    W, live = run.W, run.live
    for cams in _cam_sets(W):
        s = live.score(cams)
        listed = tuple(c for c in range(N_CAM) if scripted_counts(W)[c] > 0) if cams is None else tuple(cams)
        assert s.cams == listed
        video, lens = run.explicit(listed)
        assert s.lens == tuple(lens) and s.scores.shape == (len(listed), max(lens)) and s.latest.shape == (len(listed),)
        want = scorer.score_padded(video, lens)
        assert np.array_equal(_bits(s.scores), _bits(want)), (W, cams)
        for v, n in enumerate(lens):
            assert float(s.latest[v]) == float(s.scores[v, n - 1]) == float(live.latest[listed[v]])
            assert not s.scores[v, n:].any()
    assert live.counts.tolist() == list(live.counts_host)


def test_latest_is_nan_for_a_camera_never_scored(scorer):
    from anomaly_detection_on_video_amd.live import LiveScorer

    live = LiveScorer(scorer, 4, window=5, ncrops=NCROPS, channels=CH, device=DEV)
    assert torch.isnan(live.latest).all()
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        live.push([0, 1, 3], torch.rand((3, NCROPS, CH), generator=g).to(DEV))
    s = live.score([3, 1])
    got = live.latest.cpu()
    assert torch.isnan(got[0]) and torch.isnan(got[2])  # camera 0 has clips but was not listed; camera 2 has none
    assert float(got[3]) == float(s.latest[0]) == float(s.scores[0, 2]) and float(got[1]) == float(s.latest[1])
    live.reset([3])
    assert live.counts.tolist() == list(live.counts_host) == [3, 3, 0, 0]
    got = live.latest.cpu()
    assert torch.isnan(got[3]) and float(got[1]) == float(s.latest[1])
    assert live.score().cams == (0, 1)


def test_steady_state_is_the_unbatched_pass_bit_for_bit(run_topk, scorer):
    """Every listed length = W: score_padded's own guarantee carries over."""
    run, cams = run_topk, [3, 4, 5]
    s = run.live.score(cams)
    video, lens = run.explicit(cams)
    assert lens == [run.W] * len(cams)
    with torch.no_grad():
        want = scorer(video=video).scores.squeeze(-1)
    assert np.array_equal(_bits(s.scores), _bits(want))


def test_mixed_lengths_match_the_per_camera_pass(run_topk, scorer):
    """Lengths 1, W - 1, W, W, W in one pass; camera 1's single clip is below the per-camera pass's k = 3 (see run_topk)."""
    run = run_topk
    s = run.live.score()
    video, lens = run.explicit(s.cams)
    assert lens == [1, run.W - 1, run.W, run.W, run.W]
    for v, n in enumerate(lens):
        if n < scorer.k:
            continue
        with torch.no_grad():
            one = scorer(video=video[v:v + 1, :, :n].contiguous()).scores.reshape(-1)
        err = rel_err(s.scores[v, :n].cpu(), one.cpu())
        print(f"W={run.W} camera {s.cams[v]} len={n}: rel err vs the per-camera pass {err:.3e}")
        assert err < TOL


def test_history_cannot_leak(run, scorer):
    """Camera 5 saw 2W + 3 clips: it scores as in a fresh LiveScorer given only the last W of every listed camera."""
    from anomaly_detection_on_video_amd.live import LiveScorer

    W, cams = run.W, [3, 4, 5]
    old = run.live.score(cams)
    fresh = LiveScorer(scorer, N_CAM, window=W, ncrops=NCROPS, channels=CH, device=DEV)
    for t in range(W):
        fresh.push(cams, torch.stack([run.pushed[c][-W + t] for c in cams]))
    new = fresh.score(cams)
    assert new.lens == old.lens == (W,) * 3
    assert np.array_equal(_bits(new.scores), _bits(old.scores)) and np.array_equal(_bits(new.latest), _bits(old.latest))


@pytest.mark.parametrize("W", [5, 8])
def test_nan_stays_in_its_camera(scorer, W):
    from anomaly_detection_on_video_amd.live import LiveScorer

    g = torch.Generator().manual_seed(W)
    clips = [torch.rand((3, NCROPS, CH), generator=g).to(DEV) for _ in range(W)]
    results = []
    for poison in (False, True):
        live = LiveScorer(scorer, 3, window=W, ncrops=NCROPS, channels=CH, device=DEV)
        for t, f in enumerate(clips):
            if poison and t == 2:
                f = f.clone()
                f[1, 1, 77] = float("nan")
            cams = [0, 1, 2] if t > 0 else [0, 1]  # camera 2 is one clip short: mixed lengths
            live.push(cams, f[: len(cams)])
        results.append(live.score())
    clean, bad = results
    assert clean.lens == bad.lens == (W, W, W - 1) and torch.isfinite(clean.scores).all()
    assert torch.isnan(bad.scores[1]).all() and torch.isnan(bad.latest[1])
    for v in (0, 2):
        assert np.array_equal(_bits(bad.scores[v]), _bits(clean.scores[v])) and float(bad.latest[v]) == float(clean.latest[v])


# ---- the steady state dispatches nothing ---------------------------------------------------------------------------------------
def test_steady_state_step_dispatches_no_torch_arithmetic(scorer):
    from anomaly_detection_on_video_amd.live import LiveScorer
    from test_hip_strict import AtenAudit

    W, cams = 5, [0, 2, 3]
    live = LiveScorer(scorer, 4, window=W, ncrops=NCROPS, channels=CH, device=DEV)
    g = torch.Generator().manual_seed(11)
    feats = [torch.rand((3, NCROPS, CH), generator=g).to(DEV) for _ in range(W + 2)]
    for f in feats[:W]:
        live.push(cams, f)
    live.push(cams, feats[W])
    warm = live.score(cams)  # (lazily built operands; the id and length vectors of this camera set)
    with AtenAudit() as audit:
        live.push(cams, feats[W + 1])
        s = live.score(cams)
    assert audit.arithmetic() == {}, f"torch arithmetic on the live step: {audit.arithmetic()}"
    assert "_to_copy" not in audit.ops and "copy_" not in audit.ops, audit.ops
    assert s.lens == (W,) * 3 and not torch.equal(s.scores, warm.scores)
    assert live.counts.tolist() == list(live.counts_host) == [W + 2, 0, W + 2, W + 2]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_live_scorer_refusals(scorer):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveScorer

    with pytest.raises(HipExtensionError, match="window = 0 is not an integer >= 1"):
        LiveScorer(scorer, 4, window=0, ncrops=NCROPS, device=DEV)
    with pytest.raises(HipExtensionError, match=r"4 cameras x 3 crops x 5 clips = 60 rows is above the scorer's row limit of 59"):
        LiveScorer(scorer, 4, window=5, ncrops=NCROPS, device=DEV, max_rows=59)
    with pytest.raises(HipExtensionError, match="200000 cameras x 10 crops x 32 clips"):  # (refused before anything is allocated)
        LiveScorer(scorer, 200_000)
    live = LiveScorer(scorer, 4, window=5, ncrops=NCROPS, channels=CH, device=DEV)
    ok = torch.rand((2, NCROPS, CH), device=DEV)
    for cams, what in (([1, 1], r"duplicate camera ids \[1\]"), ([0, 4], r"camera id 4 is out of range \[0, 4\)"), ([-1, 0], "camera id -1 is out of range"),
                       ([], "an empty list of cameras"), ([0, 1.5], "camera id 1.5 is not a host integer")):
        with pytest.raises(HipExtensionError, match="LiveScorer.push: " + what):
            live.push(cams, ok)
        with pytest.raises(HipExtensionError, match="LiveScorer.score: " + what):
            live.score(cams)
    for feats in (torch.rand((3, NCROPS, CH), device=DEV), torch.rand((2, NCROPS + 1, CH), device=DEV), torch.rand((2, NCROPS, CH - 1), device=DEV),
                  torch.rand((2, NCROPS * CH), device=DEV)):
        with pytest.raises(HipExtensionError, match=r"LiveScorer.push: feats must be \(2, 3, 2048\)"):
            live.push([0, 1], feats)
    with pytest.raises(HipExtensionError, match="ring_push: feats is on 'cpu'"):
        live.push([0, 1], ok.cpu())
    with pytest.raises(HipExtensionError, match="ring_push: feats must be torch.float32"):
        live.push([0, 1], ok.double())
    with pytest.raises(HipExtensionError, match="ring_push: feats must be contiguous"):
        live.push([0, 1], torch.rand((NCROPS, 2, CH), device=DEV).transpose(0, 1))
    assert live.counts.tolist() == list(live.counts_host) == [0] * 4  # a refused push moves nothing
    with pytest.raises(HipExtensionError, match="LiveScorer.score: no camera has a clip yet"):
        live.score()
    live.push([0, 1], ok)
    with pytest.raises(HipExtensionError, match=r"LiveScorer.score: cameras \[2\] have no clip yet"):
        live.score([0, 2])
    scorer.train()  # score_padded's own refusals pass through
    try:
        with pytest.raises(HipExtensionError, match="eval mode only"):
            live.score()
    finally:
        scorer.eval()
    assert live.score().cams == (0, 1)


def test_launch_wrapper_refusals():
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    W, C = 4, 6
    ring = torch.zeros((N_CAM, NCROPS, W, C + 1), device=DEV)
    counts = torch.zeros((N_CAM,), dtype=torch.int64, device=DEV)
    feats = torch.rand((2, NCROPS, C), device=DEV)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    dst = torch.zeros((2, NCROPS, W, C + 1), device=DEV)
    rows = torch.rand((2 * NCROPS, W, 1), device=DEV)
    lens = torch.tensor([W, 1], dtype=torch.int32, device=DEV)
    latest = torch.zeros((N_CAM,), device=DEV)
    cases = [
        (lambda: mil_ops.ring_push(feats.cpu(), ids, ring, counts), "ring_push: feats is on 'cpu'"),
        (lambda: mil_ops.ring_push(feats, ids.cpu(), ring, counts), "ring_push: cam_ids is on 'cpu'"),
        (lambda: mil_ops.ring_push(feats, ids, ring.cpu(), counts), "ring_push: ring is on 'cpu'"),
        (lambda: mil_ops.ring_push(feats, ids, ring, counts.cpu()), "ring_push: counts is on 'cpu'"),
        (lambda: mil_ops.ring_push(feats.half(), ids, ring, counts), "ring_push: feats must be torch.float32, got torch.float16"),
        (lambda: mil_ops.ring_push(feats, ids.long(), ring, counts), "ring_push: cam_ids must be torch.int32, got torch.int64"),
        (lambda: mil_ops.ring_push(feats, ids, ring, counts.int()), "ring_push: counts must be torch.int64, got torch.int32"),
        (lambda: mil_ops.ring_push(feats[:, :, :5], ids, ring, counts), r"ring_push: feats must be \(\*, 3, 6\), got \(2, 3, 5\)"),
        (lambda: mil_ops.ring_push(feats, ids[:1], ring, counts), r"ring_push: cam_ids must be \(2,\), got \(1,\)"),
        (lambda: mil_ops.ring_push(feats, ids, ring, counts[:5]), r"ring_push: counts must be \(6,\), got \(5,\)"),
        (lambda: mil_ops.ring_push(feats, ids, ring[:, :, :, :6], counts), "ring_push: ring must be contiguous"),
        (lambda: mil_ops.ring_push(feats, ids, torch.zeros((N_CAM, W, NCROPS, C + 1), device=DEV).transpose(1, 2), counts), "ring_push: ring must be contiguous"),
        (lambda: mil_ops.ring_push(feats, torch.zeros((2, 2), dtype=torch.int32, device=DEV)[:, 0], ring, counts), "ring_push: cam_ids must be contiguous"),
        (lambda: mil_ops.ring_windows(ring, counts, ids, dst.cpu()), "ring_windows: dst is on 'cpu'"),
        (lambda: mil_ops.ring_windows(ring, counts, ids, dst.double()), "ring_windows: dst must be torch.float32"),
        (lambda: mil_ops.ring_windows(ring, counts, ids, dst[:, :, :, :C]), r"ring_windows: dst must be \(\*, 3, \*, 7\), got \(2, 3, 4, 6\)"),
        (lambda: mil_ops.ring_windows(ring, counts, ids, dst[:, :, :2]), "ring_windows: dst must be contiguous"),
        (lambda: mil_ops.ring_windows(ring, counts[:3], ids, dst), r"ring_windows: counts must be \(6,\)"),
        (lambda: mil_ops.ring_windows(ring, counts, ids[:1], dst), r"ring_windows: cam_ids must be \(2,\)"),
        (lambda: mil_ops.ring_windows(ring[0], counts, ids, dst), r"ring_windows: ring must be \(\*, \*, \*, \*\)"),
        (lambda: mil_ops.crop_mean_last(rows.cpu(), lens, ids, latest, NCROPS), "crop_mean_last: scores is on 'cpu'"),
        (lambda: mil_ops.crop_mean_last(rows, lens.long(), ids, latest, NCROPS), "crop_mean_last: lens must be torch.int32"),
        (lambda: mil_ops.crop_mean_last(rows[:5], lens, ids, latest, NCROPS), r"crop_mean_last: scores must be \(6, Tmax\)"),
        (lambda: mil_ops.crop_mean_last(rows, lens, ids[:1], latest, NCROPS), r"crop_mean_last: cam_ids must be \(2,\)"),
        (lambda: mil_ops.crop_mean_last(rows, lens, ids, latest.double(), NCROPS), "crop_mean_last: latest must be torch.float32"),
        (lambda: mil_ops.crop_mean_last(rows, lens, ids, latest, 0), "crop_mean_last: ncrops 0 is not a positive integer"),
    ]
    if torch.cuda.device_count() > 1:
        cases.append((lambda: mil_ops.ring_push(feats, ids.to("cuda:1"), ring, counts), "ring_push: cam_ids is on cuda:1, the arguments before it are on cuda:0"))
    for call, what in cases:
        with pytest.raises(HipExtensionError, match=what):
            call()
    assert not ring.any() and not counts.any() and not dst.any() and not latest.any()  # nothing was launched
    big = torch.zeros((1, 1, 1, 8194), device=DEV)
    with pytest.raises(HipExtensionError, match="ring_push: C=8193 above 8192"):
        mil_ops.ring_push(torch.zeros((1, 1, 8193), device=DEV), ids[:1], big, counts[:1].clone())


# ---- from frames ---------------------------------------------------------------------------------------------------------------
def test_step_frames_is_forward_frames_push_score(scorer):
    from anomaly_detection_on_video_amd.i3d import I3Res50
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveScorer

    backbone = I3Res50()
    backbone.load_state_dict(synth_i3d_state_dict())
    backbone = backbone.eval().to(DEV)
    cams, W = [2, 0], 5
    rng = np.random.default_rng(3)
    steps = [torch.from_numpy(rng.integers(0, 256, size=(2 * 16, 256, 340, 3), dtype=np.uint8)).to(DEV) for _ in range(2)]
    a = LiveScorer(scorer, 3, window=W, ncrops=2, channels=CH, device=DEV)
    b = LiveScorer(scorer, 3, window=W, ncrops=2, channels=CH, device=DEV)
    for frames in steps:
        got = a.step_frames(backbone, frames, cams, crops="center_flip")
        feats = backbone.forward_frames(frames, 0, 4, crops="center_flip").reshape(2, 2, CH)
        b.push(cams, feats)
        want = b.score(cams)
        assert got.cams == want.cams == (2, 0) and got.lens == want.lens
        assert np.array_equal(_bits(got.scores), _bits(want.scores)) and np.array_equal(_bits(got.latest), _bits(want.latest))
    assert torch.equal(a.ring, b.ring) and a.counts_host == b.counts_host == (2, 0, 2)
    with pytest.raises(HipExtensionError, match="LiveScorer.step_frames: 10 crops, the rings hold 2"):
        a.step_frames(backbone, steps[0], cams)
    with pytest.raises(HipExtensionError, match=r"LiveScorer.step_frames: frames_u8 must be \(32, FH, FW, 3\)"):
        a.step_frames(backbone, steps[0][:16], cams, crops="center_flip")
