"""GPU tests of the camera set the live classes share (live.CameraSet): a LiveScorer with events= and its LiveEventTracker hold
one id vector per camera tuple, the steady push + score on that shared cache still dispatches nothing, and LiveFrames / LiveScorer
refuse an ndarray of ids as the tracker does, with nothing moved."""
import numpy as np
import pytest
import torch

from anomaly_detection_on_video_amd.weights import synth_module_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCROPS, CH, W = 3, 2048, 5  # the shapes of the steady-state tests of test_hip_live.py / test_hip_live_events.py
CAMS = (0, 2, 3)


@pytest.fixture(scope="module")
def scorer():
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    m.load_state_dict(synth_module_state_dict(m), strict=True)
    return m.eval().to(DEV)


def test_scorer_and_tracker_share_one_id_vector_and_the_steady_step_dispatches_nothing(scorer):
    from anomaly_detection_on_video_amd.live import LiveScorer
    from test_hip_strict import AtenAudit

    live = LiveScorer(scorer, 4, window=W, ncrops=NCROPS, channels=CH, device=DEV, events=(0.2, 0.6, 9, 1, 2))
    assert live.events.cameras is not live.cameras and live.events.cameras.ids is live.cameras.ids
    g = torch.Generator().manual_seed(11)
    feats = [torch.rand((3, NCROPS, CH), generator=g).to(DEV) for _ in range(W + 2)]
    for f in feats[:W + 1]:
        live.push(CAMS, f)
        warm = live.score(CAMS)  # (lazily built operands; the id and length vectors of this camera set)
    ids = live.cameras.ids(CAMS)
    assert ids.tolist() == list(CAMS) and live.events.cameras.ids(live.events.cameras.check(CAMS, "x")) is ids
    assert list(live.cameras.ids.items) == [CAMS]  # one upload for both
    with AtenAudit() as audit:
        live.push(CAMS, feats[W + 1])
        s = live.score(CAMS)
    assert audit.arithmetic() == {}, f"torch arithmetic on the live step: {audit.arithmetic()}"
    assert "_to_copy" not in audit.ops and "copy_" not in audit.ops, audit.ops
    assert s.lens == (W,) * 3 and not torch.equal(s.scores, warm.scores)
    assert live.cameras.ids(CAMS) is ids and list(live.cameras.ids.items) == [CAMS]
    # the counts are each owner's own: clips here, samples there
    assert live.counts.tolist() == list(live.counts_host) == [W + 2, 0, W + 2, W + 2]
    assert live.events.samples.tolist() == list(live.events.samples_host) == [W + 2, 0, W + 2, W + 2]
    live.events.finish([2])
    assert live.events.samples_host == (W + 2, 0, 0, W + 2) and live.counts_host == (W + 2, 0, W + 2, W + 2)


def test_live_frames_and_live_scorer_refuse_an_ndarray_of_ids_and_move_nothing(scorer):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.live import LiveFrames, LiveScorer

    hw = (4, 4)
    lf = LiveFrames(4, frame_hw=hw, frames_per_clip=2, device=DEV)
    live = LiveScorer(scorer, 4, window=W, ncrops=NCROPS, channels=CH, device=DEV)
    frames = torch.full((2,) + hw + (3,), 7, dtype=torch.uint8, device=DEV)
    feats = torch.rand((2, NCROPS, CH), device=DEV)
    lf.push([0, 1], frames)
    live.push([0, 1], feats)
    ring_f, ring_s = lf.ring.clone(), live.ring.clone()
    what = "cams must be a sequence of host integers, got a "
    for cams, kind in ((np.array([0, 1]), "ndarray"), (torch.tensor([0, 1]), "Tensor"), (torch.tensor([0, 1], device=DEV), "Tensor")):
        with pytest.raises(HipExtensionError, match="LiveFrames.push: " + what + kind):
            lf.push(cams, frames)
        with pytest.raises(HipExtensionError, match="LiveScorer.push: " + what + kind):
            live.push(cams, feats)
    assert lf.counts.tolist() == list(lf.counts_host) == [1, 1, 0, 0] and torch.equal(lf.ring, ring_f)
    assert live.counts.tolist() == list(live.counts_host) == [1, 1, 0, 0] and torch.equal(live.ring, ring_s)
