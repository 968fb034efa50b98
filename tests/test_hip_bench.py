"""bench.py at N = 1 as the driver runs it: the plain line (headline figure only, `--full` records absent) and
`--dump-outputs`, whose arrays must be what the timed path hands its caller and the same from run to run (seeded inputs)."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import REPO, launch_fresh

pytestmark = pytest.mark.gpu


def _bench(out_dir):
    rep = launch_fresh([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], timeout=600)
    assert rep["rc"] == 0, rep["stderr"][-4000:] + rep["stdout"][-2000:]
    lines = [ln for ln in rep["stdout"].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, rep["stdout"][-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    out = _bench(tmp_path / "a")
    assert out["steps"] == 4 and out["warmup"] == 1 and out["unit"] == "clips/s" and out["dtype"] == "f32" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and abs(out["value"] - 32 * 1e3 / out["ms_per_step"]) < 1e-3 * out["value"] + 0.05
    assert not {"sustained", "mgfn_train_step", "pcie_inclusive", "cpu_baseline"} & set(out)  # --full only
    feats = np.load(tmp_path / "a" / "features.npy")
    assert feats.dtype == np.float32 and feats.shape == (32, 2048) and np.isfinite(feats).all()
    # the timed steps always hold one whole-video scoring pass (bench.stream_start): its scores, T = that video's clip count
    assert out["config"]["videos_scored_rank0"] >= 1
    scores = np.load(tmp_path / "a" / "video_scores.npy")
    assert scores.dtype == np.float32 and scores.shape == (out["config"]["clips_of_videos_scored_rank0"][-1],)
    assert np.isfinite(scores).all()
    _bench(tmp_path / "b")
    assert np.array_equal(np.load(tmp_path / "b" / "features.npy"), feats)
    assert np.array_equal(np.load(tmp_path / "b" / "video_scores.npy"), scores)
