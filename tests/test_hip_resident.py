"""GPU tests of the device-resident feature datasets: the magnitude kernel against numpy's bits (tests/_pairwise_ref.py, which
tests/test_resident_host.py holds to np.linalg.norm itself), the resident datasets against FeatureDataset item by item, and a
training run with `data.resident=true` against the same run through the host loaders -- equal, not close."""
import os

import numpy as np
import pytest
import torch

import _pairwise_ref as pw
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1024  # floats behind `out` that must stay untouched

# (a, b, C): n < 8 | one leaf, with and without a tail | the first split | uneven leaves | the golden's shape | the real row |
# a tail behind sixteen leaves | the widest row
SHAPES = [(3, 5, 1), (2, 3, 7), (2, 3, 8), (2, 3, 9), (3, 2, 127), (3, 2, 129), (2, 2, 1000), (10, 32, 48), (2, 10, 2048), (1, 3, 2049),
          (1, 2, 8192)]


def _run_kernel(x: np.ndarray, transpose: bool) -> np.ndarray:
    from anomaly_detection_on_video_amd import mil_ops

    a, b, C = x.shape
    n = a * b * (C + 1)
    buf = torch.full((n + CANARY,), -7.0, device=DEV)
    shape = (b, a, C + 1) if transpose else (a, b, C + 1)
    out = mil_ops.add_magnitude_np(torch.from_numpy(x).to(DEV), transpose=transpose, out=buf[:n].view(shape))
    assert out.data_ptr() == buf.data_ptr()
    host = buf.cpu().numpy()
    assert np.array_equal(host[n:], np.full(CANARY, -7.0, np.float32)), "the kernel wrote behind its output"
    return host[:n].reshape(shape)


def _check(x: np.ndarray):
    for transpose in (False, True):
        got, want = _run_kernel(x, transpose), pw.add_magnitude(x, transpose)
        assert np.array_equal(pw.bits(got[..., :-1]), pw.bits(want[..., :-1])), "the copied channels differ from the input"
        bad = pw.bits(got[..., -1]) != pw.bits(want[..., -1])
        assert not bad.any(), (f"{int(bad.sum())} of {bad.size} magnitudes differ from numpy's bits (transpose={transpose}); first: "
                               f"{got[..., -1][bad][:3]} vs {want[..., -1][bad][:3]}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_magnitude_kernel_has_numpys_bits(shape):
    from anomaly_detection_on_video_amd.weights import synth_tensor

    if shape == (10, 32, 48):  # the reference's own FeatureDataset.add_magnitude output
        x = synth_tensor("addmag", shape, scale=2.0).numpy()
        assert np.array_equal(pw.bits(_run_kernel(x, False)), pw.bits(np.load(os.path.join(GOLDEN, "host.npz"))["addmag"]))
    else:
        x = (np.random.default_rng(sum(shape)).standard_normal(shape) * 3).astype(np.float32)
    _check(x)


def test_magnitude_kernel_zero_inf_nan_rows():
    x = (np.random.default_rng(3).standard_normal((2, 3, 200)) * 3).astype(np.float32)
    x[0, 0] = 0.0
    x[0, 1, 130] = np.inf
    x[1, 0, 199] = np.nan
    x[1, 1, 7] = -np.inf
    want = pw.norm_rows(x)
    assert want[0, 0] == 0.0 and np.isposinf(want[0, 1]) and np.isnan(want[1, 0]) and np.isposinf(want[1, 1])
    _check(x)


def test_wrapper_allocates_and_refuses():
    from anomaly_detection_on_video_amd import _lib, mil_ops

    x = torch.rand(2, 3, 20, device=DEV)
    assert mil_ops.add_magnitude_np(x).shape == (2, 3, 21) and mil_ops.add_magnitude_np(x, transpose=True).shape == (3, 2, 21)
    with pytest.raises(ValueError, match="out must be"):
        mil_ops.add_magnitude_np(x, transpose=True, out=torch.empty(2, 3, 21, device=DEV))
    with pytest.raises(_lib.HipExtensionError, match="C=8193"):
        mil_ops.add_magnitude_np(torch.zeros(1, 1, 8193, device=DEV))


# ------------------------------------------------------------------------------ datasets
def test_resident_datasets_equal_feature_dataset_items(tmp_path):
    from anomaly_detection_on_video_amd.dataset import (ResidentFeatureDataset, ResidentItems, build_feature_dataset,
                                                        write_synthetic_feature_zips)

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=3, n_abnormal=2, n_test=4, channels=64)
    host = build_feature_dataset("train", local_path=d, filename="train.zip", dynamic_load=False)
    res = build_feature_dataset("train", local_path=d, filename="train.zip", resident=DEV)
    assert set(res) == {"normal", "abnormal"}
    for cls, n in (("normal", 3), ("abnormal", 2)):
        r, h = res[cls], host[cls]
        assert isinstance(r, ResidentFeatureDataset) and len(r) == len(h) == n and r.filenames == h.filenames
        assert r.features.shape == (n, 10, 32, 65) and r.features.is_cuda and r.anomaly.is_cuda and r.anomaly.dtype == torch.float32
        for i in range(n):
            item, want = r[i], h[i]
            assert item["feature"].data_ptr() == r.features[i].data_ptr()  # a view
            assert np.array_equal(pw.bits(item["feature"].cpu().numpy()), pw.bits(want["feature"]))
            assert float(item["anomaly"]) == float(want["anomaly"])
        assert np.array_equal(r.anomaly.cpu().numpy(), np.array([h[i]["anomaly"] for i in range(n)]))
    hv = build_feature_dataset("test", local_path=d, filename="test.zip", dynamic_load=False)
    rv = build_feature_dataset("test", local_path=d, filename="test.zip", resident=DEV)
    assert len(rv) == len(hv) == 4 and rv.filenames == hv.filenames and rv.store.is_cuda
    lo, hi = rv.store.data_ptr(), rv.store.data_ptr() + rv.store.numel() * 4
    for i, batch in enumerate(ResidentItems(rv)):
        want = hv[i]
        item = rv[i]
        t = want["feature"].shape[0]
        assert item["feature"].shape == (t, 10, 65) and np.array_equal(pw.bits(item["feature"].cpu().numpy()), pw.bits(want["feature"]))
        assert isinstance(item["label"], np.ndarray) and np.array_equal(item["label"], want["label"]) and item["anomaly"] == want["anomaly"]
        # what validation_step does with the batch lands on the stored memory: no copy, no launch
        assert batch["feature"].shape == (1, t, 10, 65) and not batch["label"].is_cuda and batch["label"].shape == (1, t * 16)
        video = batch["feature"].permute(0, 2, 1, 3).contiguous()
        assert video.data_ptr() == rv.videos[i].data_ptr() == lo + 4 * rv.offsets[i] and video.data_ptr() + video.numel() * 4 <= hi
    assert rv.offsets[-1] == rv.store.numel()


# ------------------------------------------------------------------------------ training
def _train(tmp_path, data_dir, tag, monkeypatch, extra=()):
    import run
    from anomaly_detection_on_video_amd.runner import Trainer, VideoAnomalyDetectionRunner

    seen = {"loaders": [], "fed": [], "runner": None}
    real_loader, real_feed = VideoAnomalyDetectionRunner.train_dataloader, Trainer._feed_graph_inputs

    def train_dataloader(self):
        seen["runner"] = self
        seen["loaders"].append(real_loader(self))
        return seen["loaders"][-1]

    def feed(graphed, batch):
        ok = real_feed(graphed, batch)
        if ok:
            seen["fed"].append((batch[0]["feature"], batch[1]["feature"]))
        return ok

    with monkeypatch.context() as mp:
        mp.setattr(VideoAnomalyDetectionRunner, "train_dataloader", train_dataloader)
        mp.setattr(Trainer, "_feed_graph_inputs", staticmethod(feed))
        torch.manual_seed(0)
        trainer = run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=2",
                            f"trainer.callbacks.model_checkpoint.dirpath={tmp_path / ('ckpt_' + tag)}",
                            f"trainer.logger.jsonl.path={tmp_path / (tag + '.jsonl')}", *extra])
    return trainer, seen


def test_resident_training_equals_the_host_loader_run(tmp_path, monkeypatch):
    from torch.utils.data import DataLoader

    from anomaly_detection_on_video_amd.dataset import ResidentBatches, write_synthetic_feature_zips

    data_dir = write_synthetic_feature_zips(str(tmp_path / "feat"), n_normal=4, n_abnormal=6, n_test=4, seed=2)
    t_host, s_host = _train(tmp_path, data_dir, "host", monkeypatch)
    t_res, s_res = _train(tmp_path, data_dir, "resident", monkeypatch, extra=("data.resident=true",))

    assert all(isinstance(ld, DataLoader) for pair in s_host["loaders"] for ld in pair)
    assert len(s_res["loaders"]) == 2 and all(isinstance(ld, ResidentBatches) for pair in s_res["loaders"] for ld in pair)
    # steps 4-6 are graph replays; step 4 is captured on its batch as given, steps 5 and 6 are fed straight into the graph's
    # input buffers: from the store, as CUDA views whose memory lies inside it
    assert len(s_res["fed"]) == len(s_host["fed"]) == 2
    assert t_res.graphed_step is not None and t_res.graphed_step.captures == 1
    train = s_res["runner"].train_dataset
    for side, cls in ((0, "normal"), (1, "abnormal")):
        store = train[cls].features
        lo, hi = store.data_ptr(), store.data_ptr() + store.numel() * 4
        for fed in s_res["fed"]:
            f = fed[side]
            assert f.is_cuda and f.shape == (2, 10, 32, 2049) and lo <= f.data_ptr() and f.data_ptr() + f.numel() * 4 <= hi
    assert not any(f.is_cuda for fed in s_host["fed"] for f in fed)

    loss = lambda t: [h["train_loss"] for h in t.history if "train_loss" in h]
    vals = lambda t: [(h["valid/rec_auc"], h["valid/pr_auc"]) for h in t.history if "valid/rec_auc" in h]
    assert len(loss(t_host)) == 6 and len(vals(t_host)) == 2 and all(np.isfinite(loss(t_host)))
    print("train_loss host    ", loss(t_host), "\ntrain_loss resident", loss(t_res), "\nvalid host    ", vals(t_host), "\nvalid resident",
          vals(t_res))
    assert loss(t_res) == loss(t_host)
    assert vals(t_res) == vals(t_host)
    sd_host, sd_res = s_host["runner"].model.state_dict(), s_res["runner"].model.state_dict()
    assert list(sd_host) == list(sd_res)
    for k in sd_host:
        assert torch.equal(sd_host[k], sd_res[k]), k


def test_flag_off_keeps_the_host_loaders(tmp_path):
    from torch.utils.data import DataLoader

    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.dataset import FeatureDataset, write_synthetic_feature_zips
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner
    from conftest import REPO

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=2, n_abnormal=2, n_test=2, channels=16)
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={d}", "data.batch_size=2"])
    assert cfg.data.resident is False and cfg.data.resident_max_gib == 32
    runner = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data).to(DEV)
    runner.setup("fit")
    loaders = runner.train_dataloader()
    assert len(loaders) == 2 and all(type(ld) is DataLoader for ld in loaders) and type(runner.val_dataloader()) is DataLoader
    assert isinstance(runner.valid_dataset, FeatureDataset)
