"""GPU tests of `data.device_metrics=true`: two epochs through run.py's trainer on a resident synthetic corpus with the
validation metrics computed on the device and on the host -- the (valid/rec_auc, valid/pr_auc) histories, the losses and the
final weights are equal, not close; the flag needs `data.resident=true`; with it on nothing is appended for the host."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _train(tmp_path, data_dir, tag, monkeypatch, extra=()):
    import run
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    seen = {"runner": None, "outputs": []}
    real_end = VideoAnomalyDetectionRunner.on_validation_epoch_end

    def on_validation_epoch_end(self):
        seen["runner"] = self
        seen["outputs"].append(len(self.validation_step_outputs))
        return real_end(self)

    with monkeypatch.context() as mp:
        mp.setattr(VideoAnomalyDetectionRunner, "on_validation_epoch_end", on_validation_epoch_end)
        torch.manual_seed(0)
        trainer = run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=2",
                            "data.resident=true", f"trainer.callbacks.model_checkpoint.dirpath={tmp_path / ('ckpt_' + tag)}",
                            f"trainer.logger.jsonl.path={tmp_path / (tag + '.jsonl')}", *extra])
    return trainer, seen


def test_device_metrics_run_equals_the_host_metrics_run(tmp_path, monkeypatch):
    from anomaly_detection_on_video_amd import metrics
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips

    data_dir = write_synthetic_feature_zips(str(tmp_path / "feat"), n_normal=4, n_abnormal=6, n_test=5, seed=3)
    t_host, s_host = _train(tmp_path, data_dir, "host", monkeypatch, extra=("data.device_metrics=false",))
    t_dev, s_dev = _train(tmp_path, data_dir, "device", monkeypatch, extra=("data.device_metrics=true",))

    assert s_host["runner"].auc_plan is None and s_host["outputs"] == [5, 5]
    plan = s_dev["runner"].auc_plan
    assert isinstance(plan, metrics.FrameAucPlan) and len(plan) == 5 and plan.scores.is_cuda
    assert s_dev["outputs"] == [0, 0] and s_dev["runner"].validation_step_outputs == []
    assert [int(v.shape[1]) for v in s_dev["runner"].valid_dataset.videos] == plan.items.windows

    loss = lambda t: [h["train_loss"] for h in t.history if "train_loss" in h]
    vals = lambda t: [(h["valid/rec_auc"], h["valid/pr_auc"]) for h in t.history if "valid/rec_auc" in h]
    print("valid host  ", vals(t_host), "\nvalid device", vals(t_dev))
    assert len(vals(t_host)) == 2 and np.isfinite(vals(t_host)).all() and len(loss(t_host)) == 6
    assert vals(t_dev) == vals(t_host)
    assert loss(t_dev) == loss(t_host)
    sd_host, sd_dev = s_host["runner"].model.state_dict(), s_dev["runner"].model.state_dict()
    assert list(sd_host) == list(sd_dev)
    for k in sd_host:
        assert torch.equal(sd_host[k], sd_dev[k]), k


def _runner(tmp_path, *overrides, cls=None):
    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner
    from conftest import REPO

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=2, n_abnormal=2, n_test=2, channels=16)
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={d}", "data.batch_size=2", *overrides])
    return (cls or VideoAnomalyDetectionRunner)(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data).to(DEV), cfg


def test_device_metrics_needs_resident(tmp_path):
    runner, cfg = _runner(tmp_path, "data.device_metrics=true")
    assert cfg.data.device_metrics is True and cfg.data.resident is False
    with pytest.raises(ValueError, match=r"data\.device_metrics=true needs data\.resident=true"):
        runner.setup("fit")
    assert not hasattr(runner, "valid_dataset")  # refused before anything is loaded


def test_flag_defaults_off_and_a_subclass_keeps_its_own_validation(tmp_path):
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    runner, cfg = _runner(tmp_path, "data.resident=true")
    assert cfg.data.device_metrics is False
    runner.setup("fit")
    assert runner.auc_plan is None

    class Mine(VideoAnomalyDetectionRunner):
        def validation_step(self, batch, batch_idx):
            return super().validation_step(batch, batch_idx)

    mine, _ = _runner(tmp_path / "b", "data.resident=true", "data.device_metrics=true", cls=Mine)
    mine.setup("fit")
    assert mine.auc_plan is None  # its outputs feed the host metrics
    stock, _ = _runner(tmp_path / "c", "data.resident=true", "data.device_metrics=true")
    stock.setup("fit")
    assert stock.auc_plan is not None and len(stock.auc_plan) == 2
