"""runner.optimizer.schedule / runner.optimizer.max_grad_norm on the host: optim.lr_at against its formulas written out here (the same
Python doubles, compared with ==), every refusal that needs no GPU, and the checkpoint carrying the spec."""
import math
import os

import pytest
import torch

from conftest import REPO
from anomaly_detection_on_video_amd.optim import HipAdam, check_schedule, lr_at

BASE = 1e-3


def formula(name, s, W, N, r=0.0, milestones=(), gamma=0.1, base=BASE):
    """The issue's rule, restated."""
    if s < W:
        return base * (s + 1) / W
    if name == "constant":
        return base
    if name == "multistep":
        return base * gamma ** len([m for m in milestones if m <= s])
    q = min(1.0, (s - W) / max(1, N - W))
    if name == "linear":
        return base * (r + (1.0 - r) * (1.0 - q))
    return base * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q)))


@pytest.mark.parametrize("name", ["constant", "linear", "cosine", "multistep"])
@pytest.mark.parametrize("W", [0, 5])
@pytest.mark.parametrize("r", [0.0, 0.25])
def test_lr_at_equals_the_formulas(name, W, r):
    N, ms, gamma = 40, [8, 20, 33], 0.5
    spec = {"name": name, "warmup_steps": W, "total_steps": N, "min_lr_ratio": r, "milestones": ms, "gamma": gamma}
    steps = sorted({0, max(W - 1, 0), W, W + 1, (W + N) // 2, N - 1, N, N + 5})
    for s in steps:
        assert lr_at(spec, BASE, s) == formula(name, s, W, N, r, ms, gamma), (name, W, r, s)
    # what the shapes must be, independent of the restated formula
    if W:
        assert lr_at(spec, BASE, 0) == BASE / W and lr_at(spec, BASE, W - 1) == BASE
    if name in ("linear", "cosine"):
        assert lr_at(spec, BASE, W) == BASE
        assert lr_at(spec, BASE, N) == lr_at(spec, BASE, N + 5) == pytest.approx(BASE * r, abs=1e-18)
        lrs = [lr_at(spec, BASE, s) for s in range(W, N + 1)]
        assert all(a >= b for a, b in zip(lrs, lrs[1:])) and lrs[0] > lrs[-1]
    if name == "constant":
        assert all(lr_at(spec, BASE, s) == BASE for s in range(W, N + 6))


def test_multistep_at_and_around_each_milestone():
    ms, gamma = [3, 7, 7, 12], 0.1  # (a milestone listed twice counts twice, as in torch's MultiStepLR)
    spec = {"name": "multistep", "milestones": ms, "gamma": gamma}
    for m in set(ms):
        for s in (m - 1, m, m + 1):
            k = sum(1 for x in ms if x <= s)
            assert lr_at(spec, BASE, s) == BASE * gamma ** k, s
    assert lr_at(spec, BASE, 2) == BASE and lr_at(spec, BASE, 3) == BASE * 0.1 and lr_at(spec, BASE, 6) == BASE * 0.1
    assert lr_at(spec, BASE, 7) == BASE * 0.1 ** 3 and lr_at(spec, BASE, 100) == BASE * 0.1 ** 4
    # with warm-up in front: the ramp wins below W
    warm = dict(spec, warmup_steps=5)
    assert lr_at(warm, BASE, 3) == BASE * 4 / 5 and lr_at(warm, BASE, 5) == BASE * 0.1


def test_total_steps_comes_from_the_spec_or_from_the_caller():
    spec = {"name": "cosine", "warmup_steps": 2}
    assert lr_at(spec, BASE, 6, 12) == formula("cosine", 6, 2, 12)
    assert lr_at(dict(spec, total_steps=8), BASE, 6, 12) == formula("cosine", 6, 2, 8)  # the spec's own wins
    with pytest.raises(ValueError, match="total_steps"):
        lr_at(spec, BASE, 6)
    assert lr_at(None, BASE, 17) == BASE
    assert lr_at({"name": "constant"}, BASE, 17) == BASE  # (needs no N)
    assert check_schedule({"name": "linear"}) == {"name": "linear", "warmup_steps": 0, "total_steps": None, "min_lr_ratio": 0.0, "milestones": [], "gamma": 0.1}


@pytest.mark.parametrize("spec, match", [
    ({"name": "exponential"}, "name"),
    ({}, "name"),
    ({"name": "cosine", "warmup": 3}, "unknown key"),
    ({"name": "cosine", "warmup_steps": -1}, "warmup_steps"),
    ({"name": "cosine", "warmup_steps": 1.5}, "warmup_steps"),
    ({"name": "cosine", "total_steps": -4}, "total_steps"),
    ({"name": "cosine", "min_lr_ratio": 1.5}, "min_lr_ratio"),
    ({"name": "linear", "min_lr_ratio": -0.1}, "min_lr_ratio"),
    ({"name": "multistep", "milestones": [3, -1]}, "milestones"),
    ({"name": "multistep", "milestones": 3}, "milestones"),
    ({"name": "multistep", "gamma": 0.0}, "gamma"),
    ("cosine", "mapping"),
])
def test_schedule_refusals(spec, match):
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    with pytest.raises(ValueError, match=match):
        check_schedule(spec)
    with pytest.raises(ValueError, match=match):
        lr_at(spec, BASE, 0, 10)
    # ... and by the runner's constructor: before any data is loaded
    with pytest.raises(ValueError, match=match):
        VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), {"learning_rate": 1e-3, "weight_decay": 0.0, "schedule": spec}, {"frames_per_clip": 16})
    with pytest.raises(ValueError, match="negative"):
        lr_at({"name": "constant"}, BASE, -1)


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("inf"), float("nan"), True, "1.0"])
def test_max_grad_norm_refusals(bad):
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipAdam([p], lr=1e-3, max_grad_norm=bad)
    with pytest.raises(ValueError, match="runner.optimizer.max_grad_norm"):
        VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), {"learning_rate": 1e-3, "weight_decay": 0.0, "max_grad_norm": bad}, {"frames_per_clip": 16})


def test_hip_adam_refuses_tensors_and_keeps_its_defaults():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="lr"):
        HipAdam([p], lr=torch.tensor(1e-3), device_lr=True)
    with pytest.raises(ValueError, match="max_grad_norm"):
        HipAdam([p], lr=1e-3, max_grad_norm=torch.tensor(1.0))
    opt = HipAdam([p], lr=1e-3)
    assert opt.device_lr is False and opt.max_grad_norm is None and opt.grad_norm is None and not opt.reads_device_scalars
    opt.sync_lr()  # nothing to do, and nothing allocated, for a default HipAdam
    assert opt._lr_dev is None
    opt = HipAdam([p], lr=1e-3, device_lr=True, max_grad_norm=2)
    assert opt.device_lr is True and opt.max_grad_norm == 2.0 and opt.reads_device_scalars
    # the two options are no part of the param groups: state_dict() still interchanges with torch.optim.Adam
    assert "device_lr" not in opt.param_groups[0] and "max_grad_norm" not in opt.param_groups[0]


def test_both_clip_keys_together_raise():
    from anomaly_detection_on_video_amd.runner import check_optimizer_options

    opt = {"learning_rate": 1e-3, "weight_decay": 5e-4, "max_grad_norm": 1.0}
    with pytest.raises(ValueError) as e:
        check_optimizer_options(opt, gradient_clip_val=0.5)
    assert "trainer.cls.gradient_clip_val" in str(e.value) and "runner.optimizer.max_grad_norm" in str(e.value)
    check_optimizer_options(opt, gradient_clip_val=None)  # each alone passes
    check_optimizer_options({"learning_rate": 1e-3, "weight_decay": 5e-4}, gradient_clip_val=0.5)
    check_optimizer_options({"learning_rate": 1e-3, "weight_decay": 5e-4, "max_grad_norm": None}, gradient_clip_val=0.5)


def test_fused_clip_needs_hip_adam():
    """CPU parameters get torch's Adam: the fused clip is refused by name instead of being dropped."""
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    r = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), {"learning_rate": 1e-3, "weight_decay": 0.0, "max_grad_norm": 1.0}, {"frames_per_clip": 16})
    with pytest.raises(ValueError, match="HipAdam"):
        r.configure_optimizers()
    r = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), {"learning_rate": 2e-3, "weight_decay": 0.0, "schedule": {"name": "constant"}}, {"frames_per_clip": 16})
    (opt,) = r.configure_optimizers()  # a schedule with torch's Adam works (the floats are set; it just does not keep a graph)
    assert type(opt) is torch.optim.Adam and opt.param_groups[0]["lr"] == 2e-3


def test_config_keys_compose_and_the_checkpoint_carries_the_spec():
    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner, checkpoint_state

    cfg = compose(os.path.join(REPO, "configs"), "default", ["runner=mgfn"])
    assert cfg.runner.optimizer.schedule is None and cfg.runner.optimizer.max_grad_norm is None
    cfg = compose(os.path.join(REPO, "configs"), "default", ["runner=mgfn", "runner.optimizer.max_grad_norm=0.5",
                                                              "runner.optimizer.schedule.name=cosine", "runner.optimizer.schedule.warmup_steps=3"])
    assert dict(cfg.runner.optimizer.schedule) == {"name": "cosine", "warmup_steps": 3} and cfg.runner.optimizer.max_grad_norm == 0.5
    cfg2 = compose(os.path.join(REPO, "configs"), "default", ["runner=mgfn", "runner.optimizer.schedule={name: multistep, milestones: [4, 9]}"])
    assert dict(cfg2.runner.optimizer.schedule) == {"name": "multistep", "milestones": [4, 9]}
    net = torch.nn.Linear(2, 2)
    runner = VideoAnomalyDetectionRunner(net, cfg.runner.optimizer, {"frames_per_clip": 16})
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    st = checkpoint_state(runner, opt, epoch=2, global_step=11, metrics_={})
    hp = st["hyper_parameters"]["optimizer"]
    assert hp["schedule"] == {"name": "cosine", "warmup_steps": 3} and hp["max_grad_norm"] == 0.5 and float(hp["learning_rate"]) == 1e-3
    assert st["lr_schedulers"] == [] and st["global_step"] == 11  # the lr of a resumed run: lr_at(spec, base, 11, N), nothing else saved
    assert lr_at(hp["schedule"], float(hp["learning_rate"]), st["global_step"], 20) == formula("cosine", 11, 3, 20)
