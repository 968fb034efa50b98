"""The training step under a per-step learning-rate schedule and a fused gradient-norm clip: advhip_adam_multi_dev_f32 (lr and the
gradient scale read from device memory) and advhip_grad_norm_multi_f32 against the by-value advhip_adam_multi_f32 and float64
references, optim.HipAdam(device_lr=, max_grad_norm=) under train_graph.GraphedTrainStep (ONE capture, bit-for-bit the eager loop),
and runner.Trainer with `runner.optimizer.schedule` / `runner.optimizer.max_grad_norm` configured."""
import glob
import os
import warnings

import numpy as np
import pytest
import torch

from anomaly_detection_on_video_amd.weights import synth_module_state_dict
from test_oracle_golden import mgfn_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------ kernel level
BASE_SIZES = [1, 3, 4095, 4096, 4097, 8193, (1 << 20) + 5]  # one element .. 257 blocks of 4096, vector bodies and scalar tails
FILL_SIZES = [1, 3, 5, 4095, 4097, 130]
COUNTS = [1, 80, 81, 130]  # 80 tensors fill one by-value Adam item table; 81 and 130 take a second launch
B1, B2, EPS, WD, LR = 0.9, 0.999, 1e-8, 5e-4, 1e-3 * 0.77


def sizes_for(count):
    if count == 1:
        return [4097]
    return (BASE_SIZES + [FILL_SIZES[i % len(FILL_SIZES)] for i in range(count)])[:count]


def offset_view(n, gen, scale=1.0, positive=False, shift=0):
    """n fp32 values on the device; shift = 1: a view that starts one element into its storage, so it is not 16-byte aligned."""
    t = torch.randn(n + shift, generator=gen) * scale
    if positive:
        t = t.abs()
    return t.to(DEV)[shift:]


def adam_set(count, seed=0):
    """{p, g, m, v}: lists of tensors, steps: one flat fp32 counter tensor.  Tensor 1 has every operand off 16-byte alignment, tensor 2
    (where there is one) only its gradient: the scalar path, taken for two different reasons."""
    gen = torch.Generator().manual_seed(seed)
    out = {k: [] for k in "pgmv"}
    for i, n in enumerate(sizes_for(count)):
        all_off, g_off = int(i == 1 or count == 1), int(i == 2)
        out["p"].append(offset_view(n, gen, shift=all_off))
        out["g"].append(offset_view(n, gen, scale=1.0 + i % 3, shift=max(all_off, g_off)))
        out["m"].append(offset_view(n, gen, scale=0.1, shift=all_off))
        out["v"].append(offset_view(n, gen, scale=0.01, positive=True, shift=all_off))
    out["steps"] = torch.full((count,), 3.0, device=DEV)
    assert any(t.data_ptr() % 16 for t in out["g"])
    return out


def clone_set(s, g=None):
    c = {k: [t.clone() if t.data_ptr() % 16 == 0 else torch.cat([t.new_zeros(1), t])[1:] for t in s[k]] for k in "pmv"}
    c["g"] = s["g"] if g is None else g  # (gradients are read only)
    c["steps"] = s["steps"]
    for k in "pmv":  # (clones keep their tensor's alignment class)
        assert [t.data_ptr() % 16 == 0 for t in c[k]] == [t.data_ptr() % 16 == 0 for t in s[k]]
    return c


def adam_items(s):
    from anomaly_detection_on_video_amd import _lib

    arr = (_lib.AdamItem * len(s["p"]))()
    for i, it in enumerate(arr):
        it.param, it.grad, it.exp_avg, it.exp_avg_sq, it.step, it.n = (s["p"][i].data_ptr(), s["g"][i].data_ptr(), s["m"][i].data_ptr(),
                                                                        s["v"][i].data_ptr(), s["steps"][i].data_ptr(), s["p"][i].numel())
    return arr


def adam_by_value(s, lr=LR):
    from anomaly_detection_on_video_amd import _lib

    _lib.check(_lib.load().advhip_adam_multi_f32(adam_items(s), len(s["p"]), lr, B1, B2, EPS, WD, _lib.stream(s["p"][0])))
    return s


def adam_dev(s, lr_dev, scale_dev):
    from anomaly_detection_on_video_amd import _lib

    _lib.check(_lib.load().advhip_adam_multi_dev_f32(adam_items(s), len(s["p"]), lr_dev.data_ptr(), None if scale_dev is None else scale_dev.data_ptr(),
                                                     B1, B2, EPS, WD, _lib.stream(s["p"][0])))
    return s


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_same_bits(a, b, what):
    for k in "pmv":
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(bits(x), bits(y)), f"{what}: {k}[{i}] (n = {x.numel()}) differs"


@pytest.mark.parametrize("count", COUNTS)
def test_dev_adam_equals_the_by_value_launch_bit_for_bit(count):
    """Same lr as a device double: with a null scale, and with scale 1.0, p / m / v are the by-value call's, bit for bit; with scale
    0.37 they are the by-value call's on torch's `g.mul(0.37)` (the scale is ONE separately rounded fp32 product)."""
    s = adam_set(count)
    before = clone_set(s)
    ref = adam_by_value(clone_set(s))
    lr_dev = torch.tensor([LR], device=DEV, dtype=torch.float64)
    assert_same_bits(adam_dev(clone_set(s), lr_dev, None), ref, "null scale")
    assert_same_bits(adam_dev(clone_set(s), lr_dev, torch.tensor([1.0], device=DEV)), ref, "scale 1.0")
    assert not torch.equal(bits(ref["p"][0]), bits(before["p"][0]))  # (the update did something)
    scaled_g = [g.mul(0.37) if g.data_ptr() % 16 == 0 else torch.cat([g.new_zeros(1), g.mul(0.37)])[1:] for g in s["g"]]
    ref37 = adam_by_value(clone_set(s, g=scaled_g))
    got37 = adam_dev(clone_set(s), lr_dev, torch.tensor([0.37], device=DEV))
    assert_same_bits(got37, ref37, "scale 0.37")
    assert not torch.equal(bits(ref37["p"][-1]), bits(ref["p"][-1]))
    # the lr is read at run time: another value in the same scalar, same launch arguments
    lr_dev.fill_(LR * 0.5)
    assert_same_bits(adam_dev(clone_set(s), lr_dev, None), adam_by_value(clone_set(s), lr=LR * 0.5), "lr changed in place")
    for g, g0 in zip(s["g"], adam_set(count)["g"]):
        assert torch.equal(bits(g), bits(g0))  # gradients are not written


def norm_set(count, seed=1):
    """Tensor 0: a thousand 1e4-magnitude values next to a million 1e-3 ones (an fp32 running sum would lose the small ones);
    tensor 1: 1e20-magnitude values, whose squares overflow fp32, on an unaligned view; then the ragged sizes."""
    gen = torch.Generator().manual_seed(seed)
    big = torch.randn((1 << 20) + 5, generator=gen) * 1e-3
    big[:1000] = torch.randn(1000, generator=gen) * 1e4
    out = [big.to(DEV)]
    if count > 1:
        out.append(offset_view(4097, gen, scale=1e20, shift=1))
    for i in range(2, count):
        out.append(offset_view((BASE_SIZES[:-1] + FILL_SIZES)[i % 12], gen, scale=1.0 + i % 5, shift=int(i % 7 == 3)))
    return out


def grad_norm(tensors, max_norm, partials=None):
    from anomaly_detection_on_video_amd import _lib

    need = sum((t.numel() + 4095) // 4096 for t in tensors)
    partials = torch.full((need,), float("nan"), device=DEV, dtype=torch.float64) if partials is None else partials
    out = torch.full((2,), float("nan"), device=DEV)
    arr = (_lib.NormItem * len(tensors))()
    for it, t in zip(arr, tensors):
        it.grad, it.n = t.data_ptr(), t.numel()
    _lib.check(_lib.load().advhip_grad_norm_multi_f32(arr, len(tensors), float(max_norm), partials.data_ptr(), partials.numel(), out.data_ptr(),
                                                      out.data_ptr() + 4, _lib.stream(tensors[0])))
    return out.cpu(), partials


def torch_scale(norm_f32: torch.Tensor, max_norm: float) -> torch.Tensor:
    """clip_grad_norm_'s factor as torch computes it (torch/nn/utils/clip_grad.py), on the fp32 CPU tensor."""
    return torch.clamp(max_norm / (norm_f32 + 1e-6), max=1.0)


def ulps_apart(a: np.float32, b: np.float32) -> int:
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# (240 tensors fill one item table of the norm kernel: 241 and 485 take two and three launches)
@pytest.mark.parametrize("count", [1, 2, 80, 130, 241, 485])
def test_grad_norm_against_float64_and_torchs_scale(count):
    tensors = norm_set(count)
    want = np.float32(np.sqrt(sum(float((t.cpu().numpy().astype(np.float64) ** 2).sum()) for t in tensors)))
    max_norm = 1.0
    out, partials = grad_norm(tensors, max_norm)
    print(f"count {count}: norm {out[0].item()!r}, float64 reference {want!r}, scale {out[1].item()!r}")
    assert np.isfinite(out[0].item()) and not torch.isnan(partials).any()
    # double accumulation in any order is far inside half an fp32 ulp of the sum: only the final rounding can differ
    assert ulps_apart(out[0].numpy(), want) <= 1
    assert torch.equal(bits(out[1:]), bits(torch_scale(out[0:1], max_norm))) and 0.0 < out[1].item() < 1.0
    again, partials2 = grad_norm(tensors, max_norm)
    assert torch.equal(bits(again), bits(out)) and torch.equal(partials.view(torch.int64), partials2.view(torch.int64))
    # more room than needed is fine, less is refused before anything is launched
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    if partials.numel() > 1:
        with pytest.raises(HipExtensionError, match="partial sums"):
            grad_norm(tensors, max_norm, partials=partials[:-1])


def test_grad_norm_below_the_limit_gives_scale_one_and_non_finite_values_pass_through():
    gen = torch.Generator().manual_seed(5)
    tensors = [offset_view(n, gen, scale=0.01) for n in (3, 4097, 130)]
    out, _ = grad_norm(tensors, 10.0)
    assert 0.0 < out[0].item() < 10.0 and out[1].item() == 1.0
    want = np.float32(np.sqrt(sum(float((t.cpu().numpy().astype(np.float64) ** 2).sum()) for t in tensors)))
    assert ulps_apart(out[0].numpy(), want) <= 1
    # a norm just above the limit: the factor is torch's, not 1
    just_below = float(out[0]) * 0.999
    out, _ = grad_norm(tensors, just_below)
    assert 0.99 < out[1].item() < 1.0 and torch.equal(bits(out[1:]), bits(torch_scale(out[0:1], just_below)))
    tensors[1][4000] = float("inf")
    out, _ = grad_norm(tensors, 10.0)
    assert out[0].item() == float("inf") and out[1].item() == 0.0
    tensors[2][7] = float("nan")
    out, _ = grad_norm(tensors, 10.0)
    assert np.isnan(out[0].item()) and np.isnan(out[1].item())  # (the clamp does not swallow the NaN)
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(HipExtensionError, match="max_norm"):
            grad_norm(tensors, bad)


@pytest.mark.parametrize("poison", ["nan", "inf"])
def test_non_finite_gradients_behave_as_clip_grad_norm_and_adam_on_the_cpu(poison):
    """One NaN element: NaN norm, NaN scale, every updated parameter NaN.  One inf element: inf norm, scale 0, that element NaN and
    all others updated with g = 0 plus weight decay.  The NaN pattern of the parameters is that of torch.nn.utils.clip_grad_norm_
    followed by torch.optim.Adam on CPU copies."""
    from anomaly_detection_on_video_amd.optim import HipAdam

    gen = torch.Generator().manual_seed(9)
    sizes = sizes_for(81)
    cpu_p = [torch.randn(n, generator=gen).requires_grad_() for n in sizes]
    grads = [torch.randn(n, generator=gen) for n in sizes]
    grads[6][123457] = float(poison)
    hip_p = [p.detach().to(DEV).requires_grad_() for p in cpu_p]
    for a, b, g in zip(cpu_p, hip_p, grads):
        a.grad, b.grad = g.clone(), g.to(DEV)
    torch.nn.utils.clip_grad_norm_(cpu_p, 2.0)
    torch.optim.Adam(cpu_p, lr=1e-3, weight_decay=5e-4).step()
    opt = HipAdam(hip_p, lr=1e-3, weight_decay=5e-4, max_grad_norm=2.0)
    opt.step()
    assert (np.isnan if poison == "nan" else np.isinf)(opt.grad_norm.item())
    n_nan = 0
    for i, (a, b, g) in enumerate(zip(cpu_p, hip_p, grads)):
        got, want = torch.isnan(b.detach().cpu()), torch.isnan(a.detach())
        assert torch.equal(got, want), i
        n_nan += int(got.sum())
        assert torch.equal(bits(b.grad.cpu()), bits(g))  # p.grad is not rewritten (torch's is: scaled in place)
        if poison == "inf" and i != 6:
            assert torch.allclose(b.detach().cpu(), a.detach(), rtol=1e-5, atol=1e-7), i
    assert n_nan == (sum(sizes) if poison == "nan" else 1)


# ------------------------------------------------------------------------------ step level
@pytest.fixture(scope="module")
def batches():
    """Four (4, 10, 32, 2049) inputs, made once and only read (a 12-step run cycles through them)."""
    return [mgfn_inputs(4, 32, 40 + i).to(DEV) for i in range(4)]


LABELS = lambda: (torch.ones(2, device=DEV), torch.zeros(2, device=DEV))  # (abnormal, normal)


def make(**adam):
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection
    from anomaly_detection_on_video_amd.optim import HipAdam

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    m.load_state_dict(synth_module_state_dict(m))
    m = m.to(DEV).train()
    ones = torch.ones(2, 32, device=DEV)
    m.injected_keep = (ones, ones)
    return m, HipAdam(m.parameters(), lr=1e-3, weight_decay=5e-4, **adam)


def assert_same_training_state(a, b):
    (m_a, opt_a), (m_b, opt_b) = a, b
    for (k, x), (_, y) in zip(m_a.state_dict().items(), m_b.state_dict().items()):
        assert torch.equal(x, y), k
    for pa, pb in zip(m_a.parameters(), m_b.parameters()):
        sa, sb = opt_a.state[pa], opt_b.state[pb]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and float(sa["step"]) == float(sb["step"])


def run_steps(step, opt, batches, n, lrs=None, after=None):
    al, nl = LABELS()
    losses, marks = [], []
    for i in range(n):
        if lrs is not None:
            for g in opt.param_groups:
                g["lr"] = lrs[i]
        losses.append(float(step(batches[i % len(batches)], al, nl)))
        marks.append((step.captures, step.graph is not None))
        if after is not None:
            after(i)
    return losses, marks


def test_lr_changed_every_step_keeps_one_graph_and_equals_the_eager_loop(batches):
    """Twelve steps, another lr each: with HipAdam(device_lr=True) the step is captured ONCE and replayed under every lr, and its
    losses, parameters, moments and step counts are those of the plain eager loop with a default HipAdam given the same floats
    (which, graphed, would end eager after MAX_CAPTURES re-captures).  Also driven by torch's LambdaLR."""
    from anomaly_detection_on_video_amd.train_graph import GraphedTrainStep

    lrs = [1e-3 * 0.9 ** k for k in range(12)]  # (LambdaLR below computes base_lr * lmbda(k): the same doubles)
    assert len(set(lrs)) == 12
    m_e, opt_e = make()
    losses_e, _ = run_steps(GraphedTrainStep(m_e, opt_e, eager_steps=1 << 30), opt_e, batches, 12, lrs)
    m_g, opt_g = make(device_lr=True)
    step = GraphedTrainStep(m_g, opt_g, eager_steps=3)
    losses_g, marks = run_steps(step, opt_g, batches, 12, lrs)
    assert marks == [(0, False)] * 3 + [(1, True)] * 9 and step.replays == 9, marks
    assert losses_g == losses_e, (losses_g, losses_e)
    assert_same_training_state((m_e, opt_e), (m_g, opt_g))
    assert float(opt_g.state[next(m_g.parameters())]["step"]) == 12.0 and opt_g._lr_dev.item() == lrs[-1]
    # the same schedule from torch.optim.lr_scheduler: it writes group["lr"], sync_lr() carries it to the device
    m_s, opt_s = make(device_lr=True)
    sched = torch.optim.lr_scheduler.LambdaLR(opt_s, lambda k: 0.9 ** k)
    step_s = GraphedTrainStep(m_s, opt_s, eager_steps=3)

    def tick(_i):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (a replayed step does not go through the Python optimizer.step() LambdaLR counts)
            sched.step()

    losses_s, marks_s = run_steps(step_s, opt_s, batches, 12, after=tick)
    assert marks_s == marks and losses_s == losses_e
    assert_same_training_state((m_e, opt_e), (m_s, opt_s))
    # a default HipAdam under the same schedule: re-captured on every change, eager for good after MAX_CAPTURES (what device_lr removes)
    m_d, opt_d = make()
    step_d = GraphedTrainStep(m_d, opt_d, eager_steps=3)
    run_steps(step_d, opt_d, batches, 12, lrs)
    assert step_d.captures == GraphedTrainStep.MAX_CAPTURES and step_d.graph is None


def test_fused_clip_graphed_equals_eager_and_equals_prescaled_gradients(batches):
    from anomaly_detection_on_video_amd.train_graph import GraphedTrainStep

    clip = 1e-3  # (far below any gradient norm of this loss: every step is clipped, asserted below)
    al, nl = LABELS()
    norms = []
    m_e, opt_e = make(max_grad_norm=clip)
    first = {}

    def after_eager(i):
        g64 = np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in m_e.parameters() if p.grad is not None))
        norms.append((opt_e.grad_norm.item(), g64))
        if i == 0:
            first["params"] = [p.detach().clone() for p in m_e.parameters()]
            first["scale"] = opt_e._norm_out[1].clone()

    losses_e, _ = run_steps(GraphedTrainStep(m_e, opt_e, eager_steps=1 << 30), opt_e, batches, 6, after=after_eager)
    for got, g64 in norms:
        print(f"grad_norm {got!r}, float64 norm of p.grad {g64!r}")
        assert got > clip and ulps_apart(np.float32(got), np.float32(g64)) <= 1  # (p.grad still holds the unclipped gradient)
    m_g, opt_g = make(max_grad_norm=clip)
    step = GraphedTrainStep(m_g, opt_g, eager_steps=3)
    losses_g, marks = run_steps(step, opt_g, batches, 6)
    assert marks == [(0, False)] * 3 + [(1, True)] * 3 and losses_g == losses_e, (marks, losses_g, losses_e)
    assert_same_training_state((m_e, opt_e), (m_g, opt_g))
    assert opt_g.grad_norm.item() == norms[-1][0]
    # one step: a default HipAdam on gradients pre-multiplied by the scale (torch's order: g.mul_(coef), then the optimizer)
    m_p, opt_p = make()
    assert 0.0 < first["scale"].item() < 1.0
    opt_p.register_step_pre_hook(lambda *_a: [p.grad.mul_(first["scale"]) for p in m_p.parameters() if p.grad is not None] and None)
    GraphedTrainStep(m_p, opt_p, eager_steps=1 << 30)(batches[0], al, nl)
    for i, (a, b) in enumerate(zip(first["params"], m_p.parameters())):
        assert torch.equal(bits(a), bits(b.detach())), i


def test_a_clip_that_never_bites_equals_the_unclipped_run(batches):
    from anomaly_detection_on_video_amd.train_graph import GraphedTrainStep

    m_u, opt_u = make()
    losses_u, _ = run_steps(GraphedTrainStep(m_u, opt_u, eager_steps=1 << 30), opt_u, batches, 4)
    m_c, opt_c = make(max_grad_norm=1e30)
    losses_c, _ = run_steps(GraphedTrainStep(m_c, opt_c, eager_steps=2), opt_c, batches, 4)
    assert losses_c == losses_u
    assert_same_training_state((m_u, opt_u), (m_c, opt_c))
    assert opt_c._norm_out[1].item() == 1.0 and 0.0 < opt_c.grad_norm.item() < 1e30


def test_scheduled_clipped_step_dispatches_no_torch_arithmetic(batches, monkeypatch):
    """The ATen audit of tests/test_hip_strict.py on a training step with both features on: the lr upload is a `fill_`, the clip is
    inside the HIP launches -- nothing of torch's clip_grad_norm_ chain (norms, stack, clamp, foreach-mul) is dispatched."""
    from anomaly_detection_on_video_amd import mgfn_ops
    from test_hip_strict import AtenAudit

    monkeypatch.setattr(mgfn_ops, "STRICT", True)
    al, nl = LABELS()
    model, opt = make(device_lr=True, max_grad_norm=1e-3)
    model.injected_keep = None

    def train_step():
        opt.zero_grad(set_to_none=True)
        model(video=batches[0], abnormal_labels=al, normal_labels=nl).loss.backward()
        opt.step()

    train_step()  # (the warm step: scalars and buffers are created here)
    for g in opt.param_groups:
        g["lr"] = 7e-4
    before = model.fc.weight.detach().clone()
    with AtenAudit() as audit:
        train_step()
    torch.cuda.synchronize()
    assert opt._lr_dev.item() == 7e-4 and opt.grad_norm.item() > 1e-3 and not torch.equal(model.fc.weight.detach(), before)
    assert audit.ops.get("fill_", 0) >= 1
    allowed = {"add", "add_", "native_dropout", "_foreach_add_"}
    extra = {k: v for k, v in audit.arithmetic().items() if k not in allowed}
    assert extra == {}, f"torch arithmetic in the training step: {extra} (all: {audit.arithmetic()})"
    assert sum(audit.arithmetic().values()) <= 10, audit.arithmetic()
    for forbidden in ("linalg_vector_norm", "_foreach_norm", "_foreach_mul_", "mul_", "mul", "clamp", "clamp_", "div", "div_", "reciprocal", "norm"):
        assert forbidden not in audit.ops, audit.ops


# ------------------------------------------------------------------------------ the trainer
SPEC = {"name": "cosine", "warmup_steps": 2, "min_lr_ratio": 0.1}


def _train(tmp, data_dir, tag, extra=()):
    import run

    torch.manual_seed(0)
    return run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=3",
                     "runner.model_config.dropout_rate=0.0",  # (no dropout mask: a resumed run must retrace the uninterrupted one bit for bit)
                     "runner.optimizer.schedule={name: cosine, warmup_steps: 2, min_lr_ratio: 0.1}", "runner.optimizer.max_grad_norm=0.05",
                     f"trainer.callbacks.model_checkpoint.dirpath={tmp / ('ckpt_' + tag)}", "trainer.callbacks.model_checkpoint.every_n_epochs=1",
                     f"trainer.logger.jsonl.path={tmp / (tag + '.jsonl')}", *extra])


def test_trainer_with_schedule_and_fused_clip_one_capture_and_resume(tmp_path):
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips
    from anomaly_detection_on_video_amd.optim import HipAdam, lr_at

    data_dir = write_synthetic_feature_zips(str(tmp_path / "feat"), n_normal=4, n_abnormal=4, n_test=4, seed=1)
    full = _train(tmp_path, data_dir, "full")
    steps = [h for h in full.history if "train_loss" in h]
    total = 3 * 2  # max_epochs x steps per epoch: what a null total_steps resolves to
    assert [h["step"] for h in steps] == [1, 2, 3, 4, 5, 6] and full.schedule_total_steps == total
    for h in steps:
        assert h["lr-Adam"] == lr_at(SPEC, 1e-3, h["step"], total), h
        assert np.isfinite(h["grad_norm"]) and h["grad_norm"] > 0.0 and np.isfinite(h["train_loss"])
    assert len({h["lr-Adam"] for h in steps}) == 5  # (the ramp's last value and the cosine's first are both the base lr)
    g = full.graphed_step
    assert g is not None and g.captures == 1 and g.graph is not None and g.replays == 3  # steps 1-3 eager, 4 captured, 4-6 replayed
    opt = g.optimizer
    assert type(opt) is HipAdam and opt.device_lr and opt.max_grad_norm == 0.05
    # the lr of the LAST step taken (global_step 5) is what the device scalar held when it ran; the one set since is lr_at(6)
    assert opt.param_groups[0]["lr"] == lr_at(SPEC, 1e-3, 6, total)
    found = glob.glob(str(tmp_path / "ckpt_full" / "epoch=0-*.ckpt"))
    assert len(found) == 1, found
    saved = torch.load(found[0], map_location="cpu", weights_only=False)
    assert saved["global_step"] == 2 and saved["hyper_parameters"]["optimizer"]["schedule"] == SPEC
    assert saved["hyper_parameters"]["optimizer"]["max_grad_norm"] == 0.05 and saved["lr_schedulers"] == []
    resumed = _train(tmp_path, data_dir, "resumed", extra=(f"ckpt_path={found[0]}",))
    steps_r = [h for h in resumed.history if "train_loss" in h]
    assert [h["step"] for h in steps_r] == [3, 4, 5, 6]
    assert [(h["lr-Adam"], h["train_loss"], h["grad_norm"]) for h in steps_r] == [(h["lr-Adam"], h["train_loss"], h["grad_norm"]) for h in steps[2:]]
    sd_full, sd_res = full.graphed_step.model.state_dict(), resumed.graphed_step.model.state_dict()
    assert list(sd_full) == list(sd_res)
    for k in sd_full:
        assert torch.equal(sd_full[k], sd_res[k]), k


# ------------------------------------------------------------------------------ refusals that need the GPU
def test_refusals_on_the_device(monkeypatch):
    from anomaly_detection_on_video_amd._lib import HipExtensionError
    from anomaly_detection_on_video_amd.optim import HipAdam
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    # a capture before the eager step that creates the scalars and buffers (the stream reports a capture; nothing is launched)
    for kw in ({"device_lr": True}, {"max_grad_norm": 1.0}):
        p = torch.randn(100, device=DEV, requires_grad=True)
        p.grad = torch.randn(100, device=DEV)
        opt = HipAdam([p], lr=1e-3, **kw)
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
            with pytest.raises(HipExtensionError, match="eager step first"):
                opt.step()
            with pytest.raises(HipExtensionError, match="sync_lr inside a graph capture"):
                opt.sync_lr()
        opt.step()  # the eager step
        assert opt._lr_dev.item() == 1e-3
        if "max_grad_norm" in kw:
            want = np.float32(np.sqrt(float((p.grad.double() ** 2).sum())))
            assert ulps_apart(np.float32(opt.grad_norm.item()), want) <= 1
            # ... after which a parameter the eager step has not seen is refused inside a capture too
            q = torch.randn(10000, device=DEV, requires_grad=True)
            q.grad = torch.randn(10000, device=DEV)
            opt.add_param_group({"params": [q]})
            with monkeypatch.context() as mp:
                mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
                with pytest.raises(HipExtensionError, match="eager step first"):
                    opt.step()
    opt = HipAdam([p], lr=1e-3, device_lr=True)
    opt.param_groups[0]["lr"] = torch.tensor(1e-3)
    with pytest.raises(HipExtensionError, match="tensor learning rate"):
        opt.step()
    # the fused clip with torch's Adam
    net = torch.nn.Linear(4, 4).to(DEV)
    runner = VideoAnomalyDetectionRunner(net, {"learning_rate": 1e-3, "weight_decay": 0.0, "max_grad_norm": 1.0}, {"frames_per_clip": 16})
    assert type(runner.configure_optimizers()[0]) is HipAdam
    monkeypatch.setenv("ADV_HIP_ADAM", "0")
    with pytest.raises(ValueError, match="HipAdam"):
        runner.configure_optimizers()
    monkeypatch.delenv("ADV_HIP_ADAM")
    with pytest.raises(ValueError, match="HipAdam"):
        VideoAnomalyDetectionRunner(net.to(torch.bfloat16), {"learning_rate": 1e-3, "weight_decay": 0.0, "max_grad_norm": 1.0},
                                    {"frames_per_clip": 16}).configure_optimizers()
