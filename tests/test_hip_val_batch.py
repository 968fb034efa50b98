"""GPU tests of batched validation (score videos of unequal length in one padded pass): the four temporal operators with row
lengths against their own un-padded calls (exact), the pack / scatter launches, MGFNForVideoAnomalyDetection.score_padded against
the per-video pass and the CPU oracle, its refusals and its ATen audit, and `data.val_batch_videos` through run.py's trainer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err
from anomaly_detection_on_video_amd.weights import synth_module_state_dict, synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3  # the project's parity contract
NAN = float("nan")


def _anyt_core(qkv, heads, scale):
    """The any-T forward core on an un-padded tensor, whatever its T (glance_attention_core sends T = 32 to the one-tile kernel of
    the training shape, whose arithmetic -- the softmax normalised before the second product -- is another one)."""
    from anomaly_detection_on_video_amd import _lib

    c3, b, t = qkv.shape
    out = torch.empty((c3 // 3, b, t), device=qkv.device, dtype=torch.float32)
    _lib.check(_lib.load().advhip_glance_attention_fwd_anyt_f32(_lib.ptr(qkv), _lib.ptr(out), None, heads, b, t, 64, C.c_float(scale), _lib.stream(qkv)))
    return out


def _fp64_core(x, heads, scale):
    """The torch expression of test_glance_attention_core_fwd_bwd_vs_fp64_autograd (tests/test_hip_mgfn.py)."""
    x = x.double().cpu()
    _, b, t = x.shape
    q, k, v = (u.permute(2, 0, 1, 3) for u in x.view(3, heads, 64, b, t).unbind(0))  # (b, h, d, n)
    sim = torch.matmul((q * scale).transpose(-1, -2), k)
    return torch.matmul(v, sim.softmax(dim=-1).transpose(-1, -2)).permute(1, 2, 0, 3).reshape(heads * 64, b, t)


def _with_nan_tails(x, lens, row_dim=1):
    y = x.clone()
    for r, n in enumerate(lens):
        y.select(row_dim, r)[..., n:] = NAN
    return y


def _check_attention(heads, B, T, lens, fp64_below=0):
    """out[:, r, :len] == the un-padded call on row r's first len clips, out[:, r, len:] == 0, NaN behind the ends changes no
    bit.  Rows shorter than `fp64_below` would alone take the other kernel (vector below 256 clips): those against fp64."""
    from anomaly_detection_on_video_amd import mgfn_ops

    scale = 64 ** -0.5
    qkv = synth_tensor(f"vb.qkv{heads}.{B}.{T}", (3 * heads * 64, B, T), scale=1.5).to(DEV)
    with torch.no_grad():
        out = mgfn_ops.glance_attention_core(qkv, heads, 64, scale, lens=lens)
        assert out.shape == (heads * 64, B, T)
        for r, n in enumerate(lens):
            row = qkv[:, r:r + 1, :n].contiguous()
            if n < fp64_below:
                err = rel_err(out[:, r:r + 1, :n].cpu(), _fp64_core(row, heads, scale))
                print(f"T={T} len={n}: rel err vs fp64 {err:.3e}")
                assert err < 1e-5, (r, n)
            elif n == 32:
                # (the un-padded call at T = 32 is the training shape's one-tile kernel: exact against the any-T core the lengths
                # were added to, and that kernel's own bound -- the fp64 test's -- against glance_attention_core)
                assert torch.equal(out[:, r:r + 1, :n], _anyt_core(row, heads, scale)), (r, n)
                assert rel_err(out[:, r:r + 1, :n].cpu(), mgfn_ops.glance_attention_core(row, heads, 64, scale).cpu()) < 1e-5
            else:
                assert torch.equal(out[:, r:r + 1, :n], mgfn_ops.glance_attention_core(row, heads, 64, scale)), (r, n)
            assert not out[:, r, n:].any(), (r, n)
        out_nan = mgfn_ops.glance_attention_core(_with_nan_tails(qkv, lens), heads, 64, scale, lens=lens)
        assert torch.equal(out_nan, out)
        # the lengths as a prebuilt device vector: the same launch
        dev_lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
        assert torch.equal(mgfn_ops.glance_attention_core(qkv, heads, 64, scale, lens=dev_lens), out)


@pytest.mark.parametrize("heads", [1, 2])
def test_attention_with_lengths_vector_regime(heads):
    _check_attention(heads, 6, 40, (1, 31, 32, 33, 40, 7))


@pytest.mark.parametrize("heads", [1, 16])
def test_attention_with_lengths_matrix_pipe_regime(heads):
    _check_attention(heads, 4, 321, (256, 257, 320, 321))


def test_attention_with_lengths_short_rows_in_a_matrix_pipe_launch():
    _check_attention(2, 5, 300, (1, 63, 64, 65, 300), fp64_below=256)


@pytest.mark.parametrize("K", [3, 5])
def test_dwconv_with_lengths(K):
    from anomaly_detection_on_video_amd import mgfn_ops

    Cc, H, rows, T, lens = 128, 2, 5, 9, (1, 2, 3, 8, 9)
    v = synth_tensor(f"vb.dw.v{K}", (Cc, rows, T), scale=1.0).to(DEV)
    w = synth_tensor(f"vb.dw.w{K}", (H, 1, K), scale=0.5).to(DEV)
    b = synth_tensor(f"vb.dw.b{K}", (H,), scale=0.5).to(DEV)
    with torch.no_grad():
        out = mgfn_ops.dwconv_t(v, w, b, lens=lens)
        for r, n in enumerate(lens):
            assert torch.equal(out[:, r:r + 1, :n], mgfn_ops.dwconv_t(v[:, r:r + 1, :n].contiguous(), w, b)), (r, n)
            assert not out[:, r, n:].any()
        assert torch.equal(mgfn_ops.dwconv_t(_with_nan_tails(v, lens), w, b, lens=lens), out)


def test_amp_combine_with_lengths():
    from anomaly_detection_on_video_amd import mgfn_ops

    O, rows, T, lens, width = 64, 4, 6, (1, 2, 5, 6), 9
    conv, to_mag = torch.nn.Conv1d(8, O, 3, padding=1).to(DEV), torch.nn.Conv1d(1, O, 3, padding=1).to(DEV)
    z = synth_tensor("vb.amp.z", (3, O, rows, T), scale=1.0).to(DEV)
    inp = synth_tensor("vb.amp.rows", (rows, T, width), scale=1.0).abs().to(DEV)  # the magnitude is the last column of the input rows
    mag = inp.permute(2, 0, 1)[width - 1:]
    with torch.no_grad():
        assert mgfn_ops.amp_combine_ok(z, conv, to_mag, mag)
        y = mgfn_ops.amp_combine(z, conv, to_mag, mag, 0.1, lens=lens)
        for r, n in enumerate(lens):
            ref = mgfn_ops.amp_combine(z[:, :, r:r + 1, :n].contiguous(), conv, to_mag, mag[:, r:r + 1, :n], 0.1)
            assert torch.equal(y[:, r:r + 1, :n], ref), (r, n)
            assert not y[:, r, n:].any()
        z_nan = _with_nan_tails(z, lens, row_dim=2)
        inp_nan = _with_nan_tails(inp.permute(0, 2, 1).contiguous(), lens, row_dim=0).permute(0, 2, 1).contiguous()
        assert torch.isnan(inp_nan[0, 1:]).all() and torch.equal(inp_nan[0, 0], inp[0, 0])
        assert torch.equal(mgfn_ops.amp_combine(z_nan, conv, to_mag, inp_nan.permute(2, 0, 1)[width - 1:], 0.1, lens=lens), y)
        # all lengths = T: the bits of the call without lengths
        assert torch.equal(mgfn_ops.amp_combine(z, conv, to_mag, mag, 0.1, lens=(T,) * rows), mgfn_ops.amp_combine(z, conv, to_mag, mag, 0.1))


def test_mask_tail_touches_only_the_tails():
    from anomaly_detection_on_video_amd import mgfn_ops

    Cc, rows, T, lens = 70, 5, 9, (1, 9, 3, 8, 2)  # (70 channels: the last workgroup's channel group is partial)
    x = synth_tensor("vb.mask", (Cc, rows, T), scale=1.0).to(DEV)
    y = _with_nan_tails(x, lens)
    with torch.no_grad():
        assert mgfn_ops.mask_tail_(y, lens) is y
    for r, n in enumerate(lens):
        assert torch.equal(y[:, r, :n], x[:, r, :n]) and not y[:, r, n:].any()


def test_pack_and_scatter_round_trip():
    from anomaly_detection_on_video_amd import mil_ops

    ncrops, lens, width, tmax = 3, (1, 4, 7), 5, 7
    videos = [synth_tensor(f"vb.pack{i}", (ncrops, n, width), scale=1.0).to(DEV) for i, n in enumerate(lens)]
    store = torch.cat([torch.full((3,), NAN, device=DEV)] + [v.reshape(-1) for v in videos])  # (the first video does not start the store)
    src, o = [], 3
    for v in videos:
        src.append(o)
        o += v.numel()
    src = torch.tensor(src, dtype=torch.int64, device=DEV)
    dlens = torch.tensor(lens, dtype=torch.int32, device=DEV)
    dst = torch.full((3, ncrops, tmax, width), NAN, device=DEV)
    mil_ops.pack_padded(store, src, dlens, dst)
    for i, n in enumerate(lens):
        assert torch.equal(dst[i, :, :n], videos[i]) and torch.isnan(dst[i, :, n:]).all()  # the rows behind are left as they are
    # the scatter's crop mean: mil_magnitude's `sc`, bit for bit, each video at its own offset of a flat buffer
    scores = dst[..., 0].reshape(3 * ncrops, tmax).contiguous()  # (per-crop "scores" with NaN behind every video's end)
    clean = torch.nan_to_num(scores, nan=0.0)
    feats = torch.ones((3 * ncrops, tmax, 4), device=DEV)
    sc = mil_ops.mil_magnitude(feats, clean, 3, ncrops)[1]
    flat2 = torch.full((13,), -1.0, device=DEV)
    offs2 = torch.tensor([12, 8, 1], dtype=torch.int64, device=DEV)  # (video 2 first, then 1, then 0; element 0 belongs to nobody)
    mil_ops.crop_mean_scatter(scores, dlens, offs2, flat2, 3, ncrops)
    assert torch.equal(flat2[12:13], sc[0, :1]) and torch.equal(flat2[8:12], sc[1, :4]) and torch.equal(flat2[1:8], sc[2, :7])
    assert float(flat2[0]) == -1.0  # nothing else is written


# ---- model level: the default architecture, synthetic weights, mgfn_inputs with 3 crops -----------------------------------------
@pytest.fixture(scope="module")
def scorer():
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    m = MGFNForVideoAnomalyDetection(MGFNConfig())
    sd = synth_module_state_dict(m)
    m.load_state_dict(sd, strict=True)
    return m.eval().to(DEV), sd


@pytest.fixture(scope="module")
def inputs():
    """(4, 3, 300, 2049): four videos of 300 clips x 3 crops, made once -- mgfn_inputs' ten crops of two videos dealt three at a
    time; shorter videos are their first clips (every position carries its own magnitude)."""
    from test_oracle_golden import mgfn_inputs

    x = mgfn_inputs(2, 300, 41)
    return torch.stack([x[0, 0:3], x[0, 3:6], x[0, 6:9], x[1, 0:3]]).contiguous()


def _bucket(inputs, tmax, lens, fill=0.0, swap=None):
    """Videos 0 .. of `inputs` cut to `lens` and padded to tmax with `fill`; `swap` = (slot, source video) puts other data there."""
    video = torch.full((len(lens), 3, tmax, inputs.shape[3]), fill)
    for v, n in enumerate(lens):
        src = swap[1] if swap is not None and swap[0] == v else v
        video[v, :, :n] = inputs[src, :, :n]
    return video.to(DEV)


@pytest.mark.parametrize("T", [57, 300])
@pytest.mark.parametrize("nb", [1, 2])
def test_equal_lengths_are_the_unbatched_pass_bit_for_bit(scorer, inputs, T, nb):
    model, _ = scorer
    video = inputs[:nb, :, :T].contiguous().to(DEV)
    with torch.no_grad():
        want = model(video=video).scores.squeeze(-1)
    got = model.score_padded(video, [T] * nb)
    assert got.shape == (nb, T) and got.dtype == torch.float32 and torch.equal(got, want)


@pytest.fixture(scope="module")
def bucket_results(scorer, inputs):
    """The two buckets of the tail / parity tests, scored once: {tmax: (lens, scores with zero tails)}."""
    model, _ = scorer
    return {tmax: (lens, model.score_padded(_bucket(inputs, tmax, lens), list(lens))) for tmax, lens in ((57, (57, 40, 3)), (300, (300, 256, 17)))}


@pytest.mark.parametrize("tmax", [57, 300])
def test_the_tail_cannot_leak(scorer, inputs, bucket_results, tmax):
    model, _ = scorer
    lens, base = bucket_results[tmax]
    assert base.shape == (3, tmax) and torch.isfinite(base).all()
    for v, n in enumerate(lens):
        assert not base[v, n:].any() and base[v, :n].min() > 0  # returned tails are 0; a real score is a sigmoid
    assert torch.equal(model.score_padded(_bucket(inputs, tmax, lens, fill=NAN), list(lens)), base)
    other = model.score_padded(_bucket(inputs, tmax, lens, fill=NAN, swap=(1, 3)), list(lens))
    assert torch.equal(other[0], base[0]) and torch.equal(other[2], base[2])
    assert not torch.equal(other[1], base[1])


@pytest.mark.parametrize("tmax", [57, 300])
def test_padded_scores_match_the_oracle_and_the_per_video_pass(scorer, inputs, bucket_results, tmax):
    from oracle import mgfn_oracle

    model, sd = scorer
    lens, got = bucket_results[tmax]
    for v, n in enumerate(lens):
        one = inputs[v:v + 1, :, :n].contiguous()
        with torch.no_grad():
            ref = mgfn_oracle.mgfn_forward(one, sd).scores.reshape(-1)
            hip = model(video=one.to(DEV)).scores.reshape(-1)
        e_ref, e_hip = rel_err(got[v, :n].cpu(), ref), rel_err(got[v, :n].cpu(), hip.cpu())
        print(f"Tmax={tmax} len={n}: rel err vs oracle {e_ref:.3e}, vs the per-video HIP pass {e_hip:.3e}")
        assert e_ref < TOL and e_hip < TOL


def test_score_padded_dispatches_no_torch_arithmetic(scorer, inputs):
    from anomaly_detection_on_video_amd.models.mgfn.modeling_mgfn import PaddedLens
    from test_hip_strict import AtenAudit

    model, _ = scorer
    lens = [57, 40, 3]
    video = _bucket(inputs, 57, lens)
    first = model.score_padded(video, lens)  # (lazily built operands: tables, packed / folded weights)
    with AtenAudit() as audit:
        again = model.score_padded(video, lens)
    assert audit.arithmetic() == {}, f"torch arithmetic on the padded scoring path: {audit.arithmetic()}"
    assert torch.equal(again, first)
    pl = PaddedLens(lens, 3, 57, DEV)  # prebuilt lengths: nothing is uploaded either
    with AtenAudit() as audit:
        third = model.score_padded(video, pl)
    assert audit.arithmetic() == {} and "_to_copy" not in audit.ops and "copy_" not in audit.ops, audit.ops
    assert torch.equal(third, first)


def test_score_padded_refusals(scorer, inputs):
    from anomaly_detection_on_video_amd import _lib
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    model, _ = scorer
    video = _bucket(inputs, 8, (8, 5))
    for lens, what in (([8, 0], "outside 1 .. 8"), ([9, 5], "outside 1 .. 8"), ([8], "1 lengths for 2 videos"), ([8, 5, 5], "3 lengths for 2 videos")):
        with pytest.raises(_lib.HipExtensionError, match=what):
            model.score_padded(video, lens)
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        model.score_padded(video.cpu(), [8, 5])
    model.train()
    try:
        with pytest.raises(_lib.HipExtensionError, match="eval mode only"):
            model.score_padded(video, [8, 5])
    finally:
        model.eval()
    # an architecture outside the kernels' shape rules raises, naming the rule, instead of taking a torch expression
    odd = MGFNForVideoAnomalyDetection(MGFNConfig(dims=(64, 128, 1024), depths=(1, 1, 1), dim_head=32)).eval().to(DEV)
    with pytest.raises(_lib.HipExtensionError, match=r"score_padded: .*dim_head != 64.*mgfn_ops\.eligible"):
        odd.score_padded(video, [8, 5])
    with torch.no_grad():
        assert odd(video=video).scores.shape == (2, 8, 1)  # (the per-video path still takes that architecture)


def test_score_videos_and_an_oversize_video(scorer, inputs):
    """The convenience form: five videos, buckets of two; with max_rows below one of them that video goes through the per-video
    pass (its bits)."""
    from anomaly_detection_on_video_amd import val_batch

    model, _ = scorer
    lens = [40, 3, 57, 17, 40]
    videos = [inputs[i % 4, :, :n].contiguous().to(DEV) for i, n in enumerate(lens)]
    with torch.no_grad():
        per_video = [model(video=v.unsqueeze(0)).scores.reshape(-1) for v in videos]
    got = val_batch.score_videos(model, videos, batch_videos=2)
    assert [tuple(g.shape) for g in got] == [(n,) for n in lens]
    for g, w in zip(got, per_video):
        assert rel_err(g.cpu(), w.cpu()) < TOL
    # max_rows = 150 rows: 3 crops x 57 clips = 171 is above it (video 2 alone, through the per-video pass: its bits); the two
    # 40-clip videos together would be 240 rows, so each is a padded bucket of one -- all lengths = Tmax, the per-video bits again
    plan = val_batch.ScoreBatchPlan(videos, 2, max_rows=150)
    assert plan.index_lists == [[1, 3], [0], [4], [2]] and [b.oversize for b in plan.buckets] == [False, False, False, True]
    out = plan.run(model, plan.new_scores())
    for i in (0, 2, 4):
        assert torch.equal(plan.slot(out, i), per_video[i]), i
    for i in (1, 3):
        assert torch.equal(plan.slot(out, i), got[i]), i


# ---- run level: data.val_batch_videos through run.py's trainer --------------------------------------------------------------------
def _train(tmp, data_dir, tag, extra):
    import run
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    seen = {"runner": None, "outputs": [], "steps": 0}
    real_end, real_step = VideoAnomalyDetectionRunner.on_validation_epoch_end, VideoAnomalyDetectionRunner.validation_step

    def on_validation_epoch_end(self):
        seen["runner"] = self
        seen["outputs"] = [dict(o) for o in self.validation_step_outputs]
        return real_end(self)

    def validation_step(self, batch, batch_idx):
        seen["steps"] += 1
        return real_step(self, batch, batch_idx)

    VideoAnomalyDetectionRunner.on_validation_epoch_end = on_validation_epoch_end
    VideoAnomalyDetectionRunner.validation_step = validation_step
    try:
        torch.manual_seed(0)
        trainer = run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=2", "data.resident=true",
                            f"trainer.callbacks.model_checkpoint.dirpath={tmp / ('ckpt_' + tag)}", f"trainer.logger.jsonl.path={tmp / (tag + '.jsonl')}", *extra])
    finally:
        VideoAnomalyDetectionRunner.on_validation_epoch_end = real_end
        VideoAnomalyDetectionRunner.validation_step = real_step
    return trainer, seen


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    """Three two-epoch fits on one synthetic corpus (5 test videos of 20 .. 59 clips): per-video validation, and buckets of 4 with
    the metrics on the device and on the host."""
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips

    tmp = tmp_path_factory.mktemp("val_batch")
    data_dir = write_synthetic_feature_zips(str(tmp / "feat"), n_normal=4, n_abnormal=6, n_test=5, seed=3)
    return {"per_video": _train(tmp, data_dir, "one", ("data.device_metrics=true", "data.val_batch_videos=1")),
            "device": _train(tmp, data_dir, "dev", ("data.device_metrics=true", "data.val_batch_videos=4")),
            "host": _train(tmp, data_dir, "host", ("data.device_metrics=false", "data.val_batch_videos=4"))}


_loss = lambda t: [h["train_loss"] for h in t.history if "train_loss" in h]
_vals = lambda t: [(h["valid/rec_auc"], h["valid/pr_auc"]) for h in t.history if "valid/rec_auc" in h]


def _per_video(runner, flat):
    o = runner.auc_plan.items.window_offsets if runner.auc_plan is not None else runner.score_plan.offsets
    return [flat[int(o[i]):int(o[i + 1])] for i in range(len(runner.valid_dataset.videos))]


@pytest.mark.parametrize("side", ["device", "host"])
def test_batched_validation_run(fits, side):
    from anomaly_detection_on_video_amd import metrics, val_batch

    (t_one, s_one), (t_b, s_b) = fits["per_video"], fits[side]
    r_one, r_b = s_one["runner"], s_b["runner"]
    assert r_one.score_plan is None and s_one["steps"] == 10  # the default: one validation_step per video and epoch
    assert isinstance(r_b.score_plan, val_batch.ScoreBatchPlan) and s_b["steps"] == 0
    assert [len(b) for b in r_b.score_plan.index_lists] == [4, 1]
    want = _per_video(r_one, r_one.auc_plan.scores.cpu().numpy())
    if side == "device":
        assert s_b["outputs"] == [] and r_b.validation_step_outputs == []
        got = _per_video(r_b, r_b.auc_plan.scores.cpu().numpy())
    else:
        assert r_b.auc_plan is None and len(s_b["outputs"]) == 5
        got = [o["preds"] for o in s_b["outputs"]]
        for o, labels in zip(s_b["outputs"], r_b.valid_dataset.labels):
            assert np.array_equal(o["labels"], labels)
    for i, (g, w) in enumerate(zip(got, want)):
        e = rel_err(g, w)
        print(f"{side}: video {i} ({len(w)} clips) rel err vs per-video validation {e:.3e}")
        assert g.shape == w.shape and e < TOL
    assert _loss(t_b) == _loss(t_one) and len(_loss(t_b)) == 6  # validation does not touch training
    assert len(_vals(t_b)) == 2 and np.isfinite(_vals(t_b)).all()
    assert _vals(t_b)[-1] == metrics.frame_level_auc(got, r_b.valid_dataset.labels, 16)  # the logged AUCs: the host rule on the batched scores, bit for bit


def _runner(tmp_path, *overrides, cls=None):
    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=2, n_abnormal=2, n_test=2, channels=16)
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={d}", "data.batch_size=2", *overrides])
    return (cls or VideoAnomalyDetectionRunner)(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data).to(DEV), cfg


def test_val_batch_videos_needs_resident(tmp_path):
    runner, cfg = _runner(tmp_path, "data.val_batch_videos=4")
    assert cfg.data.val_batch_videos == 4 and cfg.data.resident is False
    with pytest.raises(ValueError, match=r"data\.val_batch_videos=4 needs data\.resident=true"):
        runner.setup("fit")
    assert not hasattr(runner, "valid_dataset")  # refused before anything is loaded


def test_default_is_per_video_and_a_subclass_keeps_its_own_validation(tmp_path):
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    runner, cfg = _runner(tmp_path, "data.resident=true")
    assert cfg.data.val_batch_videos == 1
    runner.setup("fit")
    assert runner.score_plan is None

    class Mine(VideoAnomalyDetectionRunner):
        def validation_step(self, batch, batch_idx):
            return super().validation_step(batch, batch_idx)

    mine, _ = _runner(tmp_path / "b", "data.resident=true", "data.val_batch_videos=4", cls=Mine)
    mine.setup("fit")
    assert mine.score_plan is None  # the per-video loop calls its validation_step
    stock, _ = _runner(tmp_path / "c", "data.resident=true", "data.val_batch_videos=4")
    stock.setup("fit")
    assert stock.score_plan is not None and stock.score_plan.index_lists == [sorted(range(2), key=stock.score_plan.lengths.__getitem__)]
