"""GPU tests of epoch shuffling (data.shuffle): the one-launch row gather against torch indexing, bit for bit; the shuffled resident
loader against the order rule; and training runs -- resident against the host loaders (equal, not close), one gather launch per
replayed step straight into the captured step's buffers, the same order after a resume, nothing new with the flag off."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC00000
SPECIAL = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FFFFFFF],
                   dtype=np.uint32)  # NaN payloads (quiet, negative, signalling), -0.0, 0.0, +-inf, denormals, all-ones NaN


def _pattern(n_floats: int, seed: int) -> torch.Tensor:
    """n_floats fp32 values on the device whose BITS are random, with the special patterns planted."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n_floats, dtype=np.uint64).astype(np.uint32)
    where = rng.integers(0, n_floats, min(n_floats, 3 * len(SPECIAL)))
    bits[where] = SPECIAL[np.arange(len(where)) % len(SPECIAL)]
    return torch.from_numpy(bits.view(np.int32)).to(DEV).view(torch.float32)


def _store(n: int, R: int, seed: int, offset: int = 0) -> torch.Tensor:
    """A contiguous (n, R) store; offset = 1: a view that starts one float into its allocation (4-byte aligned only)."""
    return _pattern(n * R + offset, seed)[offset:].view(n, R)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _indices(n: int, b: int, seed: int) -> torch.Tensor:
    """b indices into [0, n) with repeats; index 0 and index n - 1 are among them whenever b >= 2."""
    idx = np.random.default_rng(seed).integers(0, n, b)
    if b >= 2:
        idx[0], idx[-1] = n - 1, 0
    if b >= 3:
        idx[1] = idx[0]  # a repeated index
    return torch.from_numpy(idx.astype(np.int64)).to(DEV)


PAIRS = [(1, 0), (1, 1), (2, 5), (5, 2)]
SIZES = {(1, 0): (1, 0), (1, 1): (9, 1), (2, 5): (3, 9), (5, 2): (7, 2)}  # (n0, n1): n between 1 and 9, both ends


# R: 1, 3 and 65 take the scalar form (R * 4 is no multiple of 16); 4, 260 and 20800 the 16-byte form: one element, one partial chunk
# and several chunks per row (a chunk is 1024 elements of 16 bytes; the scalar form's, at an offset store, 1024 floats)
@pytest.mark.parametrize("R", [1, 3, 4, 65, 260, 20800])
@pytest.mark.parametrize("b0,b1", PAIRS)
def test_gather_batch_equals_torch_indexing_bit_for_bit(R, b0, b1):
    from anomaly_detection_on_video_amd import mil_ops

    n0, n1 = SIZES[(b0, b1)]
    idx0 = _indices(n0, b0, R + b0)
    idx1 = _indices(n1, b1, R + b1 + 100) if b1 else None
    b = b0 + b1
    for offset in (0, 1):  # aligned stores | stores that start one float into their allocation
        s0 = _store(n0, R, 10 * R + offset, offset)
        s1 = _store(n1, R, 10 * R + offset + 5, offset) if b1 else None
        l0, l1 = _pattern(n0, R + 1), (_pattern(n1, R + 2) if b1 else None)
        want = torch.cat([_bits(s0)[idx0]] + ([_bits(s1)[idx1]] if b1 else []))
        # dst = rows [1, 1 + b) of a larger buffer (4-byte aligned only when R is odd): the guard rows keep their bits
        big = _pattern((b + 2) * R, 7 * R + offset).view(b + 2, R)
        before = _bits(big).clone()
        d0, d1 = _pattern(b0 + 2, 3), (_pattern(b1 + 2, 4) if b1 else None)
        d0_before, d1_before = _bits(d0).clone(), (_bits(d1).clone() if b1 else None)
        out = mil_ops.gather_batch(s0, idx0, s1, idx1, big[1:1 + b], labels0=l0, labels1=l1, dst_labels0=d0[1:1 + b0],
                                   dst_labels1=d1[1:1 + b1] if b1 else None)
        assert out.data_ptr() == big[1].data_ptr()
        assert torch.equal(_bits(big)[1:1 + b], want), f"R={R} offset={offset}: gathered rows differ from store[idx]"
        assert torch.equal(_bits(big)[0], before[0]) and torch.equal(_bits(big)[-1], before[-1]), "a guard row changed"
        assert torch.equal(_bits(d0)[1:1 + b0], _bits(l0)[idx0]) and torch.equal(_bits(d0)[[0, -1]], d0_before[[0, -1]])
        if b1:
            assert torch.equal(_bits(d1)[1:1 + b1], _bits(l1)[idx1]) and torch.equal(_bits(d1)[[0, -1]], d1_before[[0, -1]])
        # without labels, into a buffer of its own
        dst = torch.empty(b, R, device=DEV)
        mil_ops.gather_batch(s0, idx0, s1, idx1, dst)
        assert torch.equal(_bits(dst), want)


@pytest.mark.parametrize("R", [3, 260, 20800])
def test_gather_rows_with_and_without_out(R):
    from anomaly_detection_on_video_amd import mil_ops

    store = _store(9, R, R).view(9, 1, R)  # rows of more than one dimension
    idx = _indices(9, 4, R)
    want = _bits(store)[idx]
    got = mil_ops.gather_rows(store, idx)
    assert got.shape == (4, 1, R) and got.dtype == torch.float32 and torch.equal(_bits(got), want)
    out = torch.empty(4, 1, R, device=DEV)
    assert mil_ops.gather_rows(store, idx, out=out).data_ptr() == out.data_ptr() and torch.equal(_bits(out), want)


@pytest.mark.parametrize("R", [65, 260])  # the scalar and the 16-byte form
def test_out_of_range_indices_give_nan_rows_and_touch_nothing_else(R):
    from anomaly_detection_on_video_amd import mil_ops

    n0, n1 = 4, 3
    s0, s1, l0, l1 = _store(n0, R, 1), _store(n1, R, 2), _pattern(n0, 3), _pattern(n1, 4)
    idx0 = torch.tensor([1, n0, 3], device=DEV)    # an index of n
    idx1 = torch.tensor([-1, 2], device=DEV)       # an index of -1
    big = _pattern(7 * R, 5).view(7, R)
    before = _bits(big).clone()
    d0, d1 = torch.zeros(3, device=DEV), torch.zeros(2, device=DEV)
    mil_ops.gather_batch(s0, idx0, s1, idx1, big[1:6], labels0=l0, labels1=l1, dst_labels0=d0, dst_labels1=d1)
    torch.cuda.synchronize()  # a defined result, not a fault
    got = _bits(big)
    nan_row = torch.full((R,), NAN_BITS, dtype=torch.int32, device=DEV)
    assert torch.equal(got[2], nan_row) and torch.equal(got[4], nan_row)
    assert torch.equal(got[1], _bits(s0)[1]) and torch.equal(got[3], _bits(s0)[3]) and torch.equal(got[5], _bits(s1)[2])
    assert torch.equal(got[0], before[0]) and torch.equal(got[6], before[6])
    assert _bits(d0).tolist() == [_bits(l0)[1].item(), NAN_BITS, _bits(l0)[3].item()]
    assert _bits(d1).tolist() == [NAN_BITS, _bits(l1)[2].item()]
    rows = mil_ops.gather_rows(s0, torch.tensor([-1, 0, n0], device=DEV))
    assert torch.isnan(rows[0]).all() and torch.isnan(rows[2]).all() and torch.equal(_bits(rows)[1], _bits(s0)[0])


def test_wrapper_refusals():
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd._lib import HipExtensionError

    store, idx, dst = torch.zeros(4, 8, device=DEV), torch.tensor([0, 1], device=DEV), torch.empty(2, 8, device=DEV)
    mil_ops.gather_batch(store, idx, None, None, dst)
    with pytest.raises(HipExtensionError, match="no CPU fallback"):  # CPU tensors
        mil_ops.gather_rows(store.cpu(), idx.cpu())
    with pytest.raises(HipExtensionError, match="no CPU fallback"):
        mil_ops.gather_batch(store, idx, None, None, dst.cpu())
    with pytest.raises(HipExtensionError):  # a non-fp32 store
        mil_ops.gather_rows(store.double(), idx)
    with pytest.raises(HipExtensionError, match="fp32"):
        mil_ops.gather_rows(store.to(torch.int32), idx)
    with pytest.raises(HipExtensionError, match="contiguous"):  # a non-contiguous store
        mil_ops.gather_rows(torch.zeros(4, 16, device=DEV)[:, ::2], idx)
    with pytest.raises(HipExtensionError, match="int64"):  # an index that is not int64 ...
        mil_ops.gather_rows(store, idx.to(torch.int32))
    with pytest.raises(HipExtensionError):  # ... or not on the store's device
        mil_ops.gather_rows(store, idx.cpu())
    with pytest.raises(HipExtensionError, match="int64"):
        mil_ops.gather_batch(store, idx, store, idx.to(torch.int32), torch.empty(4, 8, device=DEV))
    for bad in (torch.empty(3, 8, device=DEV), torch.empty(2, 4, device=DEV), torch.empty(16, device=DEV)):  # a dst of another shape
        with pytest.raises(HipExtensionError, match="dst must be"):
            mil_ops.gather_batch(store, idx, None, None, bad)
    with pytest.raises(HipExtensionError, match="dst must be"):
        mil_ops.gather_batch(store, idx, store, idx, dst)  # two stores need b0 + b1 rows
    with pytest.raises(HipExtensionError, match="rows differ"):
        mil_ops.gather_batch(store, idx, torch.zeros(4, 4, device=DEV), idx, torch.empty(4, 8, device=DEV))
    with pytest.raises(HipExtensionError, match="labels"):
        mil_ops.gather_batch(store, idx, None, None, dst, labels0=torch.zeros(4, device=DEV))


# ------------------------------------------------------------------------------ the loader
def test_shuffled_resident_batches_serve_the_order(tmp_path):
    from anomaly_detection_on_video_amd.dataset import (ResidentBatches, ShuffledResidentBatches, StoreRows, build_feature_dataset, epoch_order,
                                                        write_synthetic_feature_zips)

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=7, n_abnormal=3, n_test=2, channels=16)
    ds = build_feature_dataset("train", local_path=d, filename="train.zip", resident=DEV)["normal"]
    B, seed, stream, epoch = 2, 9, 0, 3
    loader = ShuffledResidentBatches(ds, B, seed, stream, epoch)
    assert isinstance(loader, ResidentBatches) and len(loader) == len(ResidentBatches(ds, B)) == 3
    feats = _bits(ds.features)
    for restart in (0, 1):  # a second iter() serves restart 1
        order = epoch_order(7, seed, stream, epoch, restart)
        assert order.tolist() != list(range(7))
        steps = list(iter(loader))
        table = loader.table
        assert table.is_cuda and table.dtype == torch.int64 and table.tolist() == order[:3 * B].tolist()
        assert len(steps) == 3 and all(isinstance(s, StoreRows) for s in steps)
        for i, step in enumerate(steps):
            rows = order[i * B:(i + 1) * B].tolist()
            assert step.rows.data_ptr() == table[i * B].data_ptr() and step.rows.tolist() == rows  # a view of the device table
            item = step.materialize()
            assert item["feature"].shape == (B,) + tuple(ds.features.shape[1:])
            assert torch.equal(_bits(item["feature"]), feats[rows]) and torch.equal(item["anomaly"], ds.anomaly[rows])
    for bad in (0, 8):  # ResidentBatches' refusals
        with pytest.raises(ValueError):
            ShuffledResidentBatches(ds, bad, seed, stream, epoch)
    with pytest.raises(ValueError, match="seed"):
        ShuffledResidentBatches(ds, B, -1, stream, epoch)


# ------------------------------------------------------------------------------ training
SEED = 5  # epoch_order(4, 5, 0, 0) = [3 1 0 2], epoch_order(6, 5, 1, 0) = [2 5 1 4 3 0]: not the file order


def _train(tmp_path, data_dir, tag, extra=()):
    """run.main on the synthetic corpus (the pattern of tests/test_hip_resident.py::_train) with every gather launch recorded:
    seen["gathers"] = one record per mil_ops.gather_batch call, seen["steps"] = per training step, whether it was fed as a replay and
    how many gather calls it made."""
    import run
    from anomaly_detection_on_video_amd import mil_ops
    from anomaly_detection_on_video_amd.runner import Trainer, VideoAnomalyDetectionRunner

    seen = {"loaders": [], "gathers": [], "steps": [], "runner": None, "trainer": None}
    real_loader, real_feed, real_gather = VideoAnomalyDetectionRunner.train_dataloader, Trainer._feed_graph_inputs, mil_ops.gather_batch

    def train_dataloader(self):
        seen["runner"] = self
        seen["loaders"].append(real_loader(self))
        return seen["loaders"][-1]

    def gather_batch(store0, idx0, store1, idx1, dst, labels0=None, labels1=None, dst_labels0=None, dst_labels1=None):
        out = real_gather(store0, idx0, store1, idx1, dst, labels0=labels0, labels1=labels1, dst_labels0=dst_labels0, dst_labels1=dst_labels1)
        rec = {"store0": store0.data_ptr(), "idx0": idx0.tolist(), "store1": None if store1 is None else store1.data_ptr(),
               "idx1": None if idx1 is None else idx1.tolist(), "dst": dst.data_ptr(), "epoch": seen["runner"].current_epoch}
        if store1 is not None:  # the replay feed: what the buffers hold right after the call
            rec["rows_ok"] = torch.equal(_bits(dst), torch.cat((_bits(store0)[idx0], _bits(store1)[idx1])))
            rec["labels_ok"] = torch.equal(dst_labels0, labels0[idx0]) and torch.equal(dst_labels1, labels1[idx1])
            rec["label_dsts"] = (dst_labels0.data_ptr(), dst_labels1.data_ptr())
        seen["gathers"].append(rec)
        return out

    def feed(graphed, batch):
        before = len(seen["gathers"])
        ok = real_feed(graphed, batch)
        seen["steps"].append({"fed": ok, "gathers_in_feed": len(seen["gathers"]) - before, "first_gather": before,
                              "inputs": None if graphed.inputs() is None else tuple(t.data_ptr() for t in graphed.inputs())})
        return ok

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(VideoAnomalyDetectionRunner, "train_dataloader", train_dataloader)
        mp.setattr(Trainer, "_feed_graph_inputs", staticmethod(feed))
        mp.setattr(mil_ops, "gather_batch", gather_batch)
        torch.manual_seed(0)
        trainer = run.main(["data=synthetic", f"data.local_path={data_dir}", "data.batch_size=2", "trainer.cls.max_epochs=2",
                            f"trainer.callbacks.model_checkpoint.dirpath={tmp_path / ('ckpt_' + tag)}",
                            f"trainer.logger.jsonl.path={tmp_path / (tag + '.jsonl')}", *extra])
    seen["trainer"] = trainer
    return trainer, seen


def _fed_rows(seen, epoch=None):
    """{"normal": [...], "abnormal": [...]}: the store rows the run fed, step after step, from the recorded gather calls."""
    train = seen["runner"].train_dataset
    name = {train[cls].features.data_ptr(): cls for cls in ("normal", "abnormal")}
    out = {"normal": [], "abnormal": []}
    for g in seen["gathers"]:
        if epoch is not None and g["epoch"] != epoch:
            continue
        out[name[g["store0"]]] += g["idx0"]
        if g["store1"] is not None:
            out[name[g["store1"]]] += g["idx1"]
    return out


def _expected_rows(seed, epoch):
    """4 normal and 6 abnormal videos at batch_size 2: three steps per epoch, the normal loader (two steps) restarts for the third."""
    from anomaly_detection_on_video_amd.dataset import epoch_order

    normal = epoch_order(4, seed, 0, epoch, 0)[:4].tolist() + epoch_order(4, seed, 0, epoch, 1)[:2].tolist()
    return {"normal": normal, "abnormal": epoch_order(6, seed, 1, epoch, 0)[:6].tolist()}


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from anomaly_detection_on_video_amd.dataset import write_synthetic_feature_zips

    return write_synthetic_feature_zips(str(tmp_path_factory.mktemp("shuffle") / "feat"), n_normal=4, n_abnormal=6, n_test=4, seed=2)


@pytest.fixture(scope="module")
def runs(corpus, tmp_path_factory):
    """The host-loader run and the resident run, both shuffled with SEED, 2 epochs, a checkpoint after each (shared, read-only)."""
    tmp = tmp_path_factory.mktemp("shuffle_runs")
    common = ("data.shuffle=true", f"data.seed={SEED}", "trainer.callbacks.model_checkpoint.every_n_epochs=1")
    host = _train(tmp, corpus, "host", extra=common)
    resident = _train(tmp, corpus, "resident", extra=common + ("data.resident=true",))
    return {"host": host, "resident": resident, "tmp": tmp}


def test_shuffled_resident_training_equals_the_host_loader_run(runs):
    from torch.utils.data import DataLoader

    from anomaly_detection_on_video_amd.dataset import ShuffledResidentBatches, ShuffledSampler

    (t_host, s_host), (t_res, s_res) = runs["host"], runs["resident"]
    assert all(type(ld) is DataLoader and isinstance(ld.sampler, ShuffledSampler) for pair in s_host["loaders"] for ld in pair)
    assert len(s_res["loaders"]) == 2 and all(type(ld) is ShuffledResidentBatches for pair in s_res["loaders"] for ld in pair)
    assert [(ld.seed, ld.stream, ld.epoch) for pair in s_res["loaders"] for ld in pair] == [(SEED, 0, 0), (SEED, 1, 0), (SEED, 0, 1), (SEED, 1, 1)]
    assert not s_host["gathers"]  # the host path launches no gather
    loss = lambda t: [h["train_loss"] for h in t.history if "train_loss" in h]
    vals = lambda t: [(h["valid/rec_auc"], h["valid/pr_auc"]) for h in t.history if "valid/rec_auc" in h]
    print("train_loss host    ", loss(t_host), "\ntrain_loss resident", loss(t_res), "\nvalid host    ", vals(t_host), "\nvalid resident", vals(t_res))
    assert len(loss(t_host)) == 6 and len(vals(t_host)) == 2 and all(np.isfinite(loss(t_host)))
    assert loss(t_res) == loss(t_host)
    assert vals(t_res) == vals(t_host)
    sd_host, sd_res = s_host["runner"].model.state_dict(), s_res["runner"].model.state_dict()
    assert list(sd_host) == list(sd_res)
    for k in sd_host:
        assert torch.equal(sd_host[k], sd_res[k]), k


def test_every_replayed_step_is_one_gather_into_the_graphs_buffers(runs):
    t_res, s_res = runs["resident"]
    g = t_res.graphed_step
    assert g is not None and g.captures == 1 and g.replays == 3  # steps 1-3 eager, step 4 captured and replayed, steps 5 and 6 fed
    steps = s_res["steps"]
    assert len(steps) == 6 and [s["fed"] for s in steps] == [False] * 4 + [True] * 2
    static = tuple(t.data_ptr() for t in g.inputs())
    for s in steps[4:]:
        assert s["gathers_in_feed"] == 1 and s["inputs"] == static
        rec = s_res["gathers"][s["first_gather"]]
        assert rec["store1"] is not None and rec["dst"] == static[0] == g.inputs()[0].data_ptr()
        assert rec["label_dsts"] == (static[2], static[1])  # normal labels, abnormal labels
        assert rec["rows_ok"] and rec["labels_ok"]
    # the other steps got ordinary tensors: one gather per class into the loaders' own buffers, none into the graph's
    two_store = [r for r in s_res["gathers"] if r["store1"] is not None]
    one_store = [r for r in s_res["gathers"] if r["store1"] is None]
    assert len(two_store) == 2 and len(one_store) == 8 and all(r["dst"] != static[0] for r in one_store)


def test_the_order_is_shuffled_and_is_the_rule(runs):
    _, s_res = runs["resident"]
    for epoch in (0, 1):
        fed, want = _fed_rows(s_res, epoch), _expected_rows(SEED, epoch)
        assert fed == want, f"epoch {epoch}: fed {fed}, the rule gives {want}"
        assert fed["normal"] != [0, 1, 2, 3, 0, 1] and fed["abnormal"] != list(range(6))  # what the unshuffled loaders feed
    assert _fed_rows(s_res, 0) != _fed_rows(s_res, 1)


def test_same_seed_same_sequence_other_seed_another(runs, corpus):
    _, s_res = runs["resident"]
    one_epoch = ("data.shuffle=true", "data.resident=true", "trainer.cls.max_epochs=1")
    _, again = _train(runs["tmp"], corpus, "again", extra=one_epoch + (f"data.seed={SEED}",))
    _, other = _train(runs["tmp"], corpus, "other", extra=one_epoch + (f"data.seed={SEED + 1}",))
    assert _fed_rows(again) == _fed_rows(s_res, 0)
    assert _fed_rows(other) == _expected_rows(SEED + 1, 0) and _fed_rows(other) != _fed_rows(s_res, 0)


def test_resume_continues_with_the_uninterrupted_runs_order(runs, corpus):
    _, s_res = runs["resident"]
    found = glob.glob(str(runs["tmp"] / "ckpt_resident" / "epoch=0-*.ckpt"))
    assert len(found) == 1, found
    ckpt = str(runs["tmp"] / "epoch0.ckpt")
    shutil.copy(found[0], ckpt)
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert saved["epoch"] == 0 and saved["hyper_parameters"]["data"]["shuffle"] is True and saved["hyper_parameters"]["data"]["seed"] == SEED
    t, s = _train(runs["tmp"], corpus, "resumed", extra=("data.shuffle=true", f"data.seed={SEED}", "data.resident=true", f"ckpt_path={ckpt}"))
    assert [ld.epoch for pair in s["loaders"] for ld in pair] == [1, 1]  # epoch 1 only
    assert _fed_rows(s) == _fed_rows(s_res, 1) == _expected_rows(SEED, 1)  # restarts included: the normal class restarts in its third step
    assert t.global_step == 6


def test_flag_off_keeps_resident_batches_and_launches_no_gather(corpus, tmp_path):
    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.dataset import ResidentBatches
    from conftest import REPO

    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", "~data.shuffle", "~data.seed"])
    assert "shuffle" not in cfg.data  # (a config from before this key: the runner reads it with a default)
    _, s = _train(tmp_path, corpus, "off", extra=("data.resident=true", "~data.shuffle", "trainer.cls.max_epochs=1"))
    assert "shuffle" not in s["runner"].hparams.data
    assert len(s["loaders"]) == 1 and all(type(ld) is ResidentBatches for ld in s["loaders"][0])
    assert not s["gathers"] and [st["gathers_in_feed"] for st in s["steps"]] == [0, 0, 0]
