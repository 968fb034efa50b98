"""CPU-only checks of the device-resident feature datasets: the numpy restatement the magnitude kernel is held to
(tests/_pairwise_ref.py) against numpy itself, the library's leaf table, the batch schedule of `ResidentBatches` against real
DataLoaders, and the refusals (none of which touches a GPU)."""
import io
import os
import zipfile

import numpy as np
import pytest
import torch

import _pairwise_ref as pw
from conftest import GOLDEN

C_LIST = (1, 5, 7, 8, 9, 48, 64, 100, 127, 128, 129, 1000, 1024, 2047, 2048, 2049, 4096)
C_LIST_LONG = (4097, 6000, 8192)
NUMPY_DIFFERS = ("numpy on this machine sums a float32 row in another order than tests/_pairwise_ref.py restates: the restatement "
                 "(and with it the expectation the kernel is held to) does not describe this numpy; the kernel is not at fault")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    return _lib.load()


def _rows(C, rows, seed):
    return (np.random.default_rng(seed).standard_normal((1, rows, C)) * 3).astype(np.float32)


# ------------------------------------------------------------------------------ the restatement is numpy
@pytest.mark.parametrize("C", C_LIST + C_LIST_LONG)
def test_restatement_is_numpy_bit_for_bit(C):
    x = _rows(C, 6 if C in C_LIST_LONG else 12, C)
    assert np.array_equal(pw.bits(pw.norm_rows(x)), pw.bits(np.linalg.norm(x, axis=2))), NUMPY_DIFFERS


def test_restatement_on_a_train_item_special_rows_and_the_reference_golden():
    from anomaly_detection_on_video_amd.weights import synth_tensor

    x = np.abs(np.random.default_rng(0).standard_normal((10, 32, 2048))).astype(np.float32)
    assert np.array_equal(pw.bits(pw.norm_rows(x)), pw.bits(np.linalg.norm(x, axis=2))), NUMPY_DIFFERS
    s = _rows(48, 4, 1)
    s[0, 0] = 0.0
    s[0, 1, 3] = np.inf
    s[0, 2, 40] = np.nan
    got = pw.norm_rows(s)
    assert got[0, 0] == 0.0 and np.isposinf(got[0, 1]) and np.isnan(got[0, 2]) and np.isfinite(got[0, 3])
    with np.errstate(all="ignore"):
        assert np.array_equal(pw.bits(got), pw.bits(np.linalg.norm(s, axis=2))), NUMPY_DIFFERS
    # the reference's own FeatureDataset.add_magnitude output
    f = synth_tensor("addmag", (10, 32, 48), scale=2.0).numpy()
    g = np.load(os.path.join(GOLDEN, "host.npz"))["addmag"]
    assert np.array_equal(pw.bits(pw.add_magnitude(f)), pw.bits(g)), NUMPY_DIFFERS
    assert np.array_equal(pw.bits(pw.add_magnitude(f, transpose=True)), pw.bits(g.transpose(1, 0, 2)))


# ------------------------------------------------------------------------------ the library's leaf table
@pytest.mark.parametrize("C", C_LIST + C_LIST_LONG)
def test_leaf_table_tiles_the_row_and_sums_like_the_restatement(lib, C):
    from anomaly_detection_on_video_amd import mil_ops

    table = mil_ops.add_magnitude_np_leaves(C)
    assert table == pw.leaves(C)
    assert 1 <= len(table) <= 128 and table[0][0] == 0 and table[-1][0] + table[-1][1] == C
    assert all(table[i][0] + table[i][1] == table[i + 1][0] for i in range(len(table) - 1))
    assert all(1 <= n <= 128 for _, n, _ in table) and all(s % 8 == 0 for s, _, _ in table)
    assert sum(a for _, _, a in table) == len(table) - 1  # a binary tree over the leaves
    x = _rows(C, 5, 100 + C)[0]
    s = x * x
    assert np.array_equal(pw.bits(pw.sum_by_table(s, table)), pw.bits(pw.pairwise_sum(s)))


# ------------------------------------------------------------------------------ the batch schedule
class _Index(torch.utils.data.Dataset):
    def __init__(self, n, anomaly):
        self.n, self.anomaly = n, anomaly

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return {"feature": np.full((2, 3), i, dtype=np.float32), "anomaly": np.array(self.anomaly, dtype=np.float32)}


@pytest.mark.parametrize("n_normal,n_abnormal,batch", [(8, 8, 2), (7, 3, 2), (3, 7, 2), (5, 5, 5), (4, 9, 4)])
def test_resident_batches_follow_the_dataloader_schedule(n_normal, n_abnormal, batch):
    from torch.utils.data import DataLoader

    from anomaly_detection_on_video_amd.dataset import ResidentBatches, ResidentFeatureDataset
    from anomaly_detection_on_video_amd.runner import Trainer

    def resident(n, cls, anomaly):
        feats = torch.arange(n, dtype=torch.float32).view(n, 1, 1).expand(n, 2, 3).contiguous()
        return ResidentFeatureDataset([f"{cls}{i}" for i in range(n)], cls, features=feats, anomaly=torch.full((n,), anomaly))

    rn, ra = resident(n_normal, "normal", 0.0), resident(n_abnormal, "abnormal", 1.0)
    mine = (ResidentBatches(rn, batch), ResidentBatches(ra, batch))
    theirs = tuple(DataLoader(_Index(n, a), batch_size=batch, shuffle=False, drop_last=True) for n, a in ((n_normal, 0.0), (n_abnormal, 1.0)))
    assert [len(m) for m in mine] == [len(t) for t in theirs] == [n_normal // batch, n_abnormal // batch]
    for _epoch in range(2):
        got, want = list(Trainer._max_size_cycle(*mine)), list(Trainer._max_size_cycle(*theirs))
        assert len(got) == len(want) == max(n_normal, n_abnormal) // batch
        for g, w in zip(got, want):
            for side, ds in zip((0, 1), (rn, ra)):
                assert torch.equal(g[side]["feature"], w[side]["feature"]) and torch.equal(g[side]["anomaly"], w[side]["anomaly"])
                assert g[side]["feature"].dtype == w[side]["feature"].dtype and g[side]["anomaly"].shape == w[side]["anomaly"].shape
                # views of the store: a slice starting at the batch's first index
                first = int(g[side]["feature"][0, 0, 0])
                assert g[side]["feature"].data_ptr() == ds.features[first].data_ptr()
                assert g[side]["anomaly"].data_ptr() == ds.anomaly[first:].data_ptr()


# ------------------------------------------------------------------------------ refusals
def _zip(path, items):
    with zipfile.ZipFile(path, "w") as z:
        for name, arr in items:
            buf = io.BytesIO()
            np.save(buf, arr)
            z.writestr(name, buf.getvalue())


def test_ragged_train_items_are_refused_by_name(tmp_path):
    from anomaly_detection_on_video_amd.dataset import build_feature_dataset

    _zip(tmp_path / "train.zip", [("train/Normal_Videos000_x264_i3d.npy", np.zeros((10, 32, 16), np.float32)),
                                  ("train/Abuse001_x264_i3d.npy", np.zeros((10, 31, 16), np.float32))])
    with pytest.raises(ValueError, match=r"Abuse001_x264_i3d\.npy has shape \(10, 31, 16\).*one shape"):
        build_feature_dataset("train", local_path=str(tmp_path), filename="train.zip", resident="cuda:0")
    _zip(tmp_path / "train.zip", [("train/Normal_Videos000_x264_i3d.npy", np.zeros((10, 32, 16), np.float64))])
    with pytest.raises(ValueError, match=r"Normal_Videos000_x264_i3d\.npy.*float32"):
        build_feature_dataset("train", local_path=str(tmp_path), filename="train.zip", resident="cuda:0")


def test_a_class_smaller_than_the_batch_is_refused_by_name():
    from anomaly_detection_on_video_amd.dataset import ResidentBatches, ResidentFeatureDataset

    ds = ResidentFeatureDataset(["a", "b", "c"], "abnormal", features=torch.zeros(3, 2, 2, 5), anomaly=torch.ones(3))
    assert len(ResidentBatches(ds, 3)) == 1
    with pytest.raises(ValueError, match="abnormal class has 3 videos, fewer than batch_size 4"):
        ResidentBatches(ds, 4)


def test_a_corpus_over_the_byte_budget_is_refused_before_any_allocation(tmp_path):
    from anomaly_detection_on_video_amd.dataset import build_feature_dataset, write_synthetic_feature_zips

    d = write_synthetic_feature_zips(str(tmp_path), n_normal=3, n_abnormal=2, n_test=2, channels=32)
    need = 5 * 10 * 32 * 33 * 4 + 5 * 4  # features with the magnitude channel + the anomaly vector
    with pytest.raises(ValueError, match=rf"needs {need} bytes.*resident_max_bytes = {need - 1}\b"):
        build_feature_dataset("train", local_path=d, filename="train.zip", resident="cuda:0", resident_max_bytes=need - 1)
    with pytest.raises(ValueError, match=r"needs \d+ bytes.*resident_max_bytes = 1000\b"):
        build_feature_dataset("test", local_path=d, filename="test.zip", resident="cuda:0", resident_max_bytes=1000)
    # the default (resident=None) is today's host dataset
    from anomaly_detection_on_video_amd.dataset import FeatureDataset

    assert isinstance(build_feature_dataset("test", local_path=d, filename="test.zip"), FeatureDataset)


def test_capi_refuses_wide_rows_and_null_pointers_without_a_launch(lib):
    import ctypes as C

    p = C.c_void_p(4096)  # stands for a device pointer; every call below fails validation, nothing is launched
    assert lib.advhip_add_magnitude_np_f32(p, p, 2, 3, 8193, 0, None) == -1
    msg = lib.advhip_last_error()
    assert b"C=8193" in msg and b"8192" in msg
    assert lib.advhip_add_magnitude_np_f32(None, p, 2, 3, 64, 0, None) == -1
    assert b"null pointer" in lib.advhip_last_error()
    assert lib.advhip_add_magnitude_np_f32(p, None, 2, 3, 64, 1, None) == -1
    assert b"null pointer" in lib.advhip_last_error()
    assert lib.advhip_add_magnitude_np_f32(p, p, 0, 3, 64, 0, None) == -1
    assert lib.advhip_add_magnitude_np_f32(p, p, 2, 3, 64, 2, None) == -1
    n = C.c_int32()
    buf = (C.c_int32 * 384)()
    assert lib.advhip_add_magnitude_np_leaves(8193, buf, C.byref(n)) == -1
    assert lib.advhip_add_magnitude_np_leaves(64, None, C.byref(n)) == -1


def test_the_wrapper_refuses_cpu_tensors():
    from anomaly_detection_on_video_amd import _lib, mil_ops

    with pytest.raises(_lib.HipExtensionError):
        mil_ops.add_magnitude_np(torch.zeros(2, 3, 8))
