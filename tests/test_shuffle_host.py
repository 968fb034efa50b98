"""CPU-only checks of epoch shuffling (data.shuffle): the order rule pinned with literals, the host loaders' sampler, the config
defaults (shuffle off: the loaders as before), and the gather entry point's declaration against its ctypes signature."""
import os

import numpy as np
import pytest

import ctypes as C
import re

from conftest import REPO

SYMBOL = "advhip_gather_batch_f32"
_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "int": C.c_int}


def _declared(name):
    """(restype, argtypes) of `name` as include/advhip.h declares it."""
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/advhip.h"
    args = [C.c_void_p if "*" in a else _CTYPE[a.replace("const", "").split()[0]] for a in (a.strip() for a in m.group(2).split(","))]
    return _CTYPE[m.group(1)], args


def test_epoch_order_literals():
    from anomaly_detection_on_video_amd.dataset import epoch_order

    a, b = epoch_order(10, 7, 1, 3, 0), epoch_order(10, 7, 1, 3, 1)
    assert a.dtype == np.int64 and a.tolist() == [9, 5, 3, 7, 4, 1, 8, 6, 2, 0]
    assert b.dtype == np.int64 and b.tolist() == [4, 0, 7, 9, 8, 1, 3, 5, 2, 6]
    assert epoch_order(10, 7, 1, 3).tolist() == a.tolist()  # restart defaults to 0
    assert a.tolist() == np.random.RandomState([7, 1, 3, 0]).permutation(10).tolist()  # the stated rule


@pytest.mark.parametrize("n", [1, 2, 7, 1000])
def test_epoch_order_is_a_permutation_and_a_function_of_its_arguments(n):
    from anomaly_detection_on_video_amd.dataset import epoch_order

    base = epoch_order(n, 11, 0, 2, 0)
    assert base.shape == (n,) and sorted(base.tolist()) == list(range(n))
    assert epoch_order(n, 11, 0, 2, 0).tolist() == base.tolist()  # identical on a second call
    if n == 1000:  # (a permutation of 1 or 2 items cannot differ four ways)
        others = [epoch_order(n, 11, 1, 2, 0), epoch_order(n, 11, 0, 3, 0), epoch_order(n, 11, 0, 2, 1), epoch_order(n, 12, 0, 2, 0)]
        for o in others:
            assert sorted(o.tolist()) == list(range(n)) and o.tolist() != base.tolist()
        assert base.tolist() != list(range(n))


def test_epoch_order_differs_between_streams_epochs_and_restarts_at_small_n():
    from anomaly_detection_on_video_amd.dataset import epoch_order

    base = epoch_order(7, 5, 0, 0, 0).tolist()
    assert epoch_order(7, 5, 1, 0, 0).tolist() != base and epoch_order(7, 5, 0, 1, 0).tolist() != base and epoch_order(7, 5, 0, 0, 1).tolist() != base


@pytest.mark.parametrize("bad", [-1, 2 ** 32])
def test_epoch_order_refuses_values_outside_uint32(bad):
    from anomaly_detection_on_video_amd.dataset import ShuffledSampler, epoch_order

    with pytest.raises(ValueError, match="seed"):
        epoch_order(4, bad, 0, 0)
    with pytest.raises(ValueError, match="stream"):
        epoch_order(4, 0, bad, 0)
    with pytest.raises(ValueError, match="epoch"):
        epoch_order(4, 0, 0, bad)
    with pytest.raises(ValueError, match="restart"):
        epoch_order(4, 0, 0, 0, bad)
    with pytest.raises(ValueError, match="seed"):
        ShuffledSampler(4, bad, 0, 0)


def test_sampler_serves_restart_0_then_restart_1():
    from anomaly_detection_on_video_amd.dataset import ShuffledSampler, epoch_order

    s = ShuffledSampler(9, 3, 1, 4)
    assert len(s) == 9
    assert list(iter(s)) == epoch_order(9, 3, 1, 4, 0).tolist()
    assert list(iter(s)) == epoch_order(9, 3, 1, 4, 1).tolist()
    assert list(iter(s)) == epoch_order(9, 3, 1, 4, 2).tolist()


@pytest.fixture(scope="module")
def small_corpus(tmp_path_factory):
    from anomaly_detection_on_video_amd.dataset import build_feature_dataset, write_synthetic_feature_zips

    d = write_synthetic_feature_zips(str(tmp_path_factory.mktemp("shuffle_feat")), n_normal=7, n_abnormal=5, n_test=2, channels=16)
    return d, build_feature_dataset("train", local_path=d, filename="train.zip", dynamic_load=False)


@pytest.mark.parametrize("num_workers", [0, 2])
def test_dataloader_delivers_the_order_and_drops_its_tail(small_corpus, num_workers):
    from torch.utils.data import DataLoader

    from anomaly_detection_on_video_amd.dataset import ShuffledSampler, epoch_order

    _, train = small_corpus
    ds, bs = train["normal"], 2
    assert len(ds) == 7
    loader = DataLoader(ds, batch_size=bs, sampler=ShuffledSampler(len(ds), 6, 0, 1), drop_last=True, num_workers=num_workers)
    assert len(loader) == 3
    for restart in (0, 1):  # a second iter() of the same loader is the next restart
        order = epoch_order(len(ds), 6, 0, 1, restart)
        kept = order[:len(loader) * bs]
        assert order.tolist() != list(range(len(ds)))
        got = [b["feature"].numpy() for b in loader]
        assert len(got) == 3
        for i, feat in enumerate(got):
            want = np.stack([ds[int(j)]["feature"] for j in kept[i * bs:(i + 1) * bs]])
            assert feat.shape == want.shape and feat.dtype == want.dtype and feat.tobytes() == want.tobytes()


def test_config_defaults_and_plain_loaders_when_off(small_corpus):
    import torch
    from torch.utils.data import DataLoader, SequentialSampler

    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.dataset import ShuffledSampler
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    d, _ = small_corpus
    for data in ("default", "synthetic", "ucf"):
        cfg = compose(os.path.join(REPO, "configs"), "default", [f"data={data}"])
        assert cfg.data.shuffle is False and cfg.data.seed == 0
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={d}", "data.batch_size=2"])
    runner = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data)
    runner.setup("fit")
    loaders = runner.train_dataloader()
    assert len(loaders) == 2 and all(type(ld) is DataLoader and isinstance(ld.sampler, SequentialSampler) for ld in loaders)
    # on: the same loaders with the sampler, for (seed, class, current_epoch)
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", f"data.local_path={d}", "data.batch_size=2", "data.shuffle=true",
                                                             "data.seed=3"])
    assert cfg.data.shuffle is True and cfg.data.seed == 3
    runner = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data)
    runner.setup("fit")
    runner.current_epoch = 4
    loaders = runner.train_dataloader()
    assert all(type(ld) is DataLoader and ld.drop_last for ld in loaders)
    for stream, ld in enumerate(loaders):
        s = ld.sampler
        assert isinstance(s, ShuffledSampler) and (s.n, s.seed, s.stream, s.epoch, s.restart) == (len(ld.dataset), 3, stream, 4, 0)


@pytest.mark.parametrize("seed", ["-1", "4294967296"])
def test_setup_refuses_a_seed_outside_uint32_before_loading(seed):
    import torch

    from anomaly_detection_on_video_amd.config import compose
    from anomaly_detection_on_video_amd.runner import VideoAnomalyDetectionRunner

    # (the path does not exist: the refusal comes before anything is opened)
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", "data.local_path=/nonexistent/shuffle", f"data.seed={seed}"])
    runner = VideoAnomalyDetectionRunner(torch.nn.Linear(2, 2), cfg.runner.optimizer, cfg.data)
    with pytest.raises(ValueError, match="data.seed"):
        runner.setup("fit")


def test_gather_entry_point_is_declared_bound_and_exported():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    res, args = _declared(SYMBOL)
    assert SYMBOL in _lib.SIGNATURES, f"{SYMBOL} has no ctypes signature"
    assert _lib.SIGNATURES[SYMBOL] == (res, args), f"{SYMBOL}: include/advhip.h and _lib.SIGNATURES disagree"
    assert hasattr(lib, SYMBOL), f"{SYMBOL} is not exported"
    # null pointers and non-positive sizes are refused before anything is launched (no GPU needed)
    fn = lib.advhip_gather_batch_f32
    assert fn(None, None, None, 4, 2, None, None, None, 0, 0, None, None, None, 8, None) != 0 and b"gather_batch" in lib.advhip_last_error()
    buf = (C.c_float * 64)()
    idx = (C.c_int64 * 4)()
    p, q = C.addressof(buf), C.addressof(idx)
    assert fn(p, q, None, 0, 2, None, None, None, 0, 0, p, None, None, 8, None) != 0  # n0 = 0
    assert fn(p, q, None, 4, 0, None, None, None, 0, 0, p, None, None, 8, None) != 0  # b0 = 0
    assert fn(p, q, None, 4, 2, None, None, None, 0, 0, p, None, None, 0, None) != 0  # R = 0
    assert fn(p, q, None, 4, 2, None, None, None, 0, -1, p, None, None, 8, None) != 0  # b1 < 0
    assert fn(p, q, None, 4, 2, None, q, None, 4, 2, p, None, None, 8, None) != 0  # a second index without its store
    assert fn(p, q, p, 4, 2, None, None, None, 0, 0, p, None, None, 8, None) != 0  # labels without a destination
    assert fn(p, q, None, 4, 65536, None, None, None, 0, 0, p, None, None, 8, None) != 0 and b"launch grid" in lib.advhip_last_error()
