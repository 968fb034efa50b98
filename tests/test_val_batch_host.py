"""CPU-only checks of batched validation: the bucket planner's properties, the new C entry points' declarations against their
ctypes signatures, and the config default (data.val_batch_videos = 1: validation as before)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("advhip_glance_attention_fwd_lens_f32", "advhip_dwconv_t_fwd_lens_f32", "advhip_amp_combine_fwd_lens_f32", "advhip_mask_tail_f32",
               "advhip_pack_padded_f32", "advhip_crop_mean_scatter_f32")


def _check(lengths, buckets, batch_videos, ncrops, max_rows):
    assert sorted(i for b in buckets for i in b) == list(range(len(lengths)))  # every index in exactly one bucket
    assert all(b for b in buckets)
    for b in buckets:
        assert len(b) <= batch_videos
        assert len(b) == 1 or len(b) * ncrops * max(lengths[i] for i in b) <= max_rows
    flat = [i for b in buckets for i in b]
    assert flat == sorted(range(len(lengths)), key=lambda i: (lengths[i], i))  # length order, ties by index (stable)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plan_buckets_properties(seed):
    from anomaly_detection_on_video_amd.val_batch import plan_buckets

    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, 40, 57).tolist()  # many ties
    for batch_videos, ncrops, max_rows in ((1, 10, 10**9), (4, 10, 10**9), (16, 3, 400), (5, 10, 10), (100, 1, 10**9), (7, 2, 77)):
        buckets = plan_buckets(lengths, batch_videos, ncrops, max_rows)
        _check(lengths, buckets, batch_videos, ncrops, max_rows)
        assert buckets == plan_buckets(list(lengths), batch_videos, ncrops, max_rows)  # deterministic
        if batch_videos == 1:
            assert all(len(b) == 1 for b in buckets)
    assert plan_buckets([], 4, 10) == []
    # a video that alone exceeds max_rows is a bucket of one, and closes the bucket before it
    assert plan_buckets([5, 100, 6, 7], 16, 10, max_rows=200) == [[0, 2], [3], [1]]
    assert plan_buckets([3, 3, 3, 3, 3], 2, 1) == [[0, 1], [2, 3], [4]]
    for bad in ((0, 10, 10), (4, 0, 10), (4, 10, 0)):
        with pytest.raises(ValueError):
            plan_buckets([3, 4], *bad)
    with pytest.raises(ValueError):
        plan_buckets([3, 0], 4, 10)


@pytest.mark.parametrize("seed,ratio", [(0, 1.039), (1, 1.042), (2, 1.043)])
def test_ucf_sized_length_set_needs_19_passes_and_pads_under_5_percent(seed, ratio):
    from anomaly_detection_on_video_amd.val_batch import padding_ratio, plan_buckets

    lengths = np.random.default_rng(seed).integers(50, 501, 290).tolist()
    buckets = plan_buckets(lengths, 16, 10)
    _check(lengths, buckets, 16, 10, 163_840)
    got = padding_ratio(lengths, buckets)
    print(f"seed {seed}: {len(buckets)} buckets, padded / real positions {got:.4f}")
    assert len(buckets) == 19 and got <= 1.05
    assert abs(got - ratio) < 1e-3  # the figure the feature was proposed with


def test_val_batch_imports_without_torch_at_module_level():
    src = open(os.path.join(REPO, "anomaly_detection_on_video_amd", "val_batch.py")).read()
    top = [ln for ln in src.splitlines() if re.match(r"(import|from)\s", ln)]
    assert top and not any("torch" in ln for ln in top), top


_CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "int": C.c_int}


def _declared(name):
    text = open(os.path.join(REPO, "include", "advhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/advhip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "*" in a:
            args.append(C.c_void_p)
        else:
            args.append(_CTYPE[a.replace("const", "").split()[0]])
    return _CTYPE[m.group(1)], args


def test_new_entry_points_are_declared_bound_and_exported():
    import __graft_entry__

    __graft_entry__.build()
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    assert lib.advhip_abi_version() == 2
    for name in NEW_SYMBOLS:
        res, args = _declared(name)
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert _lib.SIGNATURES[name] == (res, args), f"{name}: include/advhip.h and _lib.SIGNATURES disagree"
        assert hasattr(lib, name), f"{name} is not exported"
    # null pointers and bad shapes are refused before anything is launched (no GPU needed)
    assert lib.advhip_mask_tail_f32(None, 4, 4, 4, None, None) != 0 and b"mask_tail" in lib.advhip_last_error()
    assert lib.advhip_glance_attention_fwd_lens_f32(None, None, None, 1, 1, 8, 64, 0.125, None) != 0
    assert lib.advhip_crop_mean_scatter_f32(None, None, None, None, 1, 1, 1, None) != 0


def test_config_default_is_per_video_validation():
    from anomaly_detection_on_video_amd.config import compose

    cfg = compose(os.path.join(REPO, "configs"), "default", [])
    assert cfg.data.val_batch_videos == 1
    cfg = compose(os.path.join(REPO, "configs"), "default", ["data=synthetic", "data.val_batch_videos=16"])
    assert cfg.data.val_batch_videos == 16


def test_lens_ops_refuse_autograd_and_cpu_tensors():
    import torch

    from anomaly_detection_on_video_amd import _lib, mgfn_ops
    from anomaly_detection_on_video_amd.models.mgfn import MGFNConfig, MGFNForVideoAnomalyDetection

    x = torch.zeros(192, 2, 8)
    with pytest.raises(_lib.HipExtensionError, match="no backward"):
        mgfn_ops.glance_attention_core(x, 1, 64, 0.125, lens=[8, 8])
    with pytest.raises(_lib.HipExtensionError, match="no backward"):
        mgfn_ops.mask_tail_(x, [8, 8])
    with torch.no_grad(), pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        mgfn_ops.mask_tail_(x, [8, 8])
    model = MGFNForVideoAnomalyDetection(MGFNConfig(dims=(64, 128, 1024), depths=(1, 1, 1))).eval()
    with pytest.raises(_lib.HipExtensionError, match="no CPU fallback"):
        model.score_padded(torch.zeros(2, 3, 8, 2049), [8, 8])
    model.train()
    with pytest.raises(_lib.HipExtensionError, match="eval mode only"):
        model.score_padded(torch.zeros(2, 3, 8, 2049), [8, 8])
