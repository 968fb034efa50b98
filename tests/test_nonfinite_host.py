"""Non-finite values on the reference's side (CPU): what tests/test_hip_nonfinite.py compares the kernels with.

The min-max normalisers give 0 / 0 = NaN for a constant crop or channel (tests/_normalize_ref.py), so NaN pixels are an ordinary
input of the backbone.  The rule the kernels have to keep is torch's: relu / clamp_min, max_pool3d and the mean propagate NaN, a
conv's NaN mask is the receptive-field footprint of the NaN inputs, and nothing crosses from one crop-clip to another.  This file
pins those expectations on the oracle itself -- a mistake in an expectation shows up here, not on the GPU -- and holds the cases,
poison positions and frames the GPU file imports."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _normalize_ref import tencrop_ref
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_input
from test_hip_i3d import CONV_CASES, _conv_case
from test_hip_persist import SMALL as PERSIST_SMALL
from test_hip_tfold import CASES as TFOLD_CASES

NAN, INF = float("nan"), float("inf")

# the smallest conv shapes the suite has, in CONV_CASES form: (name, Cin, Cout, kernel, stride, padding, (B, T, H, W))
CONV_NAMES = ("stem", "l1.conv1.t3", "l1.conv2", "l1.conv3", "l2.conv2.s2", "l2.ds.s2", "edge.7x7", "edge.odd", "edge.1pos")
NF_CONV_CASES = [next(c for c in CONV_CASES if c[0] == n) for n in CONV_NAMES]
assert [c[0] for c in NF_CONV_CASES] == list(CONV_NAMES)
_n, _ci, _co, _kt, _bthw = TFOLD_CASES[0]
TFOLD_CASE = ("tfold." + _n, _ci, _co, (_kt, 1, 1), (1, 1, 1), (_kt // 2, 0, 0), _bthw)
_n, _ci, _co, _bthw = PERSIST_SMALL[0]
PERSIST_CASE = ("persist." + _n, _ci, _co, (1, 1, 1), (1, 1, 1), (0, 0, 0), _bthw)
ALL_CASES = NF_CONV_CASES + [TFOLD_CASE, PERSIST_CASE]

EPILOGUES = ((False, True), (True, True), (True, False))  # (residual, ReLU)
ONE_POSITION = "edge.1pos"       # one output position: every poison is the whole footprint
STRIDE_SKIPS_P3 = "l2.ds.s2"     # P3 is an odd position of a 1x1x1 stride-2 conv: no output reads it
NAN_SHARE_CAP = 0.35             # largest NaN share of an output over all (case, poison) but the one-position case: 1/3, edge.odd / P3


def poison_sites(xshape):
    """The three input elements that are poisoned, one launch each, always in sample 0: the tensor's first element (which rows
    past M alias), sample 0's last element (adjacent in memory to sample 1), and an interior one."""
    _b, cin, t, h, w = xshape
    return {"P1": (0, 0, 0, 0, 0), "P2": (0, cin - 1, t - 1, h - 1, w - 1), "P3": (0, cin // 2, t // 2, h // 2, w // 2)}


def out_dims(thw, k, s, p):
    return tuple((thw[i] + 2 * p[i] - k[i]) // s[i] + 1 for i in range(3))


def footprint(xshape, cout, k, s, p, site):
    """bool (B, Cout, To, Ho, Wo): the outputs whose receptive field holds input element `site` -- every channel of the site's sample
    at the positions o with o * stride - pad + tap == site for a tap in [0, kernel), per axis."""
    b = xshape[0]
    od = out_dims(xshape[2:], k, s, p)
    axes = []
    for i in range(3):
        o = torch.arange(od[i])
        tap = site[2 + i] - (o * s[i] - p[i])
        axes.append((tap >= 0) & (tap < k[i]))
    m = torch.zeros((b, cout) + od, dtype=torch.bool)
    m[site[0]] = (axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :])[None]
    return m


def residual_sites(yshape):
    """P4: the first and the last element of sample 0 of the residual."""
    return [(0, 0, 0, 0, 0), (0,) + tuple(d - 1 for d in yshape[1:])]


def poisoned(x, site, value=NAN):
    x = x.clone()
    x[site] = value
    return x


@functools.lru_cache(maxsize=None)
def conv_operands(name):
    """(x, w, gamma, beta, mean, var, res) of a case, built once and never written to (poisoned() copies)."""
    return _conv_case(*next(c for c in ALL_CASES if c[0] == name))


@functools.lru_cache(maxsize=None)
def conv_oracle(name, poison, use_res, relu, value=NAN):
    """i3d_oracle.conv_bn_act on the poisoned operands (P1-P3: x; P4: the residual), computed once per argument set."""
    from oracle import i3d_oracle

    _name, _cin, _cout, _k, s, p, _bthw = next(c for c in ALL_CASES if c[0] == name)
    x, wt, g, be, mu, var, res = conv_operands(name)
    if poison == "P4":
        assert use_res
        res = res.clone()
        for site in residual_sites(res.shape):
            res[site] = value
    else:
        x = poisoned(x, poison_sites(x.shape)[poison], value)
    return i3d_oracle.conv_bn_act(x, wt, g, be, mu, var, s, p, res if use_res else None, relu)


def test_torch_relu_and_pools_propagate_nan():
    v = torch.tensor([NAN, -1.0, 2.0, -INF, INF])
    assert torch.isnan(torch.relu(v)).tolist() == [True, False, False, False, False]
    assert torch.relu(v)[1:].tolist() == [0.0, 2.0, 0.0, INF]
    assert torch.isnan(v.clamp_min(0)).tolist() == [True, False, False, False, False]
    x = torch.zeros(1, 1, 4, 6, 6)
    x[0, 0, 1, 2, 3] = NAN
    got = torch.isnan(F.max_pool3d(x, (2, 3, 3), (2, 2, 2)))
    want = torch.zeros(1, 1, 2, 2, 2, dtype=torch.bool)
    want[0, 0, 0, 0:2, 1] = True  # t window 0; rows 0-2 and 2-4; columns 2-4 only
    assert torch.equal(got, want)
    assert torch.equal(torch.isnan(F.max_pool3d(x, (2, 1, 1), (2, 1, 1))), torch.isnan(x[:, :, 1::2]))
    assert torch.isnan(F.adaptive_avg_pool3d(x, 1)).all()
    assert not torch.isnan(F.adaptive_avg_pool3d(torch.nan_to_num(x), 1)).any()


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_conv_oracle_nan_mask_is_the_receptive_field_footprint(case):
    name, cin, cout, k, s, p, bthw = case
    x, _wt, _g, _be, _mu, _var, res = conv_operands(name)
    for pname, site in poison_sites(x.shape).items():
        foot = footprint(x.shape, cout, k, s, p, site)
        assert not foot[1:].any()
        share = float(foot.float().mean())
        if name.endswith(ONE_POSITION):
            assert foot[0].all()
        else:
            assert share <= NAN_SHARE_CAP, (name, pname, share)
        if pname == "P3":
            assert foot.any() != name.endswith(STRIDE_SKIPS_P3), (name, "P3 must be read by some output except where the stride skips it")
        for use_res, relu in EPILOGUES:
            assert torch.equal(torch.isnan(conv_oracle(name, pname, use_res, relu)), foot), (name, pname, use_res, relu)
        # +inf at P3: one infinite term per output of the footprint, signed by its weight; nothing is NaN; ReLU takes -inf to 0
        if pname == "P3":
            for use_res, relu in EPILOGUES:
                y = conv_oracle(name, "P3", use_res, relu, INF)
                assert not torch.isnan(y).any() and not torch.isinf(y[~foot]).any()
                assert torch.isinf(y[foot]).any() == bool(foot.any())
                if relu:
                    assert not torch.isneginf(y).any()
    # fp64 gives the same mask as fp32
    from oracle import i3d_oracle

    site = poison_sites(x.shape)["P3"]
    ops64 = [t.double() for t in conv_operands(name)]
    y64 = i3d_oracle.conv_bn_act(poisoned(ops64[0], site), *ops64[1:6], s, p, None, True)
    assert torch.equal(torch.isnan(y64), footprint(x.shape, cout, k, s, p, site))
    # P4: a NaN in the residual stays where it is, with and without ReLU
    want = torch.zeros(res.shape, dtype=torch.bool)
    for rsite in residual_sites(res.shape):
        want[rsite] = True
    assert int(want.sum()) == (1 if res[0].numel() == 1 else 2) and not want[1:].any()
    for relu in (True, False):
        assert torch.equal(torch.isnan(conv_oracle(name, "P4", True, relu)), want)


# ---- the whole backbone: one NaN pixel in clip 1 of three ------------------------------------------------------------------------

BACKBONE_SHAPE, BACKBONE_SEED, BACKBONE_SITE = (3, 3, 16, 64, 64), 21, (1, 1, 7, 30, 30)


def backbone_input(shape=BACKBONE_SHAPE, sites=(BACKBONE_SITE,), value=NAN):
    x = synth_input(shape, BACKBONE_SEED)
    for site in sites:
        x[site] = value
    return x


@functools.lru_cache(maxsize=None)
def backbone_oracle_masks():
    """({stage: isnan(stage output)} in the oracle's order, isnan(features)) of i3d_forward on backbone_input()."""
    from oracle import i3d_oracle

    masks = {}
    y = i3d_oracle.i3d_forward(backbone_input(), synth_i3d_state_dict(), tap=lambda n, v: masks.__setitem__(n, torch.isnan(v)))
    return masks, torch.isnan(y)


def test_backbone_oracle_keeps_a_nan_pixel_in_its_clip():
    masks, ymask = backbone_oracle_masks()
    assert ymask.reshape(3, 2048).sum(dim=1).tolist() == [0, 2048, 0]
    for name, m in masks.items():
        assert not m[0].any() and not m[2].any(), name  # no tap of clips 0 and 2 holds a NaN
    share = {n: float(m[1].float().mean()) for n, m in masks.items()}
    # the stem's mask is the footprint of the pixel (2 x 3 x 3 positions, every channel: 0.2 %); maxpool1 spreads it as a max-pool does
    stem = footprint(BACKBONE_SHAPE, 64, (5, 7, 7), (2, 2, 2), (2, 3, 3), BACKBONE_SITE)
    assert torch.equal(masks["stem"], stem) and int(stem.sum()) == 64 * 18
    assert torch.equal(masks["maxpool1"], F.max_pool3d(stem.float(), (2, 3, 3), (2, 2, 2)) > 0)
    assert 0.001 < share["stem"] < 0.003 and 0.015 < share["maxpool1"] < 0.025 and 0.30 < share["layer1"] < 0.42
    assert share["stem"] < share["maxpool1"] < share["layer1.0"] <= share["layer1.1"] <= share["layer1.2"] == share["layer1"] < 1.0
    assert torch.equal(masks["maxpool2"], F.max_pool3d(masks["layer1"].float(), (2, 1, 1), (2, 1, 1)) > 0)
    assert share["maxpool2"] < share["layer2.0"] < 1.0  # (9 of 16 positions per frame after the stride-2 conv)
    for name, m in masks.items():
        if name.startswith(("layer2", "layer3", "layer4", "avgpool")) and name != "layer2.0":
            assert m[1].all(), name  # the whole clip from layer2's second block on


# ---- uint8 frames whose min-max normalisation is 0 / 0 ---------------------------------------------------------------------------

FRAME_HW, CROP, FPC = (72, 90), 64, 16
BLACK_F, BLACK_FRAME = 53, 20             # the geometry of test_extract_video_frames_with_a_normalisation; frame 20 is in clip 1
MINMAX_MODES = ("pixel_minmax", "channel_minmax")
STANDARDIZE = ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375))  # the negative control: finite for any frame
CONST_FRAME, CONST_CHANNEL = 5, 1         # one clip of 16 frames; channel 1 constant inside frame 5's top-left crop window


def noise_frames(seed, n_frames):
    return np.random.default_rng(seed).integers(0, 256, size=(n_frames,) + FRAME_HW + (3,), dtype=np.uint8)


def black_frame_video():
    """(frames with frame 20 all zeros, the same video with seeded noise there)"""
    noise = noise_frames(188, BLACK_F)
    black = noise.copy()
    black[BLACK_FRAME] = 0
    return black, noise


def constant_corner_video():
    f = noise_frames(189, FPC)
    f[CONST_FRAME, :CROP, :CROP, CONST_CHANNEL] = 17
    return f


def _nan_rows(x):
    return sorted(set(np.nonzero(np.isnan(x).reshape(x.shape[0], -1).any(axis=1))[0].tolist()))


@pytest.mark.parametrize("clip_stride,windows", [(None, [1]), (8, [1, 2])])
def test_black_frame_is_nan_in_its_windows_only(clip_stride, windows):
    black, noise = black_frame_video()
    for mode in MINMAX_MODES:
        x = tencrop_ref(black, mode, FPC, CROP, clip_stride)
        assert _nan_rows(x) == [w * 10 + j for w in windows for j in range(10)]
        for w in windows:  # ... and there in the black frame only: every pixel of it, none of another frame
            t = BLACK_FRAME - w * (clip_stride or FPC)
            rows = x[w * 10 : w * 10 + 10]
            assert np.isnan(rows[:, :, t]).all() and not np.isnan(np.delete(rows, t, axis=2)).any()
        assert not np.isnan(tencrop_ref(noise, mode, FPC, CROP, clip_stride)).any()
        keep = [r for r in range(x.shape[0]) if r // 10 not in windows]
        assert np.array_equal(x[keep], tencrop_ref(noise, mode, FPC, CROP, clip_stride)[keep])
    assert np.isfinite(tencrop_ref(black, STANDARDIZE, FPC, CROP, clip_stride)).all()


def test_constant_channel_in_one_corner_window_is_nan_in_two_crops():
    """Crops 0 (top-left) and 6 (the mirrored frame's top-right = the frame's top-left window, columns reversed) hold exactly the
    window's pixels; every other crop overlaps it but holds other pixels of channel 1 as well."""
    x = tencrop_ref(constant_corner_video(), "channel_minmax", FPC, CROP)
    assert x.shape == (10, 3, FPC, CROP, CROP) and _nan_rows(x) == [0, 6]
    for r in (0, 6):
        m = np.isnan(x[r])
        assert m[CONST_CHANNEL, CONST_FRAME].all() and int(m.sum()) == CROP * CROP
    assert np.isfinite(tencrop_ref(constant_corner_video(), "pixel_minmax", FPC, CROP)).all()
