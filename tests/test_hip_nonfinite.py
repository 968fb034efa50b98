"""NaN stays NaN and stays in its crop-clip: non-finite values through the conv kernels, the fused pooling epilogues and I3Res50
(run with -m gpu on an MI355X).

A constant crop or channel under the min-max normalisers is 0 / 0 = NaN, as in the reference, so NaN pixels reach the backbone.
The rule is torch's (tests/test_nonfinite_host.py pins it on the oracle): ReLU, max-pooling and the mean propagate NaN, a conv's NaN
mask is the receptive-field footprint, and no other clip of the launch sees anything.  Every comparison here is exact: NaN masks
equal the CPU oracle's, and outside the mask the output equals, bit for bit, the same launch (same tile, same split, so the same K
order) with the poisoned element set to 0.0 -- a launch the other test files pin to the oracle.  No tolerance anywhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_fused_pool import AVG_CASES, S2W_CASES, STEM_SHAPES, TPOOL_SHAPES
from test_hip_fused_pool import _pack as _pool_pack
from test_hip_i3d import _skip_algo
from test_hip_normalize import form  # noqa: F401  (the fixture: every uint8 stem form)
from test_nonfinite_host import (ALL_CASES, BACKBONE_SHAPE, BACKBONE_SITE, BLACK_F, CONST_FRAME, CROP, EPILOGUES, FPC, INF,
                                 MINMAX_MODES, NAN, NAN_SHARE_CAP, NF_CONV_CASES, ONE_POSITION, PERSIST_CASE, STANDARDIZE, STRIDE_SKIPS_P3,
                                 TFOLD_CASE, backbone_input, backbone_oracle_masks, black_frame_video, constant_corner_video, conv_operands,
                                 conv_oracle, footprint, poison_sites, poisoned, residual_sites)
from anomaly_detection_on_video_amd.weights import synth_i3d_state_dict, synth_tensor

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _case(name):
    return next(c for c in ALL_CASES if c[0] == name)


_PACKED = {}


def _packed(name):
    """The case's packed conv and its operands on the device, once per case."""
    from anomaly_detection_on_video_amd import ops

    if name not in _PACKED:
        _n, _cin, _cout, _k, s, p, _bthw = _case(name)
        x, wt, g, be, mu, var, res = conv_operands(name)
        dev = _dev()
        pc = ops.pack_conv(wt.to(dev), g.to(dev), be.to(dev), mu.to(dev), var.to(dev), 1e-5, s, p, name=name)
        _PACKED[name] = (pc, x.to(dev), res.to(dev))
    return _PACKED[name]


def _same_outside(out, clean, mask):
    """`out` == `clean` bit for bit on the complement of `mask`"""
    keep = ~mask
    return torch.equal(out[keep], clean[keep])


def _check_conv(name, algo, splits, bad):
    """Every epilogue and every poison of one (case, kernel, split): appends what fails to `bad`."""
    from anomaly_detection_on_video_amd import ops

    _n, _cin, cout, k, s, p, _bthw = _case(name)
    pc, xd, rd = _packed(name)
    one_pos = name.endswith(ONE_POSITION)

    def run(x, res, relu):
        return ops.conv3d_bn_act(x, pc, relu=relu, residual=res, algo=algo, splits=splits).cpu()

    for use_res, relu in EPILOGUES:
        tag = f"{name} algo={algo} splits={splits} res={use_res} relu={relu}"
        for pname, site in poison_sites(xd.shape).items():
            foot = footprint(xd.shape, cout, k, s, p, site)
            share = float(foot.float().mean())
            assert one_pos or 1.0 - share >= 1.0 - NAN_SHARE_CAP  # what is compared bit for bit: at least 65 % of the output
            if pname == "P3":
                assert foot.any() != name.endswith(STRIDE_SKIPS_P3)
            ref = conv_oracle(name, pname, use_res, relu)
            assert torch.equal(torch.isnan(ref), foot)
            res = rd if use_res else None
            clean = run(poisoned(xd, site, 0.0), res, relu)
            assert torch.isfinite(clean).all()
            out = run(poisoned(xd, site), res, relu)
            if not torch.equal(torch.isnan(out), torch.isnan(ref)):
                bad.append(f"{tag} {pname}: NaN mask differs from the oracle's ({int(torch.isnan(out).sum())} NaN, oracle {int(foot.sum())}; "
                           f"{int(torch.isnan(out[1:]).sum())} in samples >= 1)")
            if torch.isnan(out[1:]).any():
                bad.append(f"{tag} {pname}: NaN in samples >= 1")
            if not _same_outside(out, clean, foot):
                bad.append(f"{tag} {pname}: differs outside the footprint from the launch with 0.0 there")
            if pname == "P3":  # P5: +inf there
                ref = conv_oracle(name, "P3", use_res, relu, INF)
                out = run(poisoned(xd, site, INF), res, relu)
                for what, fn in (("isnan", torch.isnan), ("isposinf", torch.isposinf), ("isneginf", torch.isneginf)):
                    if not torch.equal(fn(out), fn(ref)):
                        bad.append(f"{tag} P5: {what} differs from the oracle's ({int(fn(out).sum())} vs {int(fn(ref).sum())})")
                if not _same_outside(out, clean, foot):
                    bad.append(f"{tag} P5: differs outside the footprint from the launch with 0.0 there")
        if use_res:  # P4: x clean, two NaN in the residual of sample 0
            rp = rd.clone()
            mask = torch.zeros(rd.shape, dtype=torch.bool)
            for rsite in residual_sites(rd.shape):
                rp[rsite] = NAN
                mask[rsite] = True
            assert torch.equal(torch.isnan(conv_oracle(name, "P4", True, relu)), mask)
            out, clean = run(xd, rp, relu), run(xd, rd, relu)
            if not torch.equal(torch.isnan(out), mask):
                bad.append(f"{tag} P4: NaN at {torch.isnan(out).nonzero().tolist()[:6]} (of {int(torch.isnan(out).sum())}), want exactly {mask.nonzero().tolist()}")
            if not _same_outside(out, clean, mask):
                bad.append(f"{tag} P4: differs from the clean launch outside the two elements")


# one id per kernel family: auto, igemm 64x64, fast 64x64, LDS-DMA 3-deep 64x64, 4-deep 64x64, 2-deep 128x64 / 64x64 / 64x128 / 256x64, split-bf16 128x64
ALGOS = [0, 3, 35, 67, 99, 162, 163, 164, 169, 134]


@pytest.mark.parametrize("case", NF_CONV_CASES, ids=[c[0] for c in NF_CONV_CASES])
@pytest.mark.parametrize("algo", ALGOS, ids=[f"algo{a}" for a in ALGOS])
def test_conv_nan_mask_is_the_footprint_and_the_rest_is_untouched(case, algo):
    _skip_algo(algo, case[2], case[3])
    bad = []
    _check_conv(case[0], algo, 1, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["l1.conv3", "edge.7x7"])
@pytest.mark.parametrize("algo", [3, 67, 163, 169])
@pytest.mark.parametrize("splits", [2, 3])
def test_conv_split_k_nan_mask(name, algo, splits):
    """slab reduction (the reduce pass) and the reduction inside the kernel"""
    bad = []
    _check_conv(name, algo, splits, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("family", ["tspan", "mixed", "tfold", "persist"])
def test_conv_special_families_nan_mask(family):
    """TSPAN on the temporal conv, the mixed tail on the 1x1x1 conv, the T-fold family on its first case, the persistent family on its
    first small case."""
    from anomaly_detection_on_video_amd import _lib

    cout_t = TFOLD_CASE[2] * TFOLD_CASE[6][1]  # the folded conv's channels: tiles whose N does not divide them are not instantiated for it
    runs = {"tspan": [("l1.conv1.t3", _lib.ALGO_TSPAN_128x64)], "mixed": [("l1.conv3", _lib.ALGO_MIXED_128x64)],
            "tfold": [(TFOLD_CASE[0], a) for a in _lib.TFOLD_ALGOS if cout_t % _lib.algo_tile(a)[1] == 0],
            "persist": [(PERSIST_CASE[0], a) for a in _lib.PERSIST_ALGOS]}[family]
    assert len(runs) >= (4 if family in ("tfold", "persist") else 1)
    bad = []
    for name, algo in runs:
        _check_conv(name, algo, 1, bad)
    assert not bad, "\n".join(bad)


# ---- nothing outside an operand is read into a result ----------------------------------------------------------------------------

def test_conv_and_pool_on_channel_slices_of_nan_filled_buffers():
    """test_conv_and_pool_on_channel_slices with NaN as the fill: x a channel slice of a NaN-filled buffer, the residual a slice of a
    NaN-filled buffer (whole samples either side: the residual is contiguous), out a slice of a NaN-prefilled buffer.  A kernel
    that multiplied a neighbour by a zero weight, or added a masked lane's load, would show it."""
    from anomaly_detection_on_video_amd import _lib, ops

    dev = _dev()
    for name in ("l1.conv2", "l1.conv1.t3", "stem"):
        _n, cin, cout, _k, _s, _p, bthw = _case(name)
        pc, xd, rd = _packed(name)
        b = bthw[0]
        wide_in = torch.full((b, cin + 24) + tuple(xd.shape[2:]), NAN, device=dev)
        wide_in[:, 8 : 8 + cin] = xd
        wide_res = torch.full((b + 2,) + tuple(rd.shape[1:]), NAN, device=dev)
        wide_res[1 : 1 + b] = rd
        dense = ops.conv3d_bn_act(xd, pc, relu=True, residual=rd)
        assert torch.isfinite(dense).all()
        algos = [None, 3, 35, 67, 163, 134] + ([_lib.ALGO_TSPAN_128x64] if name == "l1.conv1.t3" else [])
        for algo in algos:
            want = dense if algo is None else ops.conv3d_bn_act(xd, pc, relu=True, residual=rd, algo=algo)
            wide_out = torch.full((b, cout + 40) + tuple(rd.shape[2:]), NAN, device=dev)
            got = ops.conv3d_bn_act(wide_in[:, 8 : 8 + cin], pc, relu=True, residual=wide_res[1 : 1 + b], out=wide_out[:, 16 : 16 + cout], algo=algo)
            assert torch.isfinite(got).all(), (name, algo)
            assert torch.equal(got, want), (name, algo)
            assert torch.isnan(wide_out[:, :16]).all() and torch.isnan(wide_out[:, 16 + cout :]).all(), (name, algo)
            assert torch.isnan(wide_in[:, :8]).all() and torch.isnan(wide_in[:, 8 + cin :]).all() and torch.equal(wide_in[:, 8 : 8 + cin], xd)
            assert torch.isnan(wide_res[0]).all() and torch.isnan(wide_res[-1]).all()
    xp = synth_tensor("slice.pool", (2, 6, 4, 12, 10), scale=2.0).to(dev)
    for kk, ss in (((2, 3, 3), (2, 2, 2)), ((2, 1, 1), (2, 1, 1)), ((1, 2, 2), (1, 1, 1))):
        ref = ops.maxpool3d(xp, kk, ss)
        wide = torch.full((2, 11) + tuple(ref.shape[2:]), NAN, device=dev)
        ops.maxpool3d(xp, kk, ss, out=wide[:, 3:9])
        assert torch.equal(wide[:, 3:9], ref) and torch.isfinite(ref).all()
        assert torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 9:]).all()


# ---- fused pooling epilogues ------------------------------------------------------------------------------------------------------

def _check_fused(fused_fn, unfused_fn, oracle_fn, x, label, value_sites):
    """For every poison: fused(x) has the unfused pair's NaN mask and its bits elsewhere, the oracle's NaN mask, and no NaN in samples
    >= 1.  oracle_fn takes sample 0 alone (samples are independent)."""
    bad = []
    xd = x.to(_dev())
    for pname, site in value_sites.items():
        xp = poisoned(xd, site)
        got, want = fused_fn(xp).cpu(), unfused_fn(xp).cpu()
        ref_mask = torch.isnan(oracle_fn(poisoned(x[:1], site)))
        assert ref_mask.any() and got.shape == want.shape
        if not torch.equal(torch.isnan(got[:1]), ref_mask):
            bad.append(f"{label} {pname}: {int(torch.isnan(got[:1]).sum())} NaN in sample 0, oracle {int(ref_mask.sum())}")
        if torch.isnan(got[1:]).any():
            bad.append(f"{label} {pname}: NaN in samples >= 1")
        if not torch.equal(torch.isnan(got), torch.isnan(want)):
            bad.append(f"{label} {pname}: NaN mask differs from conv + pool ({int(torch.isnan(got).sum())} vs {int(torch.isnan(want).sum())})")
        full = torch.zeros(got.shape, dtype=torch.bool)
        full[:1] = ref_mask
        clean = fused_fn(poisoned(xd, site, 0.0)).cpu()
        if not (_same_outside(got, want, full) and _same_outside(got, clean, full)):
            bad.append(f"{label} {pname}: differs outside the NaN mask from conv + pool, or from the launch with 0.0 there")
    return bad


def _two(shape):
    return (max(2, shape[0]),) + tuple(shape[1:])


@pytest.mark.parametrize("s2w", [False, True], ids=["plain", "planes"])
def test_stem_maxpool233_epilogue_propagates_nan(s2w):
    """conv3d_bn_relu_maxpool233 on STEM_SHAPES[0] and its column-parity planes form on S2W_CASES[0] (the same stem at full size)."""
    from anomaly_detection_on_video_amd import ops
    from oracle import i3d_oracle

    b, t, h, w = _two(S2W_CASES[0][6] if s2w else STEM_SHAPES[0])
    pc, (wt, g, be, mu, var) = _pool_pack("stem", 3, 64, (5, 7, 7), (2, 2, 2), (2, 3, 3))
    assert ops.s2w_ok(pc, w)
    x = synth_tensor(f"nf.stem.x{(b, t, h, w)}", (b, 3, t, h, w), scale=2.0)
    bad = _check_fused(lambda v: ops.conv3d_bn_relu_maxpool233(v, pc, s2w=s2w),
                       lambda v: ops.maxpool3d(ops.conv3d_bn_act(v, pc, relu=True, algo=162), (2, 3, 3), (2, 2, 2)),
                       lambda v: F.max_pool3d(i3d_oracle.conv_bn_act(v, wt, g, be, mu, var, (2, 2, 2), (2, 3, 3), None, True), (2, 3, 3), (2, 2, 2)),
                       x, f"stem+pool233 s2w={s2w}", poison_sites(x.shape))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("use_res,relu", [(True, True), (False, True), (True, False)])
def test_maxpool211_epilogue_propagates_nan(use_res, relu):
    from anomaly_detection_on_video_amd import ops
    from oracle import i3d_oracle

    cin, cout = 64, 256
    b, t, h, w = _two(TPOOL_SHAPES[0])
    pc, (wt, g, be, mu, var) = _pool_pack(f"tp{cin}", cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    x = synth_tensor(f"nf.tp.x{(b, t, h, w)}", (b, cin, t, h, w), scale=2.0)
    res = synth_tensor(f"nf.tp.r{(b, t, h, w)}", (b, cout, t, h, w), scale=1.0)
    rd = res.to(_dev()) if use_res else None
    bad = _check_fused(lambda v: ops.conv3d_bn_act_maxpool211(v, pc, relu=relu, residual=rd),
                       lambda v: ops.maxpool3d(ops.conv3d_bn_act(v, pc, relu=relu, residual=rd, algo=162), (2, 1, 1), (2, 1, 1)),
                       lambda v: F.max_pool3d(i3d_oracle.conv_bn_act(v, wt, g, be, mu, var, (1, 1, 1), (0, 0, 0), res[:1] if use_res else None, relu), (2, 1, 1), (2, 1, 1)),
                       x, f"conv+pool211 res={use_res} relu={relu}", poison_sites(x.shape))
    assert not bad, "\n".join(bad)


def test_avgpool_epilogue_propagates_nan():
    from anomaly_detection_on_video_amd import _lib, ops
    from oracle import i3d_oracle

    b, cin, cout, thw, with_res = AVG_CASES[0]
    b = max(2, b)
    pc, (wt, g, be, mu, var) = _pool_pack(f"avg{cin}x{cout}", cin, cout, (1, 1, 1), (1, 1, 1), (0, 0, 0))
    x = synth_tensor(f"nf.avg.x{(b, cin) + thw}", (b, cin) + thw, scale=2.0)
    res = synth_tensor(f"nf.avg.r{(b, cout) + thw}", (b, cout) + thw, scale=1.0) if with_res else None
    rd = res.to(_dev()) if with_res else None
    assert ops.avgpool_fusable(pc, thw)
    bad = _check_fused(lambda v: ops.conv3d_bn_act_avgpool(v, pc, relu=True, residual=rd),
                       lambda v: ops.global_avgpool(ops.conv3d_bn_act(v, pc, relu=True, residual=rd, algo=_lib.ALGO_DMA2_BASE + _lib.ALGO_IGEMM_64x64, splits=1)),
                       lambda v: F.adaptive_avg_pool3d(i3d_oracle.conv_bn_act(v, wt, g, be, mu, var, (1, 1, 1), (0, 0, 0), res[:1] if with_res else None, True), 1),
                       x, "conv+mean", poison_sites(x.shape))
    assert not bad, "\n".join(bad)


# ---- the whole backbone -----------------------------------------------------------------------------------------------------------

_MODEL = {}


def _model():
    from anomaly_detection_on_video_amd.i3d import I3Res50

    if "m" not in _MODEL:
        m = I3Res50()
        m.load_state_dict(synth_i3d_state_dict())
        _MODEL["m"] = m.eval().to(_dev())
    m = _MODEL["m"]
    m.fuse_pool, m.streams = True, 2
    return m


class _Taps(dict):
    """forward_single's `taps` with every write kept in order (both max-pools are named "maxpool")"""

    def __init__(self):
        super().__init__()
        self.order = []

    def __setitem__(self, k, v):
        self.order.append((k, v))
        super().__setitem__(k, v)


def _rows_check(y, y0, nan_rows, label):
    """rows `nan_rows` of y all NaN; every other row finite and bit-equal to y0's (the same call with 0.0 for the NaN)"""
    y, y0 = y.reshape(-1, 2048).cpu(), y0.reshape(-1, 2048).cpu()
    assert y.shape == y0.shape and torch.isfinite(y0).all(), label
    bad = []
    for r in range(y.shape[0]):
        if r in nan_rows:
            if not torch.isnan(y[r]).all():
                bad.append(f"{label}: row {r} holds {int(torch.isnan(y[r]).sum())} NaN of 2048, want all (finite features of a clip with a NaN pixel)")
        elif not torch.isfinite(y[r]).all():
            bad.append(f"{label}: row {r} of a clean clip holds {int((~torch.isfinite(y[r])).sum())} non-finite values")
        elif not torch.equal(y[r], y0[r]):
            bad.append(f"{label}: row {r} of a clean clip changed with another clip's pixel")
    return bad


def test_backbone_one_nan_pixel_poisons_its_row_only():
    from anomaly_detection_on_video_amd import ops

    m = _model()
    dev = _dev()
    assert m.fuse_pool and ops.FUSE_AVGPOOL
    x, x0 = backbone_input().to(dev), backbone_input(value=0.0).to(dev)
    masks, ymask = backbone_oracle_masks()
    assert ymask.reshape(3, 2048).all(dim=1).tolist() == [False, True, False]
    bad = _rows_check(m(x), m(x0), {1}, "production forward")
    # the production path ran: the stem pools (column-parity planes form), layer1.2.conv3 pools, layer4.2.conv3 takes the mean
    assert sum(1 for u in m._plan if u.absorbed) == 3 and all(u.pool_unit is not None for u in m._plan if u.kind == "stem")
    assert m.frames_fused() and ops.s2w_ok(m._plan[0].convs[0], BACKBONE_SHAPE[-1]) and ops.avgpool_fusable(m._plan[-2].convs[2], (2, 2, 2))
    try:
        m.fuse_pool = False
        bad += _rows_check(m(x), m(x0), {1}, "fuse_pool = False")
    finally:
        m.fuse_pool = True
    taps = _Taps()
    y_t = m.forward_single(x, taps)
    bad += _rows_check(y_t, m.forward_single(x0, {}), {1}, "forward_single with taps")
    pools = iter(("maxpool1", "maxpool2"))
    seen = []
    for name, v in taps.order:
        key = next(pools) if name == "maxpool" else name
        seen.append(key)
        if not torch.equal(torch.isnan(v).cpu(), masks[key]):
            bad.append(f"tap {key}: {int(torch.isnan(v).sum())} NaN, oracle {int(masks[key].sum())}")
    for lname in ("layer1", "layer2", "layer3", "layer4"):  # the oracle's stage outputs = the stage's last block
        last = [k for k in seen if k.startswith(lname + ".")][-1]
        assert torch.equal(masks[lname], masks[last])
    assert set(seen) | {"layer1", "layer2", "layer3", "layer4"} == set(masks), sorted(set(masks) - set(seen))
    assert not bad, "\n".join(bad)


def test_backbone_nan_rows_on_two_streams():
    """B = 17 on two streams (parts of 8 and 9 clips): the first clip of each part and the last clip poisoned."""
    m = _model()
    dev = _dev()
    assert m._n_streams(17) == 2
    shape = (17,) + BACKBONE_SHAPE[1:]
    sites = tuple((c,) + BACKBONE_SITE[1:] for c in (0, 8, 16))
    y = m(backbone_input(shape, sites).to(dev))
    y0 = m(backbone_input(shape, sites, 0.0).to(dev))
    bad = _rows_check(y, y0, {0, 8, 16}, "B = 17, two streams")
    assert not bad, "\n".join(bad)


def test_black_frame_through_the_minmax_modes(form):  # noqa: F811
    """Frame 20 of 53 all zeros: 0 / 0 in every crop of it under both min-max modes, so every row of its windows is NaN and no other
    row notices; per-channel standardisation of the same frames is the negative control."""
    from anomaly_detection_on_video_amd.extract import extract_video_frames

    m = _model()
    black, noise = black_frame_video()
    assert black.shape[0] == BLACK_F
    bad = []
    fb, fn = torch.from_numpy(black).to(_dev()), torch.from_numpy(noise).to(_dev())
    for mode in MINMAX_MODES + (STANDARDIZE,):
        kw = dict(crop=CROP, crops="center_flip", normalize=mode, max_crop_clips=2, clips_per_step=3)
        for stride, windows in ((None, (1,)), (8, (1, 2))):
            got = extract_video_frames(m, torch.from_numpy(black), clip_stride=stride, **kw)
            ref = extract_video_frames(m, torch.from_numpy(noise), clip_stride=stride, **kw)
            assert got.shape == ref.shape == (4 if stride is None else 6, 2, 2048)
            label = f"extract_video_frames {form} {mode} stride={stride}"
            if mode == STANDARDIZE:
                assert np.isfinite(got).all() and np.isfinite(ref).all(), label
            else:
                bad += _rows_check(torch.from_numpy(got), torch.from_numpy(ref), {2 * w + j for w in windows for j in range(2)}, label)
        # all 40 crop-clips in one call (two streams): rows 10..19 are clip 1's
        y, y0 = m.forward_frames(fb, 0, 40, FPC, CROP, normalize=mode), m.forward_frames(fn, 0, 40, FPC, CROP, normalize=mode)
        if mode == STANDARDIZE:
            assert torch.isfinite(y).all() and torch.isfinite(y0).all()
        else:
            bad += _rows_check(y, y0, set(range(10, 20)), f"forward_frames {form} {mode}")
    assert not bad, "\n".join(bad)


def test_constant_channel_in_one_corner_window(form):  # noqa: F811
    """Channel 1 constant inside the top-left crop window of one frame, channel_minmax: crops 0 and 6 (crop 6 holds window 0's
    pixels) are 0 / 0 in that channel of that frame; the other eight crops hold other pixels too."""
    from anomaly_detection_on_video_amd import mil_ops

    m = _model()
    frames = constant_corner_video()
    assert 0 <= CONST_FRAME < FPC == frames.shape[0]
    fd = torch.from_numpy(frames).to(_dev())
    dense = mil_ops.tencrop_normalize_u8(fd, FPC, CROP, normalize="channel_minmax")
    assert sorted(set(torch.isnan(dense).reshape(10, -1).any(dim=1).nonzero().reshape(-1).tolist())) == [0, 6]
    want = m.forward_single(dense).reshape(10, 2048).cpu()
    got = m.forward_frames(fd, 0, 10, FPC, CROP, normalize="channel_minmax").reshape(10, 2048).cpu()
    bad = []
    for r in range(10):
        if r in (0, 6):
            if not torch.isnan(got[r]).all():
                bad.append(f"{form}: row (0, {r}) holds {int(torch.isnan(got[r]).sum())} NaN of 2048, want all")
        elif not torch.isfinite(got[r]).all():
            bad.append(f"{form}: row (0, {r}) is not finite")
    if not np.array_equal(got.numpy(), want.numpy(), equal_nan=True):
        bad.append(f"{form}: forward_frames differs from forward_single of the dense pass's pixels")
    assert not bad, "\n".join(bad)
