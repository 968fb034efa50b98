"""The stem + maxpool1 launch split by pool window in t (include/advhip.h: ADVHIP_ALGO_STEM_BORDER; run with -m gpu on an MI355X).

The pool windows at either end of the clip run frame by frame on 1(t) x 8(h) x 16(w) tiles that skip the k-tiles whose rows all
carry a temporal tap in the padding; the interior windows run the 2-frame bricks on a sub-range of brick rows; the merge pass
takes the max over the two frame slabs of a border window.  Whole k-tiles are skipped and K keeps its order, so the bar is
torch.equal against the single launch of the same build (border=False), plus the per-conv bound of tests/test_hip_i3d.py
(2e-5) against the CPU oracle's max_pool3d(conv_bn_act(...)).  The k-tile sets themselves are host arithmetic of the library:
test_active_ktile_lists_* need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from anomaly_detection_on_video_amd.weights import synth_tensor

TIGHT = 2e-5  # the per-conv bound of tests/test_hip_i3d.py

STEM = (3, 64, (5, 7, 7), (2, 2, 2), (2, 3, 3))

# (B, T, H, W), split expected
CASES = [
    ((2, 16, 32, 32), True),   # 2 border + 2 interior pool windows; Ho = 16, 4 brick rows
    ((1, 16, 48, 40), True),   # Wo = 20: a ragged last brick along w
    ((3, 8, 32, 32), True),    # To = 4: both windows are border, the interior launch is empty
    ((1, 16, 24, 32), False),  # Ho = 12, odd brick count: must take the single launch and still match
]


def _dev():
    return torch.device("cuda:0")


def _operands():
    cin, cout, k, s, p = STEM
    fan = cin * k[0] * k[1] * k[2]
    wt = synth_tensor("sb.stem.w", (cout, cin) + k, scale=float(np.sqrt(6.0 / fan)))
    g = synth_tensor("sb.stem.g", (cout,), scale=0.5, offset=1.0)
    be = synth_tensor("sb.stem.b", (cout,), scale=0.25)
    mu = synth_tensor("sb.stem.m", (cout,), scale=0.25)
    var = synth_tensor("sb.stem.v", (cout,), scale=0.5, offset=1.0)
    return wt, g, be, mu, var


def _pack(dev=None):
    from anomaly_detection_on_video_amd import ops

    dev = dev or _dev()
    wt, g, be, mu, var = _operands()
    return ops.pack_conv(wt.to(dev), g.to(dev), be.to(dev), mu.to(dev), var.to(dev), 1e-5, STEM[3], STEM[4], name="stem")


def _ws_bytes(pc, shape, border):
    from anomaly_detection_on_video_amd import _lib

    b, t, h, w = shape
    d = pc.desc(b, t, h, w, True, _lib.ALGO_STEM_BORDER if border else 0, 1)
    return int(_lib.load().advhip_conv3d_relu_maxpool233_workspace_bytes(C.byref(d)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,split", CASES, ids=[str(c[0]) for c in CASES])
def test_split_launch_equals_single_launch_and_oracle(shape, split):
    from anomaly_detection_on_video_amd import ops
    from oracle import i3d_oracle

    b, t, h, w = shape
    pc = _pack()
    wt, g, be, mu, var = _operands()
    x = synth_tensor(f"sb.x{shape}", (b, 3, t, h, w), scale=2.0)
    xd = x.to(_dev())
    assert ops.s2w_ok(pc, w)
    # the split launch keeps one more slab per border window: that it is (not) asked for says which path runs
    single_bytes, split_bytes = _ws_bytes(pc, shape, False), _ws_bytes(pc, shape, True)
    tp = (t // 2) // 2
    assert (split_bytes > single_bytes) == split
    if split:
        assert split_bytes * tp == single_bytes * (tp + min(tp, 2))
    old = ops.conv3d_bn_relu_maxpool233(xd, pc, s2w=True, border=False)
    new = ops.conv3d_bn_relu_maxpool233(xd, pc, s2w=True, border=True)
    again = ops.conv3d_bn_relu_maxpool233(xd, pc, s2w=True, border=True)
    assert new.shape == old.shape
    assert torch.equal(new, old), f"max diff {float((new - old).abs().max()):.3e}"
    assert torch.equal(new, again), "not run-to-run identical"
    assert torch.equal(new, ops.conv3d_bn_relu_maxpool233(xd, pc, s2w=False))  # the 4-byte gather: one launch in every case
    ref = torch.nn.functional.max_pool3d(i3d_oracle.conv_bn_act(x, wt, g, be, mu, var, STEM[3], STEM[4], None, True), (2, 3, 3), (2, 2, 2))
    e = rel_err(new.cpu(), ref)
    print(f"stem border {shape}: rel err vs oracle {e:.3e}")
    assert e < TIGHT
    # the default follows ADV_STEM_BORDER and gives the same bits either way
    assert torch.equal(ops.conv3d_bn_relu_maxpool233(xd, pc), old)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,split", CASES[:3], ids=[str(c[0]) for c in CASES[:3]])
def test_canaries_around_workspace_and_output(shape, split):
    """The entry point on a workspace of exactly the size it asks for, and an output that is a channel slice of a wider buffer:
    the floats either side of the workspace and the neighbouring channels stay as they were."""
    from anomaly_detection_on_video_amd import _lib, ops
    from anomaly_detection_on_video_amd.ops import batch_stride, check, ptr, stream

    b, t, h, w = shape
    dev = _dev()
    pc = _pack()
    xd = synth_tensor(f"sb.x{shape}", (b, 3, t, h, w), scale=2.0).to(dev)
    want = ops.conv3d_bn_relu_maxpool233(xd, pc, s2w=True, border=False)
    xs = ops.split_w(xd)
    d = pc.desc(b, t, h, w, True, _lib.ALGO_STEM_BORDER, 1)
    lib = _lib.load()
    need = int(lib.advhip_conv3d_relu_maxpool233_workspace_bytes(C.byref(d)))
    assert need > 0 and need % 4 == 0
    guard = 1024  # floats
    ws = torch.full((guard + need // 4 + guard,), -9.0, device=dev)
    wide = torch.full((b, 16 + 64 + 32) + tuple(want.shape[2:]), -7.0, device=dev)
    y = wide[:, 16:80]
    check(lib.advhip_conv3d_s2w_bn_relu_maxpool233_f32(C.byref(d), ptr(xs), 0, ptr(pc.w_packed), ptr(ops.ensure_ktab_s2w(pc, (t, h, w))), ptr(pc.scale),
                                                       ptr(pc.shift), ptr(y), batch_stride(y), ptr(ws[guard:]), need, stream(xs)), "s2w+pool233 border")
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    assert (ws[:guard] == -9.0).all() and (ws[guard + need // 4:] == -9.0).all(), "workspace canary overwritten"
    assert (wide[:, :16] == -7.0).all() and (wide[:, 80:] == -7.0).all(), "output canary overwritten"
    # one byte short of the size it asks for: refused before any launch
    rc = lib.advhip_conv3d_s2w_bn_relu_maxpool233_f32(C.byref(d), ptr(xs), 0, ptr(pc.w_packed), ptr(ops.ensure_ktab_s2w(pc, (t, h, w))), ptr(pc.scale),
                                                      ptr(pc.shift), ptr(y), batch_stride(y), ptr(ws[guard:]), need - 1, stream(xs))
    assert rc != 0


# ---- the active k-tile lists: host arithmetic, no GPU ------------------------------------------------------------------------

def _desc(T, algo=0):
    from anomaly_detection_on_video_amd import _lib

    cin, cout, k, s, p = STEM
    return _lib.ConvDesc(1, cin, T, 32, 32, cout, *k, *s, *p, 1, algo, 1)


def _active(T, ot, bk):
    from anomaly_detection_on_video_amd import _lib

    d = _desc(T)
    K = 3 * 5 * 7 * 7
    tiles = (C.c_int32 * ((K + bk - 1) // bk))()
    n = C.c_int32()
    lib = _lib.load()
    assert lib.advhip_conv3d_active_ktiles(C.byref(d), ot, bk, tiles, C.byref(n)) == 0, lib.advhip_last_error().decode()
    m = C.c_int32()
    assert lib.advhip_conv3d_active_ktiles(C.byref(d), ot, bk, None, C.byref(m)) == 0 and m.value == n.value  # count only
    return list(tiles[: n.value])


def test_active_ktile_lists_of_the_stem_at_16_frames():
    """k = ((ci*5 + dt)*7 + dh)*7 + dw, K = 735, 46 k-tiles of 16 rows.  Frame 0 has taps dt = 0, 1 in the padding (rows
    [245 ci, 245 ci + 98)), frame 7 tap dt = 4 (rows [245 ci + 196, 245 ci + 245)); row 735 is the zero row above K."""
    all_tiles = list(range(46))
    skipped0 = list(range(0, 6)) + list(range(16, 21)) + list(range(31, 36))
    skipped7 = [13, 14, 28, 29, 43, 44, 45]
    assert len(skipped0) == 16 and len(skipped7) == 7
    assert _active(16, 0, 16) == [t for t in all_tiles if t not in skipped0]
    assert _active(16, 7, 16) == [t for t in all_tiles if t not in skipped7]
    for ot in range(1, 7):  # no padded tap: the identity list
        assert _active(16, ot, 16) == all_tiles
    assert 16 + 7 == 23  # of 8 * 46 = 368 per sample column


@pytest.mark.parametrize("T", [4, 8, 16])
@pytest.mark.parametrize("bk", [16, 32])
def test_active_ktile_lists_drop_no_valid_row(T, bk):
    """Brute force over every k: a tile is in the list exactly when one of its rows k < K has its temporal tap inside the clip."""
    kt, kh, kw, st, pt, K = 5, 7, 7, 2, 2, 735
    To = (T + 2 * pt - kt) // st + 1
    for ot in range(To):
        valid = [0 <= ot * st - pt + (k // (kh * kw)) % kt < T for k in range(K)]
        want = sorted({k // bk for k in range(K) if valid[k]})
        got = _active(T, ot, bk)
        assert got == want, (T, bk, ot)
        assert got == sorted(set(got)) and all(0 <= t < -(-K // bk) for t in got)
        if all(valid):
            assert got == list(range(-(-K // bk)))


def test_active_ktiles_rejects_a_frame_outside_the_output():
    from anomaly_detection_on_video_amd import _lib

    n = C.c_int32()
    lib = _lib.load()
    assert lib.advhip_conv3d_active_ktiles(C.byref(_desc(16)), 8, 16, None, C.byref(n)) != 0
    assert lib.advhip_conv3d_active_ktiles(C.byref(_desc(16)), -1, 16, None, C.byref(n)) != 0
    assert lib.advhip_conv3d_active_ktiles(C.byref(_desc(16)), 0, 0, None, C.byref(n)) != 0


def test_split_workspace_is_host_arithmetic():
    """One slab per border window more, only where the split applies (an even number of 4-row bricks along h, even output T)."""
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    cin, cout, k, s, p = STEM

    def need(B, T, H, W, algo):
        d = _lib.ConvDesc(B, cin, T, H, W, cout, *k, *s, *p, 1, algo, 1)
        return int(lib.advhip_conv3d_relu_maxpool233_workspace_bytes(C.byref(d)))

    base = need(32, 16, 224, 224, 0)
    assert base == 32 * 4 * 28 * 7 * 64 * 27 * 4
    assert need(32, 16, 224, 224, _lib.ALGO_STEM_BORDER) == base // 4 * 6     # windows 0 and 3
    assert need(3, 8, 32, 32, _lib.ALGO_STEM_BORDER) == need(3, 8, 32, 32, 0) * 2  # both windows
    assert need(2, 4, 32, 32, _lib.ALGO_STEM_BORDER) == need(2, 4, 32, 32, 0) * 2  # one window, both frames padded
    assert need(1, 16, 24, 32, _lib.ALGO_STEM_BORDER) == need(1, 16, 24, 32, 0)    # 3 brick rows
    assert need(1, 10, 32, 32, _lib.ALGO_STEM_BORDER) == need(1, 10, 32, 32, 0)    # To = 5
