"""CPU-only checks of the temporal fold (include/advhip.h: ADVHIP_ALGO_TFOLD_BASE): the applicability rule and the shape
arithmetic of advhip_conv3d_tfold_desc (host code of the library, no GPU), and the identity itself stated in pure torch
against F.conv3d."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

# (Cin, Cout, H, W): the six (3,1,1) convs of the I3D plan that run on T = 2 frames (layers 2-4; two of layer 3 share a shape)
PLAN_SHAPES = [(256, 128, 55, 55), (512, 128, 28, 28), (512, 256, 28, 28), (1024, 256, 14, 14), (1024, 256, 14, 14), (2048, 512, 7, 7)]


def _desc(B, cin, T, H, W, cout, k=(3, 1, 1), s=(1, 1, 1), p=(1, 0, 0), algo=0, splits=1):
    from anomaly_detection_on_video_amd import _lib

    return _lib.ConvDesc(B, cin, T, H, W, cout, *k, *s, *p, 1, algo, splits)


def _fold(d):
    from anomaly_detection_on_video_amd import _lib

    lib = _lib.load()
    f = _lib.ConvDesc()
    rc = lib.advhip_conv3d_tfold_desc(C.byref(d), C.byref(f))
    return rc, f, lib.advhip_last_error().decode()


@pytest.mark.parametrize("cin,cout,H,W", PLAN_SHAPES)
def test_tfold_desc_accepts_the_plan_shapes(cin, cout, H, W):
    from anomaly_detection_on_video_amd import _lib

    for tile in (1, 2, 3, 4, 6, 7, 8, 9):
        d = _desc(32, cin, 2, H, W, cout, algo=_lib.ALGO_TFOLD_BASE + tile, splits=3)
        rc, f, msg = _fold(d)
        assert rc == 0, msg
        assert (f.B, f.Cin, f.T, f.H, f.W, f.Cout) == (32, 2 * cin, 1, H, W, 2 * cout)
        assert (f.kt, f.kh, f.kw, f.st, f.sh, f.sw, f.pt, f.ph, f.pw) == (1, 1, 1, 1, 1, 1, 0, 0, 0)
        assert (f.relu, f.algo, f.splits) == (1, _lib.ALGO_DMA2_BASE + tile, 3)
        assert _lib.algo_tile(d.algo) == _lib.algo_tile(f.algo)
        lib = _lib.load()
        assert lib.advhip_conv3d_packed_rows(C.byref(f)) == 2 * cin  # 4 rows of the folded matrix per 6 of the plain one
        assert lib.advhip_conv3d_packed_rows(C.byref(d)) == 3 * cin
        # the workspace query takes the id (host arithmetic only) and is the folded launch's
        assert lib.advhip_conv3d_workspace_bytes(C.byref(d)) == lib.advhip_conv3d_workspace_bytes(C.byref(f)) > 0
    # any other algo value is copied: sizing the operands needs no tile
    rc, f, msg = _fold(_desc(8, cin, 2, H, W, cout, algo=0))
    assert rc == 0 and f.algo == 0, msg


def test_tfold_desc_other_kernel_lengths():
    rc, f, msg = _fold(_desc(2, 48, 3, 5, 6, 128, k=(5, 1, 1), p=(2, 0, 0)))
    assert rc == 0 and (f.Cin, f.Cout, f.T, f.kt, f.pt) == (144, 384, 1, 1, 0), msg
    rc, f, msg = _fold(_desc(2, 64, 1, 5, 6, 64))  # T = 1: only the centre tap is ever inside
    assert rc == 0 and (f.Cin, f.Cout) == (64, 64), msg


@pytest.mark.parametrize("kwargs,word", [
    (dict(T=4), "T <= pt + 1"),                                    # layer 1: four frames, three taps -- a fold would cost 16 MACs for 12
    (dict(k=(3, 3, 3), p=(1, 1, 1)), "(kt,1,1)"),                  # a spatial window
    (dict(k=(3, 1, 3), p=(1, 0, 0)), "(kt,1,1)"),
    (dict(s=(1, 2, 2)), "stride 1"),
    (dict(s=(2, 1, 1)), "stride 1"),
    (dict(p=(0, 0, 0), T=3), "centred padding"),                   # missing / over-wide temporal padding: not one tap per frame pair
    (dict(p=(2, 0, 0)), "centred padding"),
    (dict(k=(5, 1, 1), p=(1, 0, 0), T=3), "centred padding"),
    (dict(p=(1, 0, 1)), "spatial padding"),
])
def test_tfold_desc_rejections_name_the_rule(kwargs, word):
    from anomaly_detection_on_video_amd import _lib

    T = kwargs.pop("T", 2)
    d = _desc(2, 64, T, 8, 8, 64, algo=_lib.ALGO_TFOLD_BASE + 3, **kwargs)
    rc, _, msg = _fold(d)
    assert rc == -1 and "TFOLD" in msg and word in msg, msg
    # the launcher's host-side query refuses the id the same way
    assert _lib.load().advhip_conv3d_workspace_bytes(C.byref(d)) == -1
    assert "TFOLD" in _lib.load().advhip_last_error().decode()


def test_tfold_tile_ids():
    from anomaly_detection_on_video_amd import _lib

    for tile in (0, 5, 10, 15):
        rc, _, msg = _fold(_desc(2, 64, 2, 8, 8, 64, algo=_lib.ALGO_TFOLD_BASE + tile))
        assert rc == -1 and "TFOLD" in msg and "not instantiated" in msg, msg
    assert _lib.TFOLD_ALGOS == tuple(range(209, 213)) + tuple(range(214, 218))
    assert all(_lib.is_tfold(a) for a in _lib.TFOLD_ALGOS) and not _lib.is_tfold(207) and not _lib.is_tfold(224)


def _fold_torch(x, w, scale, shift, residual, relu, pt):
    """The fold in torch: the conv as ONE matrix product over (ci, ti) per position, on the same memory seen as
    (B, Cin*T, H*W) -> (B, Cout*T, H*W); W'[n*T + t][ci*T + ti] = W[n][ci][ti - t + pt]."""
    B, cin, T, H, W_ = x.shape
    cout, _, kt = w.shape[:3]
    wf = torch.zeros((cout, T, cin, T), dtype=x.dtype)
    for t in range(T):
        for ti in range(T):
            wf[:, t, :, ti] = w[:, :, ti - t + pt, 0, 0]
    y = torch.matmul(wf.reshape(cout * T, cin * T), x.reshape(B, cin * T, H * W_))
    y = y * scale.repeat_interleave(T)[None, :, None] + shift.repeat_interleave(T)[None, :, None]
    y = y.reshape(B, cout, T, H, W_)
    if residual is not None:
        y = y + residual
    return y.clamp_min(0) if relu else y


@pytest.mark.parametrize("T,kt", [(2, 3), (3, 5), (1, 3)])
def test_fold_identity_equals_conv3d_in_float64(T, kt):
    """Exact equality needs sums that do not depend on their order: operands that are small integers times powers of two,
    so that every product and every partial sum is exact in float64 (the fold only drops terms that are exact zeros and
    regroups the others).  On normally distributed operands the two differ by rounding of the order of summation only."""
    g = torch.Generator().manual_seed(100 * T + kt)
    B, cin, cout, H, W_ = 2, 24, 16, 5, 6
    pt = kt // 2

    def ints(shape, lo=-8, hi=9, unit=1.0):
        return torch.randint(lo, hi, shape, generator=g).double() * unit

    x, w = ints((B, cin, T, H, W_), unit=0.25), ints((cout, cin, kt, 1, 1), unit=0.125)
    scale, shift = ints((cout,), 1, 5, 0.5), ints((cout,), unit=0.5)
    res = ints((B, cout, T, H, W_))
    for residual, relu in ((None, False), (res, True), (res, False), (None, True)):
        ref = F.conv3d(x, w, None, stride=1, padding=(pt, 0, 0)) * scale[None, :, None, None, None] + shift[None, :, None, None, None]
        if residual is not None:
            ref = ref + residual
        if relu:
            ref = ref.clamp_min(0)
        got = _fold_torch(x, w, scale, shift, residual, relu, pt)
        assert got.shape == ref.shape and torch.equal(got, ref), float((got - ref).abs().max())
    xr, wr = torch.randn((B, cin, T, H, W_), generator=g, dtype=torch.float64), torch.randn((cout, cin, kt, 1, 1), generator=g, dtype=torch.float64)
    ref = F.conv3d(xr, wr, None, stride=1, padding=(pt, 0, 0))
    got = _fold_torch(xr, wr, torch.ones(cout, dtype=torch.float64), torch.zeros(cout, dtype=torch.float64), None, False, pt)
    assert float((got - ref).abs().max()) < 1e-12 * float(ref.abs().max()) * cin * kt
