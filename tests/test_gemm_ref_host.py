"""Host tests of tests/_gemm_ref.py: the references the scorer GEMM kernels are compared with, against torch's own fp64 operators and
autograd, and the input makers' promises (integers, eighths, alignment and pitch of embedded views)."""
import pytest
import torch

import _gemm_ref as R


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("b,t", [(1, 1), (3, 1), (2, 2), (5, 3), (3, 33)])
def test_conv_cn_ref_matches_conv1d_gelu_and_autograd(k, b, t):
    cin, cout = 6, 5
    x = R.eighths(f"rh.x{k}{b}{t}", (cin, b, t), -2, 2).double()
    w = R.eighths(f"rh.w{k}{b}{t}", (cout, cin, k)).double()
    shift = R.eighths(f"rh.s{k}{b}{t}", (cout,)).double()
    res = R.eighths(f"rh.r{k}{b}{t}", (cout, b, t)).double()
    xt = x.permute(1, 0, 2).clone().requires_grad_(True)  # (B, Cin, T): torch's layout
    z = torch.nn.functional.conv1d(xt, w, shift, padding=k // 2)
    zc = z.permute(1, 0, 2)
    y, second = R.conv_cn_ref(x, w, k, shift=shift)
    assert torch.allclose(y, zc.detach(), rtol=0, atol=1e-12) and torch.equal(second, y)
    y, second = R.conv_cn_ref(x, w, k, shift=shift, residual=res)
    assert torch.allclose(y, zc.detach() + res, rtol=0, atol=1e-12)
    y, _ = R.conv_cn_ref(x, w, k, shift=shift, act=R.ACT_RELU)
    assert torch.allclose(y, zc.detach().clamp_min(0), rtol=0, atol=1e-12)
    # GELU, its derivative (autograd of torch's GELU in fp64), and the two backward forms
    zl = z.detach().clone().requires_grad_(True)
    h = torch.nn.functional.gelu(zl)
    (g,) = torch.autograd.grad(h.sum(), zl)
    y2, s2 = R.conv_cn_ref(x, w, k, shift=shift, act=R.ACT_GELU)
    y3, s3 = R.conv_cn_ref(x, w, k, shift=shift, act=R.ACT_GELU_D)
    assert torch.allclose(y2, h.detach().permute(1, 0, 2), rtol=0, atol=1e-12) and torch.allclose(s2, zc.detach(), rtol=0, atol=1e-12)
    assert torch.equal(y3, y2) and torch.allclose(s3, g.permute(1, 0, 2), rtol=0, atol=1e-12)
    yd, _ = R.conv_cn_ref(x, w, k, dact_z=res)
    ym, _ = R.conv_cn_ref(x, w, k, dact_z=R.gelu_grad(res), act=R.ACT_MUL)
    assert torch.allclose(yd, R.conv_acc(x, w, k) * R.gelu_grad(res), rtol=0, atol=1e-12) and torch.equal(yd, ym)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("b,t", [(1, 1), (2, 2), (5, 3), (2, 32)])
def test_conv_dx_ref_is_autograds_input_gradient_and_the_exact_adjoint(k, b, t):
    cin, cout = 7, 4
    x = R.ints(f"rd.x{k}{b}{t}", (cin, b, t))
    w = R.ints(f"rd.w{k}{b}{t}", (cout, cin, k))
    dy = R.ints(f"rd.g{k}{b}{t}", (cout, b, t))
    xt = x.double().permute(1, 0, 2).clone().requires_grad_(True)
    z = torch.nn.functional.conv1d(xt, w.double(), None, padding=k // 2)
    (gx,) = torch.autograd.grad(z, xt, dy.double().permute(1, 0, 2))
    dx = R.conv_dx_ref(dy, w, k)
    assert torch.equal(dx, gx.permute(1, 0, 2))
    # <conv(x), dy> == <x, dx> as integers
    y = R.conv_acc(x, w, k)
    assert torch.equal(y, y.round()) and torch.equal(dx, dx.round())
    assert int((y.long() * dy.long()).sum()) == int((x.long() * dx.long()).sum())
    # the k = 1 form of the k = 3 conv: the unfolded rows against the tap-minor weight matrix
    if k == 3:
        assert torch.equal(R.conv_acc(R.unfold3_ref(x).reshape(3 * cin, b, t), w.reshape(cout, 3 * cin, 1), 1), y)


def test_ln_fold_is_the_layernorm_applied_before_the_weight():
    # MGFNLayerNorm: (x - mean_c) / (sqrt(var_biased_c) + eps) * g + b per position; the fold runs W.diag(g) on the raw activation
    cin, cout, b, t, eps = 12, 5, 3, 4, 1e-5
    x = R.eighths("rl.x", (cin, b, t), -3, 3).double()
    w = R.eighths("rl.w", (cout, cin, 1)).double()
    g, be, bias = R.eighths("rl.g", (cin,)).double() + 1.5, R.eighths("rl.b", (cin,)).double(), R.eighths("rl.c", (cout,)).double()
    mu = x.mean(dim=0)
    rs = 1.0 / (x.var(dim=0, unbiased=False).sqrt() + eps)
    xh = (x - mu) * rs * g.reshape(cin, 1, 1) + be.reshape(cin, 1, 1)
    want = torch.einsum("oc,cbt->obt", w[:, :, 0], xh) + bias.reshape(cout, 1, 1)
    wg = w * g.reshape(1, cin, 1)
    got, _ = R.conv_cn_ref(x, wg, 1, shift=w[:, :, 0] @ be + bias, ln=(wg[:, :, 0].sum(dim=1), mu.reshape(-1), rs.reshape(-1)))
    assert torch.allclose(got, want, rtol=0, atol=1e-10)
    # and bgemm's form of the same fold: columns are (batch, n)
    a = wg[:, :, 0].unsqueeze(0).expand(b, cout, cin)
    got_b = R.bgemm_ref(a, x.permute(1, 0, 2), bias_m=w[:, :, 0] @ be + bias, ln=(wg[:, :, 0].sum(dim=1), mu.reshape(-1), rs.reshape(-1)))
    assert torch.allclose(got_b, want.permute(1, 0, 2), rtol=0, atol=1e-10)


def test_bgemm_ref_epilogue_order_and_gemm_nt_and_softmax():
    a, b = R.ints("rb.a", (3, 5, 7)), R.ints("rb.b", (1, 7, 4))
    bm, bn, res = R.ints("rb.m", (5,)), R.ints("rb.n", (4,)), R.ints("rb.r", (3, 5, 4))
    v = 0.5 * torch.matmul(a.double(), b.double()) + bm.double().reshape(1, 5, 1) + bn.double().reshape(1, 1, 4)
    assert torch.equal(R.bgemm_ref(a, b, alpha=0.5, bias_m=bm, bias_n=bn, act=1, residual=res, beta=-2.0), v.clamp_min(0) - 2.0 * res.double())
    assert torch.allclose(R.bgemm_ref(a, b, alpha=0.5, bias_m=bm, bias_n=bn, act=2), torch.nn.functional.gelu(v), rtol=0, atol=1e-12)
    p, rs = R.gemm_nt_ref(a[0], R.ints("rb.c", (6, 7)))
    assert torch.equal(p, a[0].double() @ R.ints("rb.c", (6, 7)).double().t()) and torch.equal(rs, a[0].double().sum(1))
    x = R.eighths("rb.s", (3, 9), -4, 4)
    assert torch.allclose(R.softmax_ref(x, 0.5).sum(-1), torch.ones(3, dtype=torch.float64), rtol=0, atol=1e-14)


def test_makers_keep_their_promises():
    v = R.ints("rm.i", (4000,))
    assert v.dtype == torch.float32 and torch.equal(v, v.round()) and float(v.min()) == -3 and float(v.max()) == 3
    assert float((v != 0).float().mean()) > 0.8 and torch.equal(v, R.ints("rm.i", (4000,))) and not torch.equal(v, R.ints("rm.j", (4000,)))
    e = R.eighths("rm.e", (4000,))
    assert torch.equal(e * 8, (e * 8).round()) and float(e.min()) == -1 and float(e.max()) == 1
    # the exactness the GPU tests rely on: an fp32 product of such matrices equals the fp64 product, whatever the order
    a, b = R.ints("rm.a", (70, 1536)), R.ints("rm.b", (65, 1536))
    assert torch.equal((a @ b.t()).double(), a.double() @ b.double().t()) and float((a @ b.t()).abs().max()) < 2 ** 24
    t = R.ints("rm.t", (3, 5, 6))
    for offset, align in ((0, 16), (1, 4), (2, 8), (3, 4)):
        for pitch in (None, 7, 39):
            for fill in (float("nan"), -777.0):
                view = R.embed(t, pad=6, fill=fill, offset=offset, pitch=pitch)
                assert torch.equal(view, t) and view.shape == t.shape
                assert view.stride(-1) == 1 and view.stride(-2) == (pitch or 6) and view.stride(0) == 5 * (pitch or 6)
                assert view.data_ptr() % 16 == (4 * offset) % 16 and view.data_ptr() % align == 0
                assert (pitch is None) == view.is_contiguous()
                out = R.outside(view)
                assert out.numel() == view._base.numel() - t.numel()
                assert bool(torch.isnan(out).all() if fill != fill else (out == fill).all())
                assert out.numel() >= 2 * 6  # poison on both sides


def _desc_before(cin, cout, k, b, t, act):
    """mgfn_ops._desc as it stood before conv_cn took `algo` / `splits`: the tile and the K slices from the position count"""
    from anomaly_detection_on_video_amd import mgfn_ops

    n = b * t
    algo, splits = mgfn_ops.ALGO, 1
    if cout % 128 == 0 and -(-n // 128) * (cout // 128) >= 1536:
        algo = mgfn_ops.ALGO_WIDE
    elif -(-n // 128) * (cout // 64) < 768:
        algo = mgfn_ops.ALGO_SMALL
        tiles, ktiles = -(-n // 64) * (cout // 64), -(-(cin * k) // 16)
        target, cap = (1152, 12) if ktiles >= 512 else (768, 8)
        while tiles * splits < target and splits < cap and ktiles // (splits + 1) >= 16:
            splits += 1
    return (1, cin, 1, b, t, cout, 1, 1, k, 1, 1, 1, 0, 0, k // 2, act, algo, splits)


def test_conv_cn_without_overrides_builds_the_descriptor_it_always_built():
    from anomaly_detection_on_video_amd import mgfn_ops

    fields = [n for n, _ in mgfn_ops.ConvDesc._fields_]
    seen = set()
    # the shapes of test_hip_mgfn.py's conv_cn calls, the workload's (10 240 positions) and the token conv's weight-gradient shape
    for cin, cout, b, t in [(64, 1024, 768, 32), (64, 64, 20, 32), (128, 512, 10, 57), (64, 128, 320, 32), (1024, 4096, 320, 32), (4096, 1024, 320, 32),
                            (10240, 192, 1, 33), (2048, 64, 10, 32)]:
        for k in (1, 3):
            for act in (0, 2, 3, 4):
                bb, tt = (1, b * t) if k == 1 else (b, t)
                d = mgfn_ops._desc(cin, cout, k, bb, tt, act)
                got = tuple(getattr(d, f) for f in fields)
                assert got == _desc_before(cin, cout, k, bb, tt, act), (cin, cout, k, b, t, act)
                seen.add(got[-2:])
                pinned = mgfn_ops._desc(cin, cout, k, bb, tt, act, algo=161)
                assert tuple(getattr(pinned, f) for f in fields) == got[:-2] + (161, 1)  # a pinned tile runs unsplit ...
                pinned = mgfn_ops._desc(cin, cout, k, bb, tt, act, algo=0, splits=3)
                assert tuple(getattr(pinned, f) for f in fields) == got[:-2] + (0, 3)  # ... unless the slices are pinned too
                pinned = mgfn_ops._desc(cin, cout, k, bb, tt, act, splits=2)
                assert tuple(getattr(pinned, f) for f in fields) == got[:-2] + (got[-2], 2)
    assert {a for a, _s in seen} == {mgfn_ops.ALGO, mgfn_ops.ALGO_SMALL, mgfn_ops.ALGO_WIDE} and len({s for _a, s in seen}) >= 3
