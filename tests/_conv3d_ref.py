"""Plain fp64 references of the backbone's conv entry points, the inputs that make fp32 exact, and the launchers' documented refusals.

Written from include/advhip.h's description of each entry point, not from the kernels:

  advhip_conv3d_bn_act_ex_f32 as ops.conv3d_bn_act drives it: y = act(conv3d(x, w) * scale[c] + shift[c] (+ residual)), a 3-D
      cross-correlation with zero padding and floor-mode output extents
  advhip_bn_fold_f32: scale = gamma / sqrt(var + eps), shift = beta - mean * scale
  the pools fused behind it: MaxPool3d (2,3,3) / (2,2,2) and (2,1,1) / (2,1,1), padding 0, floor mode; the mean over a sample's positions

Integer-valued operands (`_gemm_ref.ints`) and a BatchNorm whose fold is a power of two (`exact_bn`) keep every product, partial sum and
epilogue value a multiple of 1/4 below 2^22 (`assert_exact`), so an fp32 kernel must return the reference bit for bit whatever its
summation order, tile or K split.  `expected_refusal` states, from the header and the launchers' messages, which (id, case, split
count, placement) a launcher refuses and with which text.  No GPU here.
"""
import math

import numpy as np
import torch

from _gemm_ref import embed, ints, outside  # noqa: F401  (the makers and the guards are shared with the scorer's GEMM tests)

# (name, Cin, Cout, kernel, stride, padding, (B, T, H, W)): the smallest shapes that still have the property named in
# tests/test_hip_conv3d_edges.py's table
CASES = [
    ("w33.s1", 5, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 2, 7, 9)),
    ("w33.s2", 16, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 11, 10)),
    ("t3", 64, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 4, 5, 13)),
    ("t3.T2", 64, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0), (2, 2, 7, 7)),
    ("t3.T1", 32, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), (3, 1, 9, 5)),
    ("k1.s2", 32, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0), (2, 2, 9, 11)),
    ("k1.98", 64, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (3, 2, 7, 7)),
    ("k1.257", 64, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1, 257)),
    ("k1.260", 64, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 5, 52)),
    ("stem", 3, 64, (5, 7, 7), (2, 2, 2), (2, 3, 3), (2, 5, 11, 13)),
    ("odd333", 7, 64, (3, 3, 3), (1, 2, 1), (1, 0, 2), (1, 3, 5, 7)),
    ("allpad", 16, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 1, 1, 1)),
    ("k333.small", 16, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 2, 2, 3)),
]
CASE = {c[0]: c for c in CASES}
EXACT_LIMIT = 2.0 ** 24 * 0.25  # 2^24 steps of 1/4, the smallest step exact_bn's scales leave


def out_dims(thw, k, s, p):
    """floor-mode output extents, the torch formula (advhip_conv3d_out_dims, ops.conv_out_dims)"""
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(thw, k, s, p))


# ---- the operations ------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, stride, padding):
    """y[b, o, t, h, w] = sum_{c, dt, dh, dw} w[o, c, dt, dh, dw] x[b, c, t st + dt - pt, h sh + dh - ph, w sw + dw - pw], x zero outside
    its extents: (B, Cin, T, H, W), (Cout, Cin, kt, kh, kw) -> (B, Cout, To, Ho, Wo) fp64"""
    x, w = x.double(), w.double()
    b, cin, t, h, wd = x.shape
    cout, cin_w, kt, kh, kw = w.shape
    assert cin == cin_w
    (st, sh, sw), (pt, ph, pw) = stride, padding
    to, ho, wo = out_dims((t, h, wd), (kt, kh, kw), stride, padding)
    assert min(to, ho, wo) > 0
    xp = torch.zeros((b, cin, t + 2 * pt, h + 2 * ph, wd + 2 * pw), dtype=torch.float64)
    xp[:, :, pt : pt + t, ph : ph + h, pw : pw + wd] = x
    y = torch.zeros((b, cout, to, ho, wo), dtype=torch.float64)
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                win = xp[:, :, dt : dt + (to - 1) * st + 1 : st, dh : dh + (ho - 1) * sh + 1 : sh, dw : dw + (wo - 1) * sw + 1 : sw]
                y += torch.einsum("oc,bcthw->bothw", w[:, :, dt, dh, dw], win)
    return y


def bn_act_ref(acc, scale, shift, residual=None, relu=True):
    """act(acc * scale[c] + shift[c] (+ residual)) of an fp64 conv result"""
    v = acc * scale.double().reshape(1, -1, 1, 1, 1) + shift.double().reshape(1, -1, 1, 1, 1)
    if residual is not None:
        v = v + residual.double()
    return v.clamp_min(0.0) if relu else v


def conv_bn_act_ref(x, w, scale, shift, stride, padding, residual=None, relu=True):
    return bn_act_ref(conv_ref(x, w, stride, padding), scale, shift, residual, relu)


def maxpool_ref(y, kernel, stride):
    """MaxPool3d, padding 0, floor mode"""
    to, ho, wo = out_dims(y.shape[2:], kernel, stride, (0, 0, 0))
    assert min(to, ho, wo) > 0
    (st, sh, sw) = stride
    out = torch.full(tuple(y.shape[:2]) + (to, ho, wo), -math.inf, dtype=y.dtype)
    for dt in range(kernel[0]):
        for dh in range(kernel[1]):
            for dw in range(kernel[2]):
                out = torch.maximum(out, y[:, :, dt : dt + (to - 1) * st + 1 : st, dh : dh + (ho - 1) * sh + 1 : sh, dw : dw + (wo - 1) * sw + 1 : sw])
    return out


def maxpool233_ref(y):
    return maxpool_ref(y, (2, 3, 3), (2, 2, 2))


def maxpool211_ref(y):
    return maxpool_ref(y, (2, 1, 1), (2, 1, 1))


def mean_ref(y):
    """the mean over each sample's positions: (B, C, T, H, W) -> (B, C, 1, 1, 1)"""
    n = y.shape[2] * y.shape[3] * y.shape[4]
    return y.double().sum(dim=(2, 3, 4), keepdim=True) / n


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def exact_bn(name, cout):
    """-> (gamma, beta, mean, var), (scale, shift): an eval-mode BatchNorm whose fold (eps = 0.0) is exact in fp32 -- var in {0.25, 1, 4},
    gamma in {+-0.5, +-1, +-2}, integer mean in [-2, 2] and beta in [-8, 8] -- and the scale (+-0.25 ... +-4) and shift it must fold to"""
    var = 4.0 ** ints(name + ".var", (cout,), -1, 1)
    gamma = (2.0 * ints(name + ".sgn", (cout,), 0, 1) - 1.0) * 2.0 ** ints(name + ".gam", (cout,), -1, 1)
    mean, beta = ints(name + ".mean", (cout,), -2, 2), ints(name + ".beta", (cout,), -8, 8)
    scale = gamma.double() / var.double().sqrt()
    shift = beta.double() - mean.double() * scale
    assert torch.equal(scale.float().double(), scale) and torch.equal(shift.float().double(), shift)
    assert bool((gamma < 0).any()) and bool((gamma > 0).any()) and float(scale.abs().min()) >= 0.25 and float(scale.abs().max()) <= 4.0
    return (gamma, beta, mean, var), (scale.float(), shift.float())


def operands(case, tag=""):
    """x, w and the residual of a case as integers in -3..3"""
    name, cin, cout, k, s, p, (b, t, h, w) = case
    to, ho, wo = out_dims((t, h, w), k, s, p)
    return (ints(f"c3d.{tag}{name}.x", (b, cin, t, h, w)), ints(f"c3d.{tag}{name}.w", (cout, cin) + tuple(k)),
            ints(f"c3d.{tag}{name}.r", (b, cout, to, ho, wo)))


def probe_x(shape):
    """x[b, ci, t, h, w] = its own flat index + 1"""
    n = int(np.prod(shape))
    assert n + 1 < 2 ** 24
    return torch.arange(1, n + 1, dtype=torch.float32).reshape(shape)


def probe_tap(c, s, cout, K):
    """the flattened tap ((ci * kt + dt) * kh + dh) * kw + dw that output channel c of weight set s carries its single 1 at"""
    return ((s * cout + c) * 11) % K


def probe_weights(cout, cin, k, s):
    K = cin * k[0] * k[1] * k[2]
    w = torch.zeros((cout, K), dtype=torch.float32)
    w[torch.arange(cout), torch.tensor([probe_tap(c, s, cout, K) for c in range(cout)])] = 1.0
    return w.reshape((cout, cin) + tuple(k))


def probe_sets(cout, cin, k, limit=8):
    """how many weight sets it takes until every tap has been probed, `limit` at the most"""
    K = cin * k[0] * k[1] * k[2]
    seen, s = set(), 0
    while len(seen) < K and s < limit:
        seen |= {probe_tap(c, s, cout, K) for c in range(cout)}
        s += 1
    return s


def hi_image_pair(name, shape):
    """256 a + b with a, b in -3..3: 16 significant bits at the most, so a bf16 hi / lo pair (round to nearest) holds it exactly"""
    return 256.0 * ints(name + ".a", shape) + ints(name + ".b", shape)


def assert_exact(x, w, scale, shift, residual, stride, padding):
    """conv(|x|, |w|) max|scale| + max|shift| + max|residual| < 2^24 steps of 1/4, for operands that are integers and scales / shifts that
    are multiples of 1/4: every value an fp32 kernel can form on the way is exactly representable -> the bound's left side"""
    for v in (x, w) + (() if residual is None else (residual,)):
        assert torch.equal(v, v.round()), "not integers"
    for v in (scale, shift):
        assert torch.equal(v * 4.0, (v * 4.0).round()), "not multiples of 1/4"
    top = float(conv_ref(x.abs(), w.abs(), stride, padding).max()) * float(scale.abs().max()) + float(shift.abs().max())
    if residual is not None:
        top += float(residual.abs().max())
    assert top < EXACT_LIMIT, f"{top} is not below {EXACT_LIMIT}: fp32 would round"
    return top


# ---- the launchers' preconditions -------------------------------------------------------------------------------------------------------
def algos():
    """{id: (family, BM, BN, BK)} of every id advhip_conv3d_algo_info accepts; a T-fold id's family is 'tfold' here (the query reports the
    2-deep-ring kernel its folded launch runs)"""
    from anomaly_detection_on_video_amd import _lib
    from test_conv_algo_table import _accepted

    return {a: ((("tfold",) + tuple(info[1:])) if _lib.is_tfold(a) else tuple(info)) for a, info in sorted(_accepted().items())}


def _launch_geometry(fam, case):
    """(Cout, K, positions per sample) of the launch: the conv's own, or the folded 1x1x1 conv's (B, Cin*T, 1, H, W) -> Cout*T of a T-fold id"""
    name, cin, cout, k, s, p, (b, t, h, w) = case
    to, ho, wo = out_dims((t, h, w), k, s, p)
    if fam == "tfold":
        return cout * t, cin * t, h * w
    return cout, cin * k[0] * k[1] * k[2], to * ho * wo


def k_tiles(algo_info, case):
    fam, bm, bn, bk = algo_info
    kpad = -(-_launch_geometry(fam, case)[1] // 32) * 32
    return -(-kpad // bk)


def max_splits(algo_info, case):
    """the largest split count the id accepts on the case: one K slice per k-tile, 64 at the most; TSPAN, MIXED and PERSIST run unsplit"""
    return 1 if algo_info[0] in ("tspan", "mixed", "persist") else min(k_tiles(algo_info, case), 64)


def expected_refusal(algo_info, case, form, splits, x_aligned16):
    """The text (a regular expression) of the precondition of include/advhip.h / the launchers' messages that this launch does not
    meet, in the order the launchers state them, or None: it must run.  `form`: (residual, relu, in place) -- none of them is one of the
    MGFN epilogue operands, so no precondition depends on it.  `x_aligned16`: x on a 16-byte aligned base, its batch stride a multiple
    of 4 floats."""
    fam, bm, bn, bk = algo_info
    name, cin, cout, k, s, p, (b, t, h, w) = case
    to, ho, wo = out_dims((t, h, w), k, s, p)
    one, unit, nopad = tuple(k) == (1, 1, 1), tuple(s) == (1, 1, 1), tuple(p) == (0, 0, 0)
    if fam == "tfold":
        if k[1:] != (1, 1) or p[1:] != (0, 0):
            return r"ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs a \(kt,1,1\) conv without spatial padding"
        if not unit:
            return "ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs stride 1"
        if 2 * p[0] + 1 != k[0]:
            return "ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs the centred padding pt = kt/2 of an odd kt"
        if t > p[0] + 1:
            return r"ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs T <= pt \+ 1 frames"
        one = True  # from here on the launch is the folded one: a dense 1x1x1 stride-1 conv
    if fam not in ("generic",) and max(k) > 10:
        return "fast kernel needs kernel extents <= 10"
    n, K, positions = _launch_geometry(fam, case)
    if n % bn:
        return f"Cout={n} not a multiple of the {bn}-wide N tile"
    if splits > k_tiles(algo_info, case) or splits > 64 or splits < 1:
        return f"bad split count {splits}"
    if fam == "tspan":
        if k[1:] != (1, 1) or not unit or p[1:] != (0, 0) or 2 * p[0] + 1 != k[0]:
            return r"ADVHIP_ALGO_TSPAN needs a \(kt,1,1\) stride-1 conv with padding kt/2"
        if splits != 1 or to % 2:
            return "ADVHIP_ALGO_TSPAN runs unsplit on an even number of frames"
    # rows of 4 positions as 16-byte pieces: an unmasked (1x1x1, no padding, K a multiple of 32) stride-1 conv on 16-byte aligned rows
    # of a multiple of 4 positions -- or of any length, which the families built on the 2-deep ring pad in the index space
    unmasked = one and unit and nopad and K % 32 == 0
    a16 = unmasked and x_aligned16
    if fam == "mixed" and not (a16 and splits == 1):
        return "ADVHIP_ALGO_MIXED_128x64 takes unsplit 1x1x1 stride-1 convs on 16-byte aligned rows"
    if fam == "persist":
        if -(-K // 32) * 32 < 64:
            return "the persistent kernels need K >= 64"
        if not (a16 and splits == 1):
            return r"the persistent kernels \(algo \d+\) take unsplit 1x1x1 stride-1 convs on 16-byte aligned rows"
    return None
