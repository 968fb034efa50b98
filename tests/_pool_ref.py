"""Plain references of the pooling entry points and of the 8x8 head, the comparison rule, and the makers of the inputs.

Written from include/advhip.h's description of each entry point, not from the kernels and not from F.max_pool3d:

  advhip_maxpool3d_f32 / _strided_f32 / _padded_f32: nn.MaxPool3d, floor mode, implicit -inf padding -> maxpool_ref
  advhip_global_avgpool_f32: the mean of each row -> mean_ref (the fp64 row sum, divided, rounded once to fp32)
  the i3d_8x8_r50 head, AdaptiveAvgPool3d(1)(AvgPool3d((4,7,7), 1)(x)) -> head_ref, in fp64

Max pooling selects: every result is one of the inputs, so the kernel must return the reference bit for bit wherever it is not a
zero (`differs`: the same NaN positions, `==` elsewhere; zeros of either sign compare equal -- torch keeps the first zero it meets,
fmaxf need not, and the pooled tensors are post-ReLU).  `quarters` makes rows whose every partial sum in any order is exact in fp32,
so the mean has one correct answer as well.  `embed` / `outside` (tests/_gemm_ref.py) put an operand between NaN or sentinels inside
one allocation.  Every function here runs on whatever device its argument lives on; nothing here needs a GPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from _gemm_ref import embed, ints, outside  # noqa: F401  (the guards are shared with the GEMM and conv edge tests)
from anomaly_detection_on_video_amd.weights import hash_uniform

HEAD_POOL = (4, 7, 7)  # the head's AvgPool3d window (pytorchvideo's create_res_basic_head as i3d_8x8_r50 configures it)


def out_dims(thw, k, s, p=(0, 0, 0)):
    """floor-mode output extents, the torch formula"""
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(thw, k, s, p))


# ---- the operations ------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x, k, s, p=(0, 0, 0)):
    """(B, C, T, H, W) -> (B, C, To, Ho, Wo): -inf padding, then the running maximum over the kt kh kw shifted strided slices.
    torch.maximum returns NaN when either side is NaN: a NaN anywhere in a window gives NaN."""
    b, c, t, h, w = x.shape
    to, ho, wo = out_dims((t, h, w), k, s, p)
    assert min(to, ho, wo) > 0
    xp = torch.full((b, c, t + 2 * p[0], h + 2 * p[1], w + 2 * p[2]), -math.inf, dtype=x.dtype, device=x.device)
    xp[:, :, p[0] : p[0] + t, p[1] : p[1] + h, p[2] : p[2] + w] = x
    out = torch.full((b, c, to, ho, wo), -math.inf, dtype=x.dtype, device=x.device)
    for dt in range(k[0]):
        for dh in range(k[1]):
            for dw in range(k[2]):
                out = torch.maximum(out, xp[:, :, dt : dt + (to - 1) * s[0] + 1 : s[0], dh : dh + (ho - 1) * s[1] + 1 : s[1],
                                            dw : dw + (wo - 1) * s[2] + 1 : s[2]])
    return out


def windows_holding(thw, k, s, p, pos):
    """the output positions (to, ho, wo) whose window holds input position `pos` = (t, h, w), as a set"""
    dims = out_dims(thw, k, s, p)
    per_axis = []
    for x, kk, ss, pp, no in zip(pos, k, s, p, dims):
        per_axis.append([o for o in range(no) if o * ss - pp <= x < o * ss - pp + kk])
    return {(a, b, c) for a in per_axis[0] for b in per_axis[1] for c in per_axis[2]}


def mean_ref(x2d):
    """(rows, n) -> (rows,) fp32: the fp64 row sum, divided by n, rounded once.  Where the sum is an fp32 value this is the correctly
    rounded fp32 quotient (53 >= 2 * 24 + 2 bits: the detour through fp64 cannot round twice)."""
    return (x2d.double().sum(dim=1) / x2d.shape[1]).float()


def mean_ref64(x2d):
    return x2d.double().sum(dim=1) / x2d.shape[1]


def head_ref(x):
    """(B, C, T, H, W) -> (B, C) fp64: the head as torch states it, AvgPool3d((4,7,7), stride 1) then the mean over what is left"""
    return F.avg_pool3d(x.double(), HEAD_POOL, 1).mean((2, 3, 4))


# ---- the launchers' preconditions -------------------------------------------------------------------------------------------------------
def expected_refusal(shape, k, s, p=None, y_batch_stride=0):
    """The text (a regular expression) with which the launcher refuses this call, from include/advhip.h and the launchers' messages, or
    None: it must run.  p = None: the un-padded entry points (y_batch_stride in elements, 0 = dense); else advhip_maxpool3d_padded_f32."""
    b, c, t, h, w = shape
    positive = min(b, c) > 0 and min(k) > 0 and min(s) > 0
    if p is None:
        if not positive or t < k[0] or h < k[1] or w < k[2]:
            return r"maxpool3d: bad shape \(B="
        per_sample = c * math.prod(out_dims((t, h, w), k, s))
        if y_batch_stride != 0 and y_batch_stride < per_sample:
            return rf"maxpool3d: y batch stride {y_batch_stride} < one sample \({per_sample}\)"
        return None
    if (not positive or min(p) < 0 or any(2 * pp > kk for pp, kk in zip(p, k))
            or any(n + 2 * pp < kk for n, pp, kk in zip((t, h, w), p, k))):
        return r"maxpool3d_padded: bad shape \(T=.*padding at most half the window\)"
    return None


def mean_refusal(rows, n):
    return None if rows > 0 and n > 0 else "global_avgpool: bad arguments"


# ---- the comparison rule ---------------------------------------------------------------------------------------------------------------
def differs(got, want):
    """bool tensor: True where `got` is not `want` -- NaN where the other is not, or unequal values (zeros of either sign are equal)"""
    gn, wn = got != got, want != want
    return (gn != wn) | (~wn & ~gn & (got != want))


def describe(got, want, limit=4):
    """'n wrong elements of m: index got / want, ...'"""
    got, want = got.detach().cpu(), want.detach().cpu()
    bad = differs(got, want).reshape(-1).nonzero().reshape(-1)
    first = []
    for i in bad[:limit].tolist():
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        first.append(f"{idx} got {float(got.reshape(-1)[i])!r} want {float(want.reshape(-1)[i])!r}")
    return f"{bad.numel()} wrong elements of {got.numel()}: " + "; ".join(first)


# ---- inputs (a pure function of the name, like weights.synth_tensor) ------------------------------------------------------------------
TIES = (-1.0, -0.0, 0.0, 0.5, 0.5, 2.0)
DENORMAL = 2.0 ** -140  # below the smallest normal fp32 (2^-126)


def values(name, shape, k=None, nan=0.0):
    """fp32 (B, C, T, H, W): 74 % uniform in [-4, 4), 16 % from six values that tie (zeros of both signs among them), 5 % denormals
    of either sign, 1 % +inf, 4 % -inf, `nan` (a fraction) NaN on top; with `k`, the first kt x kh x kw corner of sample 0,
    channel 0 is all -inf (its first window, padded or not, then holds nothing else)."""
    n = int(np.prod(shape))
    u = hash_uniform(name, n)
    kind = (hash_uniform(name + ".kind", n) + 1.0) * 0.5
    pick = (hash_uniform(name + ".pick", n) + 1.0) * 0.5
    v = (u * 4.0).astype(np.float32)
    tie = (kind >= 0.74) & (kind < 0.90)
    v[tie] = np.asarray(TIES, dtype=np.float32)[np.minimum((pick[tie] * len(TIES)).astype(np.int64), len(TIES) - 1)]
    den = (kind >= 0.90) & (kind < 0.95)
    v[den] = (np.sign(u[den]) * np.ceil(pick[den] * 7.0) * DENORMAL).astype(np.float32)
    v[(kind >= 0.95) & (kind < 0.96)] = np.inf
    v[kind >= 0.96] = -np.inf
    if nan:
        v[(hash_uniform(name + ".nan", n) + 1.0) * 0.5 < nan] = np.nan
    t = torch.from_numpy(v.reshape(shape))
    if k is not None:
        t[0, 0, : k[0], : k[1], : k[2]] = -math.inf
    return t


def corner(shape, k, s, p=None):
    """the `k` to hand to `values`: the all -inf window, unless it would be the only window of its (sample, channel)"""
    return k if math.prod(out_dims(shape[2:], k, s, p or (0, 0, 0))) > 1 else None


def background(name, shape):
    """finite fp32 in [-4, 4): what the position sweeps put their one NaN / +1000 into"""
    return torch.from_numpy((hash_uniform(name, int(np.prod(shape))) * 4.0).astype(np.float32).reshape(shape))


def sweep_input(name, thw, value):
    """(T H W, 1, T, H, W): sample i is a random background of its own with `value` at flat position i"""
    n = thw[0] * thw[1] * thw[2]
    x = background(name, (n, 1) + tuple(thw))
    x.reshape(n, n)[torch.arange(n), torch.arange(n)] = value
    return x


def big_values(seed, shape):
    """millions of values cheaply: uniform in [-4, 4), every fourth one rounded to a multiple of 1/2 (ties)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g) * 8.0 - 4.0
    tie = torch.rand(shape, generator=g) < 0.25
    return torch.where(tie, (x * 2.0).round() / 2.0, x)


def quarters(name, shape):
    """integers in [-256, 256] divided by 4: with n 64 4 < 2^24 every partial sum of a row of n, in any order, is exact in fp32"""
    assert shape[-1] * 64 * 4 < 2 ** 24
    return ints(name, shape, -256, 256) / 4.0


def mixed(name, shape):
    """real values of both signs in [-2, 2)"""
    return torch.from_numpy((hash_uniform(name, int(np.prod(shape))) * 2.0).astype(np.float32).reshape(shape))
