"""Plain fp64 references of the scorer's GEMM-shaped kernels, and the makers of the inputs that make fp32 exact.

Written from include/advhip.h's description of each entry point, not from the kernels:

  advhip_conv3d_bn_act_ex_f32 as mgfn_ops.conv_cn drives it (scale = 1): the LayerNorm fold v = acc*rs[m] - u[n]*mu[m]*rs[m], + shift,
      + residual, the second output (the pre-activation, or GELU' of it for code 3), the activation, then x GELU'(dact_z) -- or
      x dact_z as is for code 4
  advhip_bgemm_f32: alpha * A B, the LayerNorm fold, + bias_m + bias_n, the activation, + beta * R
  advhip_gemm_nt_rowsum_f32: A B^T and the row sums of A
  advhip_softmax_rows_f32

Integer-valued operands (`ints`) keep every product and partial sum an integer below 2^24, so an fp32 kernel must return the
reference bit for bit whatever its summation order; operands that are integers / 8 (`eighths`) keep a pre-activation exact, so
that only the evaluation of GELU is left to compare.  `embed` puts an operand into a larger buffer filled with NaN (or a sentinel):
a read outside the operand poisons the result, a store outside the output changes the sentinel.  No GPU here.
"""
import math

import numpy as np
import torch

from anomaly_detection_on_video_amd.weights import hash_uniform

ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_D, ACT_MUL = 0, 1, 2, 3, 4
U24 = 2.0 ** -24  # half an ulp of an fp32 value in [1, 2)


# ---- input makers (seeded like weights.synth_tensor: a pure function of the name) -----------------------------------------------
def ints(name, shape, lo=-3, hi=3):
    """fp32 tensor of integers, uniform over lo..hi"""
    n = int(np.prod(shape)) if len(shape) else 1
    u = (hash_uniform(name, n) + 1.0) * 0.5  # [0, 1)
    v = np.minimum(np.floor(u * (hi - lo + 1)), hi - lo) + lo
    return torch.from_numpy(v.astype(np.float32).reshape(shape))


def eighths(name, shape, lo=-1, hi=1):
    """fp32 tensor of multiples of 1/8 in [lo, hi]: products are multiples of 1/64"""
    return ints(name, shape, 8 * lo, 8 * hi) / 8.0


def embed(t, pad=64, fill=float("nan"), offset=0, pitch=None, device=None):
    """A view equal to `t` inside a larger `fill`-filled 1-D buffer (view._base), `pad` (rounded up to a multiple of 4) + `offset`
    floats from its start -- the buffer itself is at least 16-byte aligned, so offset % 4 = 0 / 2 / 1 puts the view on a 16- / 8- /
    4-byte-aligned base -- with rows (the last dim) `pitch` floats apart (default: dense).  `pad` floats follow the last row."""
    cols = t.shape[-1] if t.dim() else 1
    pitch = cols if pitch is None else pitch
    assert pitch >= cols and t.dim() >= 1
    rows = t.numel() // max(cols, 1)
    start = -(-pad // 4) * 4 + offset
    buf = torch.full((start + rows * pitch + pad,), fill, dtype=t.dtype)
    strides, run = [1], pitch
    for d in reversed(t.shape[:-1]):
        strides.insert(0, run)
        run *= d
    buf.as_strided(t.shape, strides, start).copy_(t)
    if device is not None:
        buf = buf.to(device)
    return buf.as_strided(t.shape, strides, start)


def outside(view):
    """the elements of view._base that are not part of `view`, as a 1-D tensor"""
    buf = view._base
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    return buf[mask]


# ---- activations ---------------------------------------------------------------------------------------------------------------------
def gelu(z):
    z = z.double()
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# ---- the conv entry point as conv_cn drives it -----------------------------------------------------------------------------------------
def conv_acc(x, w, k):
    """sum_c sum_j w[o, c, j] x[c, b, t + j - k//2] with zero padding per sequence: x (Cin, B, T), w (Cout, Cin, k) -> (Cout, B, T) fp64"""
    x, w = x.double(), w.double().reshape(w.shape[0], x.shape[0], k)
    cin, b, t = x.shape
    p = k // 2
    xp = torch.zeros((cin, b, t + 2 * p), dtype=torch.float64)
    xp[:, :, p : p + t] = x
    acc = torch.zeros((w.shape[0], b, t), dtype=torch.float64)
    for j in range(k):
        acc += torch.einsum("oc,cbt->obt", w[:, :, j], xp[:, :, j : j + t])
    return acc


def conv_cn_ref(x, w, k=1, shift=None, residual=None, act=ACT_NONE, dact_z=None, dact_is_multiplier=False, ln=None):
    """-> (y, second): second = the pre-activation z (codes 0, 1, 2, 4) or GELU'(z) (code 3)"""
    v = conv_acc(x, w, k)
    cout = v.shape[0]
    if ln is not None:
        u, mu, rs = (q.double() for q in ln)
        mu, rs = mu.reshape(1, *v.shape[1:]), rs.reshape(1, *v.shape[1:])
        v = v * rs - u.reshape(cout, 1, 1) * mu * rs
    if shift is not None:
        v = v + shift.double().reshape(cout, 1, 1)
    if residual is not None:
        v = v + residual.double()
    second = gelu_grad(v) if act == ACT_GELU_D else v.clone()
    if act == ACT_RELU:
        v = v.clamp_min(0.0)
    elif act in (ACT_GELU, ACT_GELU_D):
        v = gelu(v)
    if dact_z is not None:
        v = v * (dact_z.double() if dact_is_multiplier or act == ACT_MUL else gelu_grad(dact_z))
    return v, second


def conv_dx_ref(dy, w, k):
    """The adjoint of conv_acc in x: dy (Cout, B, T), w (Cout, Cin, k) -> dx (Cin, B, T), dx[c, b, s] = sum_o sum_j w[o, c, j] dy[o, b, s - j + k//2]"""
    dy, w = dy.double(), w.double()
    cout, b, t = dy.shape
    p = k // 2
    dyp = torch.zeros((cout, b, t + 2 * p), dtype=torch.float64)
    dyp[:, :, p : p + t] = dy
    dx = torch.zeros((w.shape[1], b, t), dtype=torch.float64)
    for j in range(k):
        dx += torch.einsum("oc,obt->cbt", w[:, :, j], dyp[:, :, 2 * p - j : 2 * p - j + t])
    return dx


def unfold3_ref(x):
    """(C, B, T) -> (3C, B*T), row c*3 + j = x[c, b, t + j - 1] (zero outside the sequence): the operand of the k = 1 form of a k = 3 conv"""
    c, b, t = x.shape
    xp = torch.nn.functional.pad(x, (1, 1))
    return torch.stack([xp[:, :, j : j + t] for j in range(3)], dim=1).reshape(3 * c, b * t)


# ---- the other entry points ----------------------------------------------------------------------------------------------------------
def gemm_nt_ref(a, b):
    a, b = a.double(), b.double()
    return a @ b.t(), a.sum(dim=1)


def bgemm_ref(a, b, alpha=1.0, bias_m=None, bias_n=None, act=0, residual=None, beta=1.0, ln=None):
    """a (batch | 1, M, K), b (batch | 1, K, N) -> (batch, M, N); ln = (u[M], mu[batch*N], rs[batch*N])"""
    a, b = a.double(), b.double()
    a = a.unsqueeze(0) if a.dim() == 2 else a
    b = b.unsqueeze(0) if b.dim() == 2 else b
    v = alpha * torch.matmul(a, b)
    batch, m, n = v.shape
    if ln is not None:
        u, mu, rs = (q.double() for q in ln)
        mu, rs = mu.reshape(batch, 1, n), rs.reshape(batch, 1, n)
        v = v * rs - u.reshape(1, m, 1) * mu * rs
    if bias_n is not None:
        v = v + bias_n.double().reshape(1, 1, n)
    if bias_m is not None:
        v = v + bias_m.double().reshape(1, m, 1)
    if act == 1:
        v = v.clamp_min(0.0)
    elif act == 2:
        v = gelu(v)
    if residual is not None:
        v = v + beta * residual.double().reshape(batch, m, n)
    return v


def softmax_ref(x, scale=1.0):
    return torch.softmax(x.double() * scale, dim=-1)


# ---- how far an fp32 libm of ordinary quality is from fp64, measured on the host -------------------------------------------------------
def host_units(fn32, fn64, z, unit):
    """worst |fn32(z) - fn64(z)| / unit(z) over the grid z (an fp32 tensor), with torch's own fp32 evaluation on the CPU"""
    z = z.detach().cpu().float().reshape(-1)
    return float(((fn32(z).double() - fn64(z.double())).abs() / unit(z.double())).max())


def gelu32(z):
    return torch.nn.functional.gelu(z)


def gelu_grad32(z):
    z = z.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(torch.nn.functional.gelu(z).sum(), z)
    return g


def gelu_unit(z):
    return U24 * z.abs().clamp_min(1.0)


def grad_unit(z):
    return torch.full_like(z, U24)
