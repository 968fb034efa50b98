"""Thin Python wrappers over the C ABI (include/advhip.h): shape checks, output allocation
(torch is used only for device memory and streams) and the launch on torch's current stream.

Every function here REQUIRES CUDA tensors and the built HIP extension; none has a fallback.
"""
from __future__ import annotations

import os

import ctypes as C
import hashlib
import math
import numbers
import struct
from dataclasses import dataclass, field
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, check, ptr, require_gpu, stream


def _triple(v) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(i) for i in v)
    assert len(v) == 3
    return v


def conv_out_dims(in_thw: Sequence[int], k: Sequence[int], s: Sequence[int], p: Sequence[int]) -> Tuple[int, int, int]:
    return tuple((n + 2 * pp - kk) // ss + 1 for n, kk, ss, pp in zip(in_thw, k, s, p))  # type: ignore


@dataclass
class PackedConv:
    """Load-time state of one conv+BN unit: packed weights, folded BN, gather tables per input size."""

    cout: int
    cin: int
    kernel: Tuple[int, int, int]
    stride: Tuple[int, int, int]
    padding: Tuple[int, int, int]
    w_packed: torch.Tensor  # [Kpad, Cout]
    scale: torch.Tensor
    shift: torch.Tensor
    ktabs: Dict[Tuple[int, int, int], torch.Tensor] = field(default_factory=dict)
    ktabs_s2w: Dict[Tuple[int, int, int], torch.Tensor] = field(default_factory=dict)  # column-parity gather tables (stem)
    algo: int = _lib.ALGO_AUTO
    name: str = ""
    splits: int = 0  # 0 = library heuristic
    weight: Optional[torch.Tensor] = None   # the torch-layout fp32 weights (a reference, not a copy)
    w_split: Optional[torch.Tensor] = None  # bf16 hi/lo images for the opt-in split-bf16 kernels, packed on first use
    # operands of the temporal fold (ADVHIP_ALGO_TFOLD_BASE), built on first use: T -> (w_folded [Kpad', Cout*T], scale, shift of
    # Cout*T entries); (T,H,W) -> the folded 1x1x1 conv's gather table
    tfold_w: Dict[int, Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = field(default_factory=dict)
    tfold_ktabs: Dict[Tuple[int, int, int], torch.Tensor] = field(default_factory=dict)
    # (B,T,H,W) -> (algo, splits) resolved from the measured table (tuned.py)
    choices: Dict[Tuple[int, int, int, int], Tuple[int, int]] = field(default_factory=dict)

    def key(self, B: int, T: int, H: int, W: int) -> str:
        return ",".join(str(v) for v in (self.cin, self.cout, *self.kernel, *self.stride, *self.padding, B, T, H, W))

    def desc(self, B: int, T: int, H: int, W: int, relu: bool, algo: Optional[int] = None,
             splits: Optional[int] = None) -> ConvDesc:
        kt, kh, kw = self.kernel
        st, sh, sw = self.stride
        pt, ph, pw = self.padding
        if algo is None and splits is None:
            ch = self.choices.get((B, T, H, W))
            if ch is None:
                from . import tuned

                ch = tuned.lookup(self.key(B, T, H, W), (self.algo, self.splits))
                if ARITH == "bf16x3":  # opt-in: every conv on the split-bf16 kernels (128x64x32 tile fits every Cout of the net)
                    ch = (_lib.ALGO_BF16X3_BASE + 6, 1)
                self.choices[(B, T, H, W)] = ch
            algo, splits = ch
        return ConvDesc(B, self.cin, T, H, W, self.cout, kt, kh, kw, st, sh, sw, pt, ph, pw, int(relu),
                        self.algo if algo is None else algo, self.splits if splits is None else splits)


def bn_fold(gamma, beta, mean, var, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval-mode BatchNorm -> (scale, shift) on device."""
    require_gpu(gamma, beta, mean, var)
    lib = _lib.load()
    c = gamma.numel()
    scale = torch.empty(c, device=gamma.device, dtype=torch.float32)
    shift = torch.empty_like(scale)
    check(lib.advhip_bn_fold_f32(ptr(gamma), ptr(beta), ptr(mean), ptr(var), C.c_float(eps), c, ptr(scale), ptr(shift), stream()), "bn_fold")
    return scale, shift


def _packed_rows(d: ConvDesc) -> int:
    kpad = _lib.load().advhip_conv3d_packed_rows(C.byref(d))
    if kpad < 0:
        check(kpad, "conv3d_packed_rows")
    return kpad


def _build_ktab(pc: PackedConv, thw: Tuple[int, int, int]) -> torch.Tensor:
    d = pc.desc(1, *thw, relu=False)
    ktab = torch.empty((_packed_rows(d) * 6,), device=pc.w_packed.device, dtype=torch.int32)
    check(_lib.load().advhip_conv3d_build_ktab(C.byref(d), ptr(ktab), stream()), "build_ktab")
    return ktab


def split_weight(pc: PackedConv) -> torch.Tensor:
    """The bf16 hi/lo weight images of `pc` (uint16 [2][Cout][Kpad]) for the ADVHIP_ALGO_BF16X3_* kernels."""
    if pc.w_split is None:
        kt, kh, kw = pc.kernel
        d = pc.desc(1, kt, kh, kw, relu=False, algo=0, splits=1)
        out = torch.empty((2, pc.cout, pc.w_packed.shape[0]), device=pc.weight.device, dtype=torch.int16)
        check(_lib.load().advhip_conv3d_pack_weight_bf16x3(C.byref(d), ptr(pc.weight), ptr(out), stream()), "pack_weight_bf16x3")
        pc.w_split = out
    return pc.w_split


def tfold_desc(d: ConvDesc) -> ConvDesc:
    """The dense 1x1x1 conv (B, Cin*T, 1, H, W) -> Cout*T that the (kt,1,1) conv `d` on T <= kt//2 + 1 frames is
    (include/advhip.h: advhip_conv3d_tfold_desc); raises HipExtensionError where the fold does not apply."""
    f = ConvDesc()
    check(_lib.load().advhip_conv3d_tfold_desc(C.byref(d), C.byref(f)), "conv3d_tfold_desc")
    return f


def tfold_operands(pc: PackedConv, thw: Tuple[int, int, int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(w_folded, ktab, scale, shift) of `pc` for the ADVHIP_ALGO_TFOLD_* launch on (T,H,W) inputs, built on the current
    stream on first use (the weights and the BN pair once per T, the table once per (T,H,W))."""
    T = thw[0]
    d = pc.desc(1, *thw, relu=False, algo=0, splits=1)
    ops_t = pc.tfold_w.get(T)
    ktab = pc.tfold_ktabs.get(thw)
    if ops_t is not None and ktab is not None:
        return ops_t[0], ktab, ops_t[1], ops_t[2]
    if pc.weight is None:
        raise _lib.HipExtensionError(f"{pc.name}: the temporal fold packs its operand from the torch-layout weights, which this conv does not keep")
    f = tfold_desc(d)
    lib = _lib.load()
    dev = pc.w_packed.device
    if ops_t is None:
        wf = torch.empty((_packed_rows(f), f.Cout), device=dev, dtype=torch.float32)
        check(lib.advhip_conv3d_pack_weight_tfold_f32(C.byref(d), ptr(pc.weight), ptr(wf), stream()), f"pack_weight_tfold[{pc.name}]")
        sc, sh = torch.empty((f.Cout,), device=dev, dtype=torch.float32), torch.empty((f.Cout,), device=dev, dtype=torch.float32)
        check(lib.advhip_conv3d_tfold_scale_shift_f32(C.byref(d), ptr(pc.scale), ptr(pc.shift), ptr(sc), ptr(sh), stream()), f"tfold_scale_shift[{pc.name}]")
        ops_t = pc.tfold_w[T] = (wf, sc, sh)
    if ktab is None:
        ktab = torch.empty((_packed_rows(f) * 6,), device=dev, dtype=torch.int32)
        check(lib.advhip_conv3d_build_ktab(C.byref(f), ptr(ktab), stream()), f"build_ktab_tfold[{pc.name}]")
        pc.tfold_ktabs[thw] = ktab
    return ops_t[0], ktab, ops_t[1], ops_t[2]


def ensure_ktab(pc: PackedConv, thw: Tuple[int, int, int], batch: Optional[int] = None) -> torch.Tensor:
    """The gather table of `pc` for input dims (T,H,W), built on the current stream on first use.  With `batch`, also
    every other lazily built operand the launch for (batch, T, H, W) will read -- the bf16 hi/lo weight images of the
    opt-in split-bf16 kernels, the folded operands of the temporal fold -- so that a caller about to fork streams has
    ALL of them behind one event."""
    ktab = pc.ktabs.get(thw)
    if ktab is None:
        ktab = pc.ktabs[thw] = _build_ktab(pc, thw)
    if batch is not None:
        d = pc.desc(batch, *thw, relu=False)
        if _lib.ALGO_BF16X3_BASE <= d.algo < _lib.ALGO_DMA2_BASE:
            split_weight(pc)
        if _lib.is_tfold(d.algo):
            tfold_operands(pc, thw)
    return ktab


def pack_conv(weight: torch.Tensor, gamma, beta, mean, var, eps: float, stride, padding, name: str = "",
              algo: int = _lib.ALGO_AUTO) -> PackedConv:
    """Pack one conv (torch layout (Cout,Cin,kt,kh,kw)) + its eval BatchNorm for the HIP kernels."""
    require_gpu(weight)
    weight = weight.detach().contiguous()
    cout, cin, kt, kh, kw = weight.shape
    scale, shift = bn_fold(gamma.detach(), beta.detach(), mean.detach(), var.detach(), eps)
    pc = PackedConv(cout, cin, (kt, kh, kw), _triple(stride), _triple(padding), weight, scale, shift, name=name, algo=algo)
    d = pc.desc(1, kt, kh, kw, relu=False)
    wp = torch.empty((_packed_rows(d), cout), device=weight.device, dtype=torch.float32)
    check(_lib.load().advhip_conv3d_pack_weight_f32(C.byref(d), ptr(weight), ptr(wp), stream()), "pack_weight")
    pc.w_packed = wp
    pc.weight = weight
    return pc


# ADV_ARITH=bf16x3: opt-in split-bf16 arithmetic for every conv (see include/advhip.h ADVHIP_ALGO_BF16X3_BASE); default: exact fp32
ARITH = os.environ.get("ADV_ARITH", "f32")

_WORKSPACES: Dict[Tuple[torch.device, int], torch.Tensor] = {}


def workspace(dev: torch.device, nbytes: int) -> Optional[torch.Tensor]:
    """Grow-only scratch for the split-K partial slabs (caller-owned, per the C ABI), one per
    (device, launch stream): launches on different streams may run at the same time."""
    if nbytes <= 0:
        return None
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _WORKSPACES[key] = torch.empty(((nbytes + 3) // 4,), device=dev, dtype=torch.float32)
    return ws


_ZERO_WORKSPACES: Dict[Tuple[torch.device, int], torch.Tensor] = {}


def zeroed_workspace(dev: torch.device, nbytes: int) -> Optional[torch.Tensor]:
    """Grow-only scratch per (device, launch stream) that is ZERO when handed out for the first time -- for kernels that keep
    arrival counters in it and leave them zero (advhip_gemm_nt_reduced_f32): zero-filled once per allocation, not per launch."""
    if nbytes <= 0:
        return None
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _ZERO_WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _ZERO_WORKSPACES[key] = torch.zeros(((nbytes + 3) // 4,), device=dev, dtype=torch.float32)
    return ws


_SPLITK_COUNTERS: Dict[Tuple[torch.device, int], torch.Tensor] = {}


def splitk_counters(dev: torch.device) -> torch.Tensor:
    """The arrival-counter block of the in-launch split-K reduction for launches on the current stream of `dev`
    (include/advhip.h: advhip_conv3d_epilogue.splitk_counters): zero-filled ONCE here; every launch leaves it zero."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    cnt = _SPLITK_COUNTERS.get(key)
    if cnt is None:
        cnt = _SPLITK_COUNTERS[key] = torch.zeros((16384,), device=dev, dtype=torch.int32)
    return cnt


def reset_stream_state(dev: Optional[torch.device] = None) -> None:
    """Forget the self-resetting counter block and the zero-initialised workspace of the current stream (of `dev`, default: the
    current device).  Those are zero-filled once and trusted to be left zero by every launch; a launch that did not run to its
    end -- an entry point that reported an error, a graph capture that was abandoned after it recorded the zero-fill -- may
    have broken that promise, so the next call allocates and zero-fills again.  `_lib.check` calls this on every reported error;
    call it yourself after abandoning a capture."""
    if not torch.cuda.is_available():
        return
    d = torch.device("cuda", torch.cuda.current_device()) if dev is None else dev
    key = (d, torch.cuda.current_stream(d).cuda_stream)
    _SPLITK_COUNTERS.pop(key, None)
    _ZERO_WORKSPACES.pop(key, None)


_lib.ON_FAILURE.append(reset_stream_state)


def batch_stride(t: torch.Tensor) -> int:
    """Elements between consecutive samples of an NCDHW tensor that is contiguous per sample: a contiguous tensor,
    or a channel slice `wide[:, a:b]` of one (the kernels take the batch stride; everything inside a sample must be
    dense).  Raises for any other layout."""
    n, c, t_, h, w = t.shape
    inner = (t_ * h * w, h * w, w, 1)
    for dim in range(1, 5):
        if t.shape[dim] > 1 and t.stride(dim) != inner[dim - 1]:
            raise ValueError(f"tensor {tuple(t.shape)} with strides {tuple(t.stride())} is not dense within a sample")
    return int(t.stride(0)) if n > 1 else c * inner[0]


def conv3d_bn_act(x: torch.Tensor, pc: PackedConv, relu: bool = True, residual: Optional[torch.Tensor] = None,
                  algo: Optional[int] = None, out: Optional[torch.Tensor] = None, splits: Optional[int] = None) -> torch.Tensor:
    """act(conv3d(x) * scale + shift (+ residual)) in one fused HIP launch.  `x` and `out` may be channel slices of wider
    NCDHW tensors (see batch_stride); the residual must be contiguous."""
    require_gpu(x, out, contiguous=False)
    require_gpu(residual)
    if x.dim() != 5 or x.shape[1] != pc.cin:
        raise ValueError(f"{pc.name}: expected (B,{pc.cin},T,H,W), got {tuple(x.shape)}")
    B, _, T, H, W = x.shape
    to, ho, wo = conv_out_dims((T, H, W), pc.kernel, pc.stride, pc.padding)
    if min(to, ho, wo) <= 0:
        raise ValueError(f"{pc.name}: input {tuple(x.shape)} smaller than the kernel")
    y = out if out is not None else torch.empty((B, pc.cout, to, ho, wo), device=x.device, dtype=torch.float32)
    if tuple(y.shape) != (B, pc.cout, to, ho, wo) or y.dtype != torch.float32 or y.device != x.device:
        raise ValueError(f"{pc.name}: out {tuple(y.shape)} {y.dtype} on {y.device} != {(B, pc.cout, to, ho, wo)} float32 on {x.device}")
    if residual is not None and residual.shape != y.shape:
        raise ValueError(f"{pc.name}: residual {tuple(residual.shape)} != output {tuple(y.shape)}")
    ktab = ensure_ktab(pc, (T, H, W))
    if algo is not None and splits is None:
        splits = 1  # an explicitly pinned tile runs unsplit unless the caller also pins the split
    d = pc.desc(B, T, H, W, relu, algo, splits)
    lib = _lib.load()
    need = lib.advhip_conv3d_workspace_bytes(C.byref(d))
    if need < 0:
        check(int(need), f"conv3d_workspace_bytes[{pc.name}]")
    ws = workspace(x.device, need)
    w, scale, shift = pc.w_packed, pc.scale, pc.shift
    if _lib.ALGO_BF16X3_BASE <= d.algo < _lib.ALGO_DMA2_BASE:
        w = split_weight(pc)
    if _lib.is_tfold(d.algo):  # the same memory as a dense 1x1x1 conv over Cin*T channels: only the operands differ
        w, ktab, scale, shift = tfold_operands(pc, (T, H, W))
    xbs, ybs = batch_stride(x), batch_stride(y)  # (x and / or y may be a channel slice of a wider tensor)
    ep = None
    if need > 0:  # split-K: this stream's self-resetting arrival counters instead of a memset ahead of every launch
        cnt = splitk_counters(x.device)
        ep = C.byref(_lib.ConvEpilogue(None, None, None, None, None, ptr(cnt), cnt.numel() * 4))
    check(lib.advhip_conv3d_bn_act_ex_f32(C.byref(d), ptr(x), xbs, ptr(w), ptr(ktab), ptr(scale), ptr(shift), ptr(residual), ptr(y), ybs,
                                          ep, ptr(ws), need, stream()), f"conv3d[{pc.name}]")
    return y


def conv_pool_out_dims(in_thw: Sequence[int], pc: "PackedConv", pool_kernel, pool_stride) -> Tuple[int, int, int]:
    """(T, H, W) of conv `pc` on in_thw followed by a floor-mode, padding-0 max-pool."""
    return conv_out_dims(conv_out_dims(in_thw, pc.kernel, pc.stride, pc.padding), _triple(pool_kernel), _triple(pool_stride), (0, 0, 0))


# The fused stem can gather 16-byte pieces from column-parity planes of its input (advhip.h: advhip_conv3d_s2w_*): the conv
# launch is 6.5 % faster (2.25 vs 2.41 ms at B = 32), the planes cost a pass over the input (0.145 ms for an fp32 NCDHW
# tensor).  For resized uint8 frames the TenCrop / normalise pass writes the planes itself, so that path uses them by default
# (U8_STEM_FORM "planes"); for an fp32 NCDHW input the extra pass cancels the gain in isolation and adds 0.7 GB of HBM
# traffic per step; in the three-lane stream it buys +0.4 % on the 20-step line and +0.7 % sustained (round 5, four alternating
# runs on one box: 3 796 -> 3 812 and 3 846 -> 3 872 clips/s; round 3 on its kernels: +0.3 %), bit-identical features: ON by
# default since round 5 (ADV_STEM_S2W=0: the 4-byte gather straight from the NCDHW tensor).
STEM_S2W = os.environ.get("ADV_STEM_S2W", "1") == "1"
# The planes-form stem can split its launch by pool window in t (advhip.h: ADVHIP_ALGO_STEM_BORDER): the windows at either end of
# the clip run frame by frame on 1(t) x 8(h) x 16(w) tiles that skip the k-tiles whose temporal taps all lie in the padding (23 of
# 368 per sample column at T = 16, 6.25 % of the stem's MFMAs), the max over their two frames moves to the merge pass; bit-identical
# features.  ADV_STEM_BORDER=0: the single launch on 2-frame bricks.
STEM_BORDER = os.environ.get("ADV_STEM_BORDER", "1") == "1"


def s2w_ok(pc: PackedConv, W: int) -> bool:
    """Stride 2, odd kernel <= 9 with padding kw // 2 along w, W even and W / 2 a multiple of 4 (advhip.h: advhip_conv3d_s2w_*)."""
    kw, sw, pw = pc.kernel[2], pc.stride[2], pc.padding[2]
    return sw == 2 and kw % 2 == 1 and pw == kw // 2 and pw <= 4 and W % 8 == 0 and W >= 8 and pc.kernel[0] <= 10 and pc.kernel[1] <= 10


def split_w(x: torch.Tensor) -> torch.Tensor:
    """(B, C, T, H, W) contiguous -> (B, C, T, H, 2, W/2 + 4): the even and odd columns of every row as two zero-padded planes
    (one HIP pass; the operand of the stem's 16-byte gather, include/advhip.h: advhip_split_w_f32)."""
    require_gpu(x)
    B, Cc, T, H, W = x.shape
    lib = _lib.load()
    wp = lib.advhip_split_w_plane_floats(W)
    if wp < 0:
        raise ValueError(f"split_w: W = {W} must be even")
    xs = torch.empty((B, Cc, T, H, 2, wp), device=x.device, dtype=torch.float32)
    check(lib.advhip_split_w_f32(ptr(x), ptr(xs), B * Cc * T * H, W, stream(x)), "split_w")
    return xs


def ensure_ktab_s2w(pc: PackedConv, thw: Tuple[int, int, int]) -> torch.Tensor:
    tab = pc.ktabs_s2w.get(thw)
    if tab is None:
        d = pc.desc(1, *thw, relu=True, algo=0, splits=1)
        tab = torch.empty((_packed_rows(d) * 2,), device=pc.w_packed.device, dtype=torch.int32)
        check(_lib.load().advhip_conv3d_s2w_build_ktab(C.byref(d), ptr(tab), stream()), "build_ktab_s2w")
        pc.ktabs_s2w[thw] = tab
    return tab


def active_ktiles(pc: PackedConv, thw: Tuple[int, int, int], ot: int, bk: int = 16) -> list:
    """The k-tiles of `bk` packed rows that hold a row whose temporal tap lies inside the clip for output frame `ot` of `pc` on
    (T, H, W) inputs, ascending (host arithmetic: advhip_conv3d_active_ktiles) -- what a frame-uniform stem tile multiplies."""
    d = pc.desc(1, *thw, relu=True, algo=0, splits=1)
    k = pc.cin * pc.kernel[0] * pc.kernel[1] * pc.kernel[2]
    tiles = (C.c_int32 * ((k + bk - 1) // bk))()
    n = C.c_int32()
    check(_lib.load().advhip_conv3d_active_ktiles(C.byref(d), ot, bk, tiles, C.byref(n)), f"conv3d_active_ktiles[{pc.name}]")
    return list(tiles[: n.value])


def _pool233_out(pc: PackedConv, d: ConvDesc, what: str, out: Optional[torch.Tensor], dev: torch.device):
    """What the three fused-stem wrappers share behind their own argument checks: the (2,3,3) / (2,2,2)-pooled output of the conv
    `d` describes (`out`, checked, or a new tensor) and the launch's workspace -> (y, workspace, its bytes).  `what` names the
    input in the too-small message."""
    lib = _lib.load()
    tp, hp, wp = C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.advhip_conv3d_pool_out_dims(C.byref(d), 2, 3, 3, 2, 2, 2, C.byref(tp), C.byref(hp), C.byref(wp)), "conv3d_pool_out_dims")
    shape = (d.B, pc.cout, tp.value, hp.value, wp.value)
    if min(shape) <= 0:
        raise ValueError(f"{pc.name}: {what} too small for conv + (2,3,3) pooling")
    y = out if out is not None else torch.empty(shape, device=dev, dtype=torch.float32)
    if tuple(y.shape) != shape or y.dtype != torch.float32 or y.device != dev:
        raise ValueError(f"{pc.name}: out {tuple(y.shape)} != {shape}")
    need = lib.advhip_conv3d_relu_maxpool233_workspace_bytes(C.byref(d))
    if need < 0:
        check(int(need), f"conv3d_relu_maxpool233_workspace_bytes[{pc.name}]")
    return y, workspace(dev, need), need


def conv3d_s2w_bn_relu_maxpool233(xs: torch.Tensor, pc: PackedConv, out: Optional[torch.Tensor] = None, border: Optional[bool] = None) -> torch.Tensor:
    """The fused stem on column-parity planes xs (B, Cin, T, H, 2, W/2 + 4) of its input (split_w / tencrop_planes_u8).
    `border` (default STEM_BORDER): split the launch by pool window in t where the geometry allows (ADVHIP_ALGO_STEM_BORDER);
    same results bit for bit."""
    require_gpu(xs)
    require_gpu(out, contiguous=False)
    if xs.dim() != 6 or xs.shape[1] != pc.cin or xs.shape[4] != 2:
        raise ValueError(f"{pc.name}: expected planes (B,{pc.cin},T,H,2,W/2+4), got {tuple(xs.shape)}")
    B, _, T, H, _, wp = xs.shape
    W = 2 * (wp - 4)
    if not s2w_ok(pc, W):
        raise ValueError(f"{pc.name}: the column-parity gather does not apply to W = {W} with k/s/p {pc.kernel[2]}/{pc.stride[2]}/{pc.padding[2]}")
    d = pc.desc(B, T, H, W, True, _lib.ALGO_STEM_BORDER if (STEM_BORDER if border is None else border) else 0, 1)
    y, ws, need = _pool233_out(pc, d, "input", out, xs.device)
    check(_lib.load().advhip_conv3d_s2w_bn_relu_maxpool233_f32(C.byref(d), ptr(xs), 0, ptr(pc.w_packed), ptr(ensure_ktab_s2w(pc, (T, H, W))),
                                                               ptr(pc.scale), ptr(pc.shift), ptr(y), batch_stride(y), ptr(ws), need, stream(xs)),
          f"conv3d s2w+pool233[{pc.name}]")
    return y


def resolve_frame_step(frame_step: Optional[int]) -> int:
    """The temporal sampling step d: sampled frame t of a window is source frame start + t * d.  None = 1 (consecutive frames, the
    reference's clips); an integer >= 1."""
    if frame_step is None:
        return 1
    if isinstance(frame_step, bool) or not isinstance(frame_step, numbers.Integral) or int(frame_step) < 1:
        raise ValueError(f"frame_step {frame_step!r}: an integer >= 1")
    return int(frame_step)


def resolve_clip_stride(frames_per_clip: int, clip_stride: Optional[int], frame_step: Optional[int] = None) -> int:
    """The distance between window starts.  A window spans frames_per_clip * frame_step frames: None = that span (back-to-back
    spans; frame_step 1: the reference's back-to-back clips); 1 <= s <= span (a larger stride would leave frames in no span)."""
    d = resolve_frame_step(frame_step)
    span = frames_per_clip * d
    s = span if clip_stride is None else int(clip_stride)
    if not 1 <= s <= span:
        if d == 1:
            raise ValueError(f"clip_stride {clip_stride} outside [1, frames_per_clip = {frames_per_clip}]")
        raise ValueError(f"clip_stride {clip_stride} outside [1, frames_per_clip * frame_step = {span}]")
    return s


def n_windows(n_frames: int, frames_per_clip: int = 16, clip_stride: Optional[int] = None, frame_step: Optional[int] = None) -> int:
    """Windows of a video of `n_frames`: window w starts at frame w * clip_stride and spans frames_per_clip * frame_step frames,
    and the last one is the first whose span reaches the video's end (it may be short: LoopPad).  frame_step 1, clip_stride =
    frames_per_clip: (F - 1) // fpc + 1, the reference's clip count (src/dataset.py)."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    if n_frames < 1:
        raise ValueError(f"n_windows: {n_frames} frames")
    return 1 + max(0, -(-(n_frames - frames_per_clip * d) // s))


def buffer_frames(n: int, frames_per_clip: int = 16, clip_stride: Optional[int] = None, frame_step: Optional[int] = None) -> int:
    """Frames of a buffer that holds `n` WHOLE windows, as the fused stems read it: it ends with the last window's last sampled
    frame, (n - 1) * clip_stride + (frames_per_clip - 1) * frame_step + 1 (frame_step 1, back-to-back clips: n * frames_per_clip)."""
    d = resolve_frame_step(frame_step)
    return (n - 1) * resolve_clip_stride(frames_per_clip, clip_stride, d) + (frames_per_clip - 1) * d + 1


def buffer_windows(n_frames: int, frames_per_clip: int = 16, clip_stride: Optional[int] = None, frame_step: Optional[int] = None) -> int:
    """Whole windows at the head of a buffer of `n_frames` (0: not even one); the buffer is whole where buffer_frames of that
    count gives `n_frames` back."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    return max(0, (n_frames - buffer_frames(1, frames_per_clip, s, d)) // s + 1)


def window_frame_indices(n_frames: int, w: int, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                         frame_step: Optional[int] = None) -> Tuple[int, ...]:
    """The frames_per_clip source frames window `w` of a video of `n_frames` is made of, LoopPad included: w * s + (t % L) * d with
    L = min(frames_per_clip, ceil((n_frames - w * s) / d)) -- what the kernels address."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    if not 0 <= w < n_windows(n_frames, frames_per_clip, s, d):
        raise ValueError(f"window {w} of a video of {n_frames} frames")
    length = min(frames_per_clip, -(-(n_frames - w * s) // d))
    return tuple(w * s + (t % length) * d for t in range(frames_per_clip))


CROP_SETS = {"ten": tuple(range(10)), "five": (0, 1, 2, 3, 4), "center": (4,), "centre": (4,), "center_flip": (4, 9)}


def resolve_crops(crops) -> Tuple[int, ...]:
    """A crop subset of TenCrop as a strictly ascending tuple of indices 0..9: 0-3 top-left, top-right, bottom-left,
    bottom-right, 4 centre, 5-9 the same five windows of the horizontally flipped frame.  None / "ten" = all ten, "five" =
    (0..4), "center" / "centre" = (4,), "center_flip" = (4, 9), or 1 to 10 indices.  Ascending order keeps the crop order
    TenCrop's own; duplicates, descending or out-of-range indices and an empty set raise ValueError."""
    if crops is None:
        return CROP_SETS["ten"]
    if isinstance(crops, str):
        if crops not in CROP_SETS:
            raise ValueError(f"crops {crops!r}: not one of {sorted(CROP_SETS)} or a tuple of TenCrop indices")
        return CROP_SETS[crops]
    try:
        idx = tuple(crops)
    except TypeError:
        raise ValueError(f"crops {crops!r}: a name or a tuple of TenCrop indices") from None
    if not 1 <= len(idx) <= 10:
        raise ValueError(f"crops {crops!r}: 1 to 10 indices")
    for c in idx:
        if isinstance(c, bool) or not isinstance(c, numbers.Integral) or not 0 <= int(c) <= 9:
            raise ValueError(f"crops {crops!r}: indices are integers in 0..9")
    idx = tuple(int(c) for c in idx)
    if any(b <= a for a, b in zip(idx, idx[1:])):
        raise ValueError(f"crops {crops!r}: indices must be strictly ascending (TenCrop order, no duplicates)")
    return idx


def resolve_sampling(frames_per_clip: int, clip_stride: Optional[int] = None, crops=None,
                     frame_step: Optional[int] = None) -> Tuple[int, Tuple[int, ...], int]:
    """The three clip-sampling arguments resolved once: (clip_stride, crops, frame_step) as resolve_clip_stride, resolve_crops and
    resolve_frame_step give them."""
    d = resolve_frame_step(frame_step)
    return resolve_clip_stride(frames_per_clip, clip_stride, d), resolve_crops(crops), d


def pack_crops(crops) -> Tuple[int, int]:
    """(ncrops, packed) as the kernels take a crop set: index j in bits [4 j, 4 j + 4) of one 64-bit launch argument."""
    idx = resolve_crops(crops)
    return len(idx), sum(c << (4 * j) for j, c in enumerate(idx))


def unpack_crops(ncrops: int, packed: int) -> Tuple[int, ...]:
    return tuple((packed >> (4 * j)) & 15 for j in range(ncrops))


def crops_tag(crops) -> str:
    """The file-name tag of a crop subset: "" for all ten, else "_c<digits>" ("_c4", "_c01234")."""
    idx = resolve_crops(crops)
    return "" if len(idx) == 10 else "_c" + "".join(str(c) for c in idx)


PIXEL_MEAN, PIXEL_STD = 114.75, 57.375  # GroupNormalize constants, src/dataset.py:180-181


class Normalize(NamedTuple):
    """A normalisation of the uint8-frame path in canonical form (resolve_normalize): `kind` and two per-channel triples of
    Python floats -- (mean, std) for "standardize", (lo, hi) for the two min-max kinds."""

    kind: str
    a: Tuple[float, float, float]
    b: Tuple[float, float, float]


# kind -> (its default parameters, its file-name tag, its ADVHIP_NORM_* mode)
NORMALIZE_KINDS = {"standardize": ((114.75, 57.375), "_nstd", _lib.NORM_STANDARDIZE),
                   "pixel_minmax": ((0.0, 1.0), "_npix", _lib.NORM_PIXEL_MINMAX),
                   "channel_minmax": ((0.0, 1.0), "_nch", _lib.NORM_CHANNEL_MINMAX)}


def _f32(v: float) -> float:
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _norm_triple(spec, v, scalar_only: bool) -> Tuple[float, float, float]:
    def num(x):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(float(x)) or abs(float(x)) > 3.0e38:
            raise ValueError(f"normalize {spec!r}: parameters are finite numbers (fp32 range)")
        return float(x)

    if isinstance(v, numbers.Real) and not isinstance(v, bool):
        return (num(v),) * 3
    try:
        t = tuple(v)
    except TypeError:
        raise ValueError(f"normalize {spec!r}: a parameter is a number or three numbers, one per channel") from None
    if len(t) != 3:
        raise ValueError(f"normalize {spec!r}: a per-channel parameter has three entries")
    t = tuple(num(x) for x in t)
    if scalar_only and not t[0] == t[1] == t[2]:
        raise ValueError(f"normalize {spec!r}: pixel_minmax takes one range for all channels")
    return t


def resolve_normalize(spec) -> Normalize:
    """The normalisation of a uint8-frame call in canonical form, the reference's three normalisers (src/gtransforms.py:57-112):
      None, "standardize", ("standardize", mean, std): (x - mean[c]) / std[c]; default (114.75, 57.375), the reference's own, and
          in that form "none" in every respect: the existing kernels, no file-name tag;
      "pixel_minmax", ("pixel_minmax", lo, hi): (x - mn) / (mx - mn) * (hi - lo) + lo with mn, mx over all channels of each
          (frame, crop); scalars, lo < hi, default (0, 1);
      "channel_minmax", ("channel_minmax", lo, hi): the same with mn, mx, lo, hi per channel; at least one channel has lo < hi
          (the reference's condition), default (0, 1).
    A parameter is a number (broadcast to the three channels) or three numbers; ints are numbers (the reference's
    isinstance(x, float) quirk, where an int builds an empty tensor, is not reproduced).  Anything else raises ValueError."""
    if isinstance(spec, Normalize):
        kind, params = spec.kind, (spec.a, spec.b)
    elif spec is None:
        kind, params = "standardize", None
    elif isinstance(spec, str):
        kind, params = spec, None
    else:
        try:
            t = tuple(spec)
        except TypeError:
            raise ValueError(f"normalize {spec!r}: a kind, or (kind, a, b)") from None
        if len(t) != 3 or not isinstance(t[0], str):
            raise ValueError(f"normalize {spec!r}: a kind, or (kind, a, b)")
        kind, params = t[0], t[1:]
    if kind not in NORMALIZE_KINDS:
        raise ValueError(f"normalize {spec!r}: kind is one of {sorted(NORMALIZE_KINDS)}")
    if params is None:
        params = NORMALIZE_KINDS[kind][0]
    a, b = (_norm_triple(spec, v, kind == "pixel_minmax") for v in params)
    if kind == "standardize":
        if any(_f32(s) == 0.0 for s in b):
            raise ValueError(f"normalize {spec!r}: std must be non-zero")
    elif kind == "pixel_minmax":
        if not a[0] < b[0]:
            raise ValueError(f"normalize {spec!r}: lo must be below hi")
    elif not any(lo < hi for lo, hi in zip(a, b)):
        raise ValueError(f"normalize {spec!r}: lo must be below hi in at least one channel")
    return Normalize(kind, a, b)


def normalize_is_default(spec) -> bool:
    """The reference's own (x - 114.75) / 57.375 under any of its spellings (compared as the fp32 values the kernels take)."""
    n = resolve_normalize(spec)
    return n.kind == "standardize" and all(_f32(m) == PIXEL_MEAN for m in n.a) and all(_f32(s) == PIXEL_STD for s in n.b)


def normalize_tag(spec) -> str:
    """The file-name tag of a normalisation: "" for the default; else "_nstd", "_npix" or "_nch", and where the parameters are not
    that kind's defaults "-" plus the first 8 hex digits of the SHA-1 of the six parameters as little-endian fp32 (mean or lo of
    the three channels, then std or hi): "_npix", "_npix-5a2b...", "_nstd-...".  (Ranges that differ only below fp32 precision
    share a tag.)"""
    n = resolve_normalize(spec)
    if normalize_is_default(n):
        return ""
    (da, db), tag, _ = NORMALIZE_KINDS[n.kind]
    if all(_f32(v) == _f32(da) for v in n.a) and all(_f32(v) == _f32(db) for v in n.b):
        return tag
    return tag + "-" + hashlib.sha1(struct.pack("<6f", *n.a, *n.b)).hexdigest()[:8]


def crop_stats_pitch(frames_per_clip: int, clip_stride: Optional[int] = None, frame_step: Optional[int] = None) -> int:
    """The frame pitch of a call's statistics table: gcd(clip_stride, frame_step) -- every frame any window samples, w * clip_stride
    + t * frame_step, is a multiple of it (frame_step 1: every frame)."""
    d = resolve_frame_step(frame_step)
    return math.gcd(resolve_clip_stride(frames_per_clip, clip_stride, d), d)


def crop_minmax_u8(frames: torch.Tensor, crop: int = 224, frame_pitch: int = 1) -> torch.Tensor:
    """Resized uint8 frames (F, H, W, C) -> uint8 (ceil(F / frame_pitch), 6, C, 2): (min, max) per channel of the six windows
    that hold the pixels of TenCrop's ten crops -- the four corners, the centre, and the centre of the mirrored frame (the
    centre's own window only where W - crop is even) -- of frames 0, frame_pitch, 2 * frame_pitch, ...: crop j < 5 has window j's
    pixels, a mirrored corner 5..8 those of the opposite corner (j - 5) ^ 1, crop 9 those of window 5.  The statistics of the
    min-max normalisations, one HIP launch, exact."""
    frames = frames.contiguous()
    require_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"expected uint8 (F,H,W,C), got {frames.dtype} {tuple(frames.shape)}")
    f, h, w, c = frames.shape
    if isinstance(frame_pitch, bool) or not isinstance(frame_pitch, numbers.Integral) or frame_pitch < 1:
        raise ValueError(f"crop_minmax_u8: frame_pitch {frame_pitch!r}: an integer >= 1")
    if f < 1 or h < crop or w < crop or crop < 1:
        raise ValueError(f"crop_minmax_u8: {f} frames of {h}x{w}, crop {crop}")
    stats = torch.empty((-(-f // int(frame_pitch)), 6, c, 2), device=frames.device, dtype=torch.uint8)
    check(_lib.load().advhip_crop_minmax_u8(ptr(frames), ptr(stats), f, h, w, c, crop, int(frame_pitch), stream(frames)), "crop_minmax_u8")
    return stats


def normalize_launch_args(norm: Normalize, frames: torch.Tensor, crop: int, frames_per_clip: int, clip_stride: int, frame_step: int,
                          crop_stats: Optional[torch.Tensor]):
    """(mode, a, b, stats, stats_pitch) as the `_modes` entry points take them for `frames` (F, H, W, C) on the device: the
    min-max kinds' table is `crop_stats` (checked against the call's pitch and frames) or computed here on the current stream."""
    mode = NORMALIZE_KINDS[norm.kind][2]
    a, b = (C.c_double * 3)(*norm.a), (C.c_double * 3)(*norm.b)
    pitch = crop_stats_pitch(frames_per_clip, clip_stride, frame_step)
    if mode == _lib.NORM_STANDARDIZE:
        return mode, a, b, None, pitch
    if crop_stats is None:
        crop_stats = crop_minmax_u8(frames, crop, pitch)
    else:
        require_gpu(crop_stats)
        want = (-(-frames.shape[0] // pitch), 6, frames.shape[3], 2)
        if crop_stats.dtype != torch.uint8 or tuple(crop_stats.shape) != want or crop_stats.device != frames.device:
            raise ValueError(f"crop_stats {crop_stats.dtype} {tuple(crop_stats.shape)} on {crop_stats.device}: expected uint8 {want} on "
                             f"{frames.device} (ops.crop_minmax_u8 at frame pitch {pitch})")
    return mode, a, b, crop_stats, pitch


def normalize_permute_u8(frames: torch.Tensor, mean: float = PIXEL_MEAN, std: float = PIXEL_STD) -> torch.Tensor:
    """uint8 (N, T, C, H, W) -> fp32 (N, C, T, H, W), (x - mean) / std, one HIP pass."""
    frames = frames.contiguous()
    require_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 5:
        raise ValueError(f"expected uint8 (N,T,C,H,W), got {frames.dtype} {tuple(frames.shape)}")
    n, t, c, h, w = frames.shape
    out = torch.empty((n, c, t, h, w), device=frames.device, dtype=torch.float32)
    check(_lib.load().advhip_normalize_permute_u8(ptr(frames), ptr(out), n, t, c, h, w, C.c_float(mean), C.c_float(std), stream()),
          "normalize_permute_u8")
    return out


def _tencrop_call(who: str, frames: torch.Tensor, frames_per_clip: int, mean: float, std: float, clip_stride, crops, frame_step, normalize):
    """What the two TenCrop passes do before they look at their own arguments: the sampling and the normalisation resolved, the
    frames checked.  -> (frames, (clip_stride, frame_step, ncrops, packed crops), norm, the video's crop-clips)."""
    s, crops, d = resolve_sampling(frames_per_clip, clip_stride, crops, frame_step)
    nc, packed = pack_crops(crops)
    norm = resolve_normalize(normalize)
    frames = frames.contiguous()
    require_gpu(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"expected uint8 (F,H,W,C), got {frames.dtype} {tuple(frames.shape)}")
    if not normalize_is_default(norm) and (mean, std) != (PIXEL_MEAN, PIXEL_STD):
        raise ValueError(f"{who}: give the constants in `normalize`, not in `mean` / `std` as well")
    return frames, (s, d, nc, packed), norm, n_windows(frames.shape[0], frames_per_clip, s, d) * nc


def _tencrop_launch(name: str, frames: torch.Tensor, out: torch.Tensor, frames_per_clip: int, crop: int, sampling, window, norm: Normalize,
                    mean: float, std: float, crop_stats: Optional[torch.Tensor]) -> torch.Tensor:
    """advhip_<name>_sampled with the scalar pair for the default normalisation, advhip_<name>_modes for any other.  `window`: the
    arguments between the crop set and the normalisation -- (first, count) of the planes pass, () of the dense one."""
    lib = _lib.load()
    f, h, w, c = frames.shape
    s, d, nc, packed = sampling
    head = (ptr(frames), ptr(out), f, h, w, c, frames_per_clip, s, d, crop, nc, packed, *window)
    if normalize_is_default(norm):
        check(getattr(lib, f"advhip_{name}_sampled")(*head, C.c_float(mean), C.c_float(std), stream(frames)), name)
    else:
        mode, a, b, stats, pitch = normalize_launch_args(norm, frames, crop, frames_per_clip, s, d, crop_stats)
        check(getattr(lib, f"advhip_{name}_modes")(*head, mode, a, b, ptr(stats), pitch, stream(frames)), f"{name}_modes")
    return out


def tencrop_normalize_u8(frames: torch.Tensor, frames_per_clip: int = 16, crop: int = 224, mean: float = PIXEL_MEAN,
                         std: float = PIXEL_STD, clip_stride: Optional[int] = None, crops=None,
                         frame_step: Optional[int] = None, normalize=None, crop_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Resized uint8 frames (F, H, W, C) of one video -> the backbone's input (n_clips * 10, C, frames_per_clip, crop, crop)
    fp32: TenCrop, float, normalise, LoopPad and the layout permutes of TenCropVideoFrameDataset / _extract
    (src/dataset.py:175-195, src/gtransforms.py, extract_features.py:83) in one HIP pass.  Row = clip * 10 + crop.
    `clip_stride` (default frames_per_clip): clip w starts at frame w * clip_stride, n_clips = n_windows(F, ...).
    `crops` (resolve_crops; default all ten): (n_clips * len(crops), ...), row = clip * len(crops) + j holds crop crops[j].
    `frame_step` d (default 1): sampled frame t of clip w is frames[w * clip_stride + t * d]; a clip spans frames_per_clip * d
    frames, clip_stride defaults to that span (1 <= clip_stride <= span), and a short last clip of L = ceil((F - w * s) / d)
    sampled frames repeats them (LoopPad): frame t >= L is frames[w * s + (t % L) * d].  Row w is the row of the call without
    `frame_step` on those frames as a one-clip video, bit for bit; nothing is gathered.
    `normalize` (resolve_normalize; default: (x - mean) / std with the two scalars): ("standardize", mean, std) with
    per-channel lists, "pixel_minmax" / ("pixel_minmax", lo, hi) or "channel_minmax" / ("channel_minmax", lo, hi) -- the
    reference's three normalisers (src/gtransforms.py:57-112), bit for bit, NaN for a constant crop / channel included.  The
    min-max kinds read per-(frame, window, channel) statistics: `crop_stats` (crop_minmax_u8 at frame pitch
    crop_stats_pitch(frames_per_clip, clip_stride, frame_step)), computed here when not given."""
    frames, sampling, norm, n = _tencrop_call("tencrop_normalize_u8", frames, frames_per_clip, mean, std, clip_stride, crops, frame_step, normalize)
    _, h, w, c = frames.shape
    if h < crop or w < crop:
        raise ValueError(f"frames {h}x{w} smaller than the {crop} crop")
    out = torch.empty((n, c, frames_per_clip, crop, crop), device=frames.device, dtype=torch.float32)
    return _tencrop_launch("tencrop_normalize_u8", frames, out, frames_per_clip, crop, sampling, (), norm, mean, std, crop_stats)


def tencrop_planes_u8(frames: torch.Tensor, first: int, count: int, frames_per_clip: int = 16, crop: int = 224, mean: float = PIXEL_MEAN,
                      std: float = PIXEL_STD, clip_stride: Optional[int] = None, crops=None, frame_step: Optional[int] = None,
                      normalize=None, crop_stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tencrop_normalize_u8's rows [first, first + count) as column-parity planes (count, C, frames_per_clip, crop, 2,
    crop/2 + 4): the same arguments, the same values, written as the operand of the stem's 16-byte gather with zero padding
    columns (include/advhip.h: advhip_conv3d_s2w_*)."""
    frames, sampling, norm, n = _tencrop_call("tencrop_planes_u8", frames, frames_per_clip, mean, std, clip_stride, crops, frame_step, normalize)
    _, h, w, c = frames.shape
    if h < crop or w < crop or crop % 2 or first < 0 or count <= 0 or first + count > n:
        raise ValueError(f"tencrop_planes_u8: crop-clips [{first},{first + count}) of {n}, frames {h}x{w}, crop {crop}")
    xs = torch.empty((count, c, frames_per_clip, crop, 2, crop // 2 + 4), device=frames.device, dtype=torch.float32)
    return _tencrop_launch("tencrop_normalize_planes_u8", frames, xs, frames_per_clip, crop, sampling, (first, count), norm, mean, std, crop_stats)


def conv3d_bn_relu_maxpool233(x: torch.Tensor, pc: PackedConv, out: Optional[torch.Tensor] = None, s2w: Optional[bool] = None,
                              border: Optional[bool] = None) -> torch.Tensor:
    """maxpool3d(relu(conv3d(x) * scale + shift), (2,3,3), (2,2,2)) without the un-pooled activation ever reaching HBM
    (the stem of I3Res50, src/i3d.py:303-306).  Bit-identical to conv3d_bn_act(relu=True) + maxpool3d.  `s2w` (default: where
    the geometry allows): gather 16-byte pieces from column-parity planes of x (one extra pass over x, 4x fewer gather
    instructions in the conv; same results bit for bit).  `border`: see conv3d_s2w_bn_relu_maxpool233 (the planes form only)."""
    require_gpu(x, out, contiguous=False)
    if x.dim() != 5 or x.shape[1] != pc.cin:
        raise ValueError(f"{pc.name}: expected (B,{pc.cin},T,H,W), got {tuple(x.shape)}")
    B, _, T, H, W = x.shape
    d = pc.desc(B, T, H, W, True, 0, 1)
    y, ws, need = _pool233_out(pc, d, f"input {tuple(x.shape)}", out, x.device)
    ktab = ensure_ktab(pc, (T, H, W))
    if s2w is None:
        s2w = STEM_S2W
    if s2w and s2w_ok(pc, W) and x.is_contiguous():
        return conv3d_s2w_bn_relu_maxpool233(split_w(x), pc, out=y, border=border)
    xbs, ybs = batch_stride(x), batch_stride(y)
    check(_lib.load().advhip_conv3d_bn_relu_maxpool233_f32(C.byref(d), ptr(x), xbs, ptr(pc.w_packed), ptr(ktab), ptr(pc.scale), ptr(pc.shift),
                                                           ptr(y), ybs, ptr(ws), need, stream()), f"conv3d+pool233[{pc.name}]")
    return y


# how forward_frames feeds the stem from resized uint8 frames: "planes" (default where the geometry allows): one TenCrop /
# normalise pass writing column-parity planes + the 16-byte-gather stem (features equal the fp32 pipeline's bit for bit);
# "taps": the stem kernel reads whole pixels itself (one 4-byte gather per tap, no fp32 tensor at all); "bytes": one byte
# gather per (channel, tap)
U8_STEM_FORM = os.environ.get("ADV_U8_STEM", "planes")


def readable_bytes(t: torch.Tensor) -> int:
    """Bytes of the tensor's allocation from its first element on."""
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def with_slack(frames: torch.Tensor, slack: int = 4) -> torch.Tensor:
    """`frames` in an allocation that extends `slack` bytes past its last element (a copy only if it does not already)."""
    if readable_bytes(frames) >= frames.numel() + slack:
        return frames
    buf = torch.empty((frames.numel() + slack,), device=frames.device, dtype=torch.uint8)
    buf[: frames.numel()].copy_(frames.reshape(-1))
    return buf[: frames.numel()].view(frames.shape)


def pad_windows_u8(frames: torch.Tensor, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                   frame_step: Optional[int] = None) -> torch.Tensor:
    """`frames` (F, H, W, C) on the device as WHOLE windows, (n - 1) * clip_stride + frames_per_clip frames: a short last window's
    LoopPad frames (src/gtransforms.py:119-132: frame (n - 1) * s + t % len for t in [len, frames_per_clip)) appended behind
    frame F - 1 -- a uint8 gather of < frames_per_clip frames; only the last window reads them.  Whole already: `frames`
    itself, no copy.
    With `frame_step` d > 1 window w samples frames w * s + t * d: the whole-window buffer has (n - 1) * s + (frames_per_clip - 1) *
    d + 1 frames, and of the frames behind F - 1 only the slots start + t * d, t >= len = ceil((F - start) / d), are written (with
    frame start + (t % len) * d); the slots between them are never read.  A last window whose sampled frames all exist (its span
    may still overrun the video) is whole: `frames[:that many]`, a view."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    F = frames.shape[0]
    n = n_windows(F, frames_per_clip, s, d)
    start, whole = (n - 1) * s, buffer_frames(n, frames_per_clip, s, d)
    length = min(frames_per_clip, -(-(F - start) // d))
    if length == frames_per_clip:
        return frames[:whole]
    out = torch.empty((whole,) + tuple(frames.shape[1:]), device=frames.device, dtype=frames.dtype)
    out[:F].copy_(frames)
    t = torch.arange(length, frames_per_clip, device=frames.device)
    out[start + t * d] = frames[start + (t % length) * d]
    return out


def _u8_stem_tables(pc: "PackedConv", form: str, frame_hw: Tuple[int, int], clip_thw: Tuple[int, int, int], mean: float, frame_step: int):
    """The tables of a uint8-frame stem for frames of (FH, FW) and clips of (T, crop, crop), cached on the conv (built on the
    current stream: callers that fork streams build them first, like the other lazily built tables).  `form` "u8": (gather table,
    border corrections); "u8_taps": those and the re-laid weights.  `frame_step`: the temporal term of the gather table is
    frame_step frames per tap -- part of the cache key."""
    key = (("taps",) if form == "u8_taps" else ()) + (tuple(frame_hw), tuple(clip_thw), float(mean), int(frame_step))
    cache = pc.__dict__.setdefault("_u8_tables", {})
    tabs = cache.get(key)
    if tabs is None:
        d = pc.desc(1, *clip_thw, True, 0, 1)
        lib = _lib.load()
        sizes = [C.c_int64() for _ in range(3 if form == "u8_taps" else 2)]
        check(getattr(lib, f"advhip_conv3d_{form}_table_sizes")(C.byref(d), *(C.byref(n) for n in sizes)), f"conv3d_{form}_table_sizes")
        dev = pc.w_packed.device
        tabs = tuple(torch.empty((n.value,), device=dev, dtype=torch.int32 if i == 0 else torch.float32) for i, n in enumerate(sizes))
        check(getattr(lib, f"advhip_conv3d_{form}_build_tables_sampled")(C.byref(d), frame_hw[0], frame_hw[1], int(frame_step), ptr(pc.w_packed),
                                                                         C.c_float(mean), *(ptr(t) for t in tabs), stream(dev)),
              f"conv3d_{form}_build_tables[{pc.name}]")
        cache[key] = tabs
    return tabs


def ensure_u8_taps_tables(pc: "PackedConv", frame_hw: Tuple[int, int], clip_thw: Tuple[int, int, int], mean: float = PIXEL_MEAN,
                          frame_step: int = 1):
    """(ktab, corr, weights) of the whole-pixel ("taps") uint8-frame stem: _u8_stem_tables."""
    return _u8_stem_tables(pc, "u8_taps", frame_hw, clip_thw, mean, frame_step)


def ensure_u8_tables(pc: "PackedConv", frame_hw: Tuple[int, int], clip_thw: Tuple[int, int, int], mean: float = PIXEL_MEAN,
                     frame_step: int = 1):
    """(ktab, corr) of the byte-gather uint8-frame stem: _u8_stem_tables."""
    return _u8_stem_tables(pc, "u8", frame_hw, clip_thw, mean, frame_step)


def conv3d_u8_tencrop_bn_relu_maxpool233(frames: torch.Tensor, pc: "PackedConv", first: int, count: int, frames_per_clip: int = 16,
                                         crop: int = 224, out: Optional[torch.Tensor] = None, mean: float = PIXEL_MEAN,
                                         std: float = PIXEL_STD, clip_stride: Optional[int] = None, crops=None,
                                         frame_step: Optional[int] = None) -> torch.Tensor:
    """The stem (conv1 + bn1 + relu + maxpool1, src/i3d.py:303-306) of crop-clips [first, first + count) of a video given as
    resized uint8 frames (F, FH, FW, 3): row = clip * 10 + crop (TenCrop order).  TenCrop, float conversion and
    (x - mean) / std happen in the conv's load stage (src/gtransforms.py:29-38,57-73, extract_features.py:83-89).
    `clip_stride` (default frames_per_clip): clip w = frames [w * clip_stride, w * clip_stride + frames_per_clip); the frames
    are whole windows, F = (n - 1) * clip_stride + frames_per_clip (pad_windows_u8 appends a short last window's LoopPad frames).
    `crops` (resolve_crops; default all ten): row = clip * len(crops) + j holds crop crops[j], bit for bit the ten-crop row of
    that (clip, crop); the set is a by-value argument of the same kernel.
    `frame_step` d (default 1): clip w = frames w * clip_stride + t * d, t in [0, frames_per_clip); clip_stride defaults to
    frames_per_clip * d, and the whole-window buffer has F = (n - 1) * clip_stride + (frames_per_clip - 1) * d + 1 frames
    (pad_windows_u8 with the same arguments).  Scalar set-up of the same kernel plus gather tables built for d."""
    require_gpu(frames)
    require_gpu(out, contiguous=False)
    s, crops, fstep = resolve_sampling(frames_per_clip, clip_stride, crops, frame_step)
    nc, packed = pack_crops(crops)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != pc.cin:
        raise ValueError(f"{pc.name}: expected uint8 (F,H,W,{pc.cin}) frames, got {frames.dtype} {tuple(frames.shape)}")
    F, FH, FW, _ = frames.shape
    n = buffer_windows(F, frames_per_clip, s, fstep)
    if n == 0 or buffer_frames(n, frames_per_clip, s, fstep) != F or FH < crop or FW < crop:
        raise ValueError(f"{pc.name}: {F} frames of {FH}x{FW} are not whole {frames_per_clip}-frame clips (stride {s}"
                         + (f", frame step {fstep}" if fstep != 1 else "") + f") of at least {crop}x{crop}")
    n *= nc
    if count <= 0 or first < 0 or first + count > n:
        raise ValueError(f"{pc.name}: crop-clips [{first}, {first + count}) outside the video's {n}")
    d = pc.desc(count, frames_per_clip, crop, crop, True, 0, 1)
    y, ws, need = _pool233_out(pc, d, f"clips of ({frames_per_clip},{crop},{crop})", out, frames.device)
    lib = _lib.load()
    if U8_STEM_FORM in ("taps", "planes") and pc.cin == 3 and pc.cout == 64:
        frames = with_slack(frames)
        ktab, corr, wt = ensure_u8_taps_tables(pc, (FH, FW), (frames_per_clip, crop, crop), mean, fstep)
        check(lib.advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_sampled_f32(C.byref(d), ptr(frames), F, FH, FW, s, fstep, nc, packed,
                                                                               readable_bytes(frames), first, ptr(wt), ptr(ktab), ptr(corr),
                                                                               ptr(pc.scale), ptr(pc.shift), C.c_float(std), ptr(y),
                                                                               batch_stride(y), ptr(ws), need, stream()),
              f"conv3d_u8_taps+pool233[{pc.name}]")
        return y
    ktab, corr = ensure_u8_tables(pc, (FH, FW), (frames_per_clip, crop, crop), mean, fstep)
    check(lib.advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32(C.byref(d), ptr(frames), F, FH, FW, s, fstep, nc, packed, first,
                                                                      ptr(pc.w_packed), ptr(ktab), ptr(corr), ptr(pc.scale), ptr(pc.shift),
                                                                      C.c_float(std), ptr(y), batch_stride(y), ptr(ws), need, stream()),
          f"conv3d_u8+pool233[{pc.name}]")
    return y


def conv3d_bn_act_maxpool211(x: torch.Tensor, pc: PackedConv, relu: bool = True, residual: Optional[torch.Tensor] = None,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """maxpool3d(act(conv3d(x) * scale + shift (+ residual)), (2,1,1), (2,1,1)) in one launch, for a 1x1x1 stride-1 conv
    (layer1's last conv3 + maxpool2, src/i3d.py:111-121, 309).  `residual`: un-pooled shape, contiguous."""
    require_gpu(x, out, contiguous=False)
    require_gpu(residual)
    if x.dim() != 5 or x.shape[1] != pc.cin:
        raise ValueError(f"{pc.name}: expected (B,{pc.cin},T,H,W), got {tuple(x.shape)}")
    B, _, T, H, W = x.shape
    if T < 2:
        raise ValueError(f"{pc.name}: T={T} smaller than the temporal pooling window")
    shape = (B, pc.cout, T // 2, H, W)
    y = out if out is not None else torch.empty(shape, device=x.device, dtype=torch.float32)
    if tuple(y.shape) != shape or y.dtype != torch.float32 or y.device != x.device:
        raise ValueError(f"{pc.name}: out {tuple(y.shape)} != {shape}")
    if residual is not None and tuple(residual.shape) != (B, pc.cout, T, H, W):
        raise ValueError(f"{pc.name}: residual {tuple(residual.shape)} != un-pooled output {(B, pc.cout, T, H, W)}")
    ktab = ensure_ktab(pc, (T, H, W))
    d = pc.desc(B, T, H, W, relu, 0, 1)
    check(_lib.load().advhip_conv3d_bn_act_maxpool211_f32(C.byref(d), ptr(x), batch_stride(x), ptr(pc.w_packed), ptr(ktab), ptr(pc.scale),
                                                          ptr(pc.shift), ptr(residual), ptr(y), batch_stride(y), stream()),
          f"conv3d+pool211[{pc.name}]")
    return y


def maxpool3d(x: torch.Tensor, kernel, stride, out: Optional[torch.Tensor] = None, padding=(0, 0, 0)) -> torch.Tensor:
    """`out`: optional destination, contiguous or a channel slice of a wider NCDHW tensor (un-padded pooling only)."""
    require_gpu(x)
    require_gpu(out, contiguous=False)
    B, Cc, T, H, W = x.shape
    k, s = _triple(kernel), _triple(stride)
    p = _triple(padding)
    if any(p):
        if out is not None:
            raise ValueError("maxpool3d: `out` is not supported together with padding")
        to, ho, wo = conv_out_dims((T, H, W), k, s, p)
        y = torch.empty((B, Cc, to, ho, wo), device=x.device, dtype=torch.float32)
        check(_lib.load().advhip_maxpool3d_padded_f32(ptr(x), ptr(y), B, Cc, T, H, W, *k, *s, *p, stream()), "maxpool3d_padded")
        return y
    to, ho, wo = conv_out_dims((T, H, W), k, s, (0, 0, 0))
    y = out if out is not None else torch.empty((B, Cc, to, ho, wo), device=x.device, dtype=torch.float32)
    if tuple(y.shape) != (B, Cc, to, ho, wo):
        raise ValueError(f"maxpool3d: out {tuple(y.shape)} != {(B, Cc, to, ho, wo)}")
    ybs = batch_stride(y)
    check(_lib.load().advhip_maxpool3d_strided_f32(ptr(x), ptr(y), 0 if ybs == Cc * to * ho * wo else ybs, B, Cc, T, H, W, *k, *s, stream()),
          "maxpool3d")
    return y


FUSE_AVGPOOL = os.environ.get("ADV_I3D_FUSE_AVGPOOL", "1") == "1"


def avgpool_fusable(pc: PackedConv, thw: Tuple[int, int, int]) -> bool:
    """conv3d_bn_act_avgpool takes this conv on (T,H,W) inputs (include/advhip.h: advhip_conv3d_epilogue.avgpool_out)."""
    return (pc.kernel == (1, 1, 1) and pc.stride == (1, 1, 1) and pc.padding == (0, 0, 0) and thw[0] * thw[1] * thw[2] <= 128
            and pc.cout % 64 == 0 and pc.cin % 32 == 0)


def conv3d_bn_act_avgpool(x: torch.Tensor, pc: PackedConv, relu: bool = True, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """global_avgpool(act(conv3d(x) * scale + shift (+ residual))) -> (B, Cout, 1, 1, 1) in ONE launch: the conv's own output is
    never written.  Bit for bit global_avgpool(conv3d_bn_act(...)) (src/i3d.py:111-121 + 314)."""
    require_gpu(x, residual)
    B, _, T, H, W = x.shape
    if x.shape[1] != pc.cin or not avgpool_fusable(pc, (T, H, W)):
        raise ValueError(f"{pc.name}: conv + mean in one launch needs a 1x1x1 stride-1 conv on <= 128 positions, got {tuple(x.shape)}")
    if residual is not None and tuple(residual.shape) != (B, pc.cout, T, H, W):
        raise ValueError(f"{pc.name}: residual {tuple(residual.shape)} != output {(B, pc.cout, T, H, W)}")
    y = torch.empty((B, pc.cout, 1, 1, 1), device=x.device, dtype=torch.float32)
    d = pc.desc(B, T, H, W, relu, _lib.ALGO_DMA2_BASE + _lib.ALGO_IGEMM_128x64, 1)
    ep = _lib.ConvEpilogue(None, None, None, None, None, None, 0, ptr(y))
    check(_lib.load().advhip_conv3d_bn_act_ex_f32(C.byref(d), ptr(x), 0, ptr(pc.w_packed), ptr(ensure_ktab(pc, (T, H, W))), ptr(pc.scale),
                                                  ptr(pc.shift), ptr(residual), None, 0, C.byref(ep), None, 0, stream()), f"conv3d+mean[{pc.name}]")
    return y


def global_avgpool(x: torch.Tensor) -> torch.Tensor:
    """(B,C,T,H,W) -> (B,C,1,1,1)"""
    require_gpu(x)
    B, Cc = x.shape[:2]
    n = x[0, 0].numel()
    y = torch.empty((B, Cc, 1, 1, 1), device=x.device, dtype=torch.float32)
    check(_lib.load().advhip_global_avgpool_f32(ptr(x), ptr(y), B * Cc, n, stream()), "global_avgpool")
    return y


def bgemm(a: torch.Tensor, b: torch.Tensor, *, alpha: float = 1.0, bias_m: Optional[torch.Tensor] = None,
          bias_n: Optional[torch.Tensor] = None, act: int = 0, residual: Optional[torch.Tensor] = None, beta: float = 1.0,
          ln: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i] = epi(alpha * a[i] @ b[i]) on the fp32 MFMA (include/advhip.h: advhip_bgemm_f32).  a: (batch, M, K), b: (batch, K, N)
    -- any views whose last two dims have one unit stride each (transposes and channel slices included; batch stride 0 =
    broadcast); 2-D operands are one batch.  `ln` = (u[M], mu[batch*N], rs[batch*N]): the LayerNorm fold of the header.
    `act`: 0 none, 1 ReLU, 2 GELU(erf).  `residual`: like out."""
    if a.dim() == 2:
        a = a.unsqueeze(0)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    require_gpu(a, b, out, residual, contiguous=False)
    require_gpu(bias_m, bias_n)
    batch = max(a.shape[0], b.shape[0])
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != b.shape[1] or a.shape[0] not in (1, batch) or b.shape[0] not in (1, batch):
        raise ValueError(f"bgemm: incompatible operands {tuple(a.shape)} x {tuple(b.shape)}")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise _lib.HipExtensionError("bgemm computes in fp32")
    M, K, N = a.shape[1], a.shape[2], b.shape[2]
    y = out if out is not None else torch.empty((batch, M, N), device=a.device, dtype=torch.float32)
    if y.dim() == 2:
        y = y.unsqueeze(0)
    if tuple(y.shape) != (batch, M, N) or y.dtype != torch.float32:
        raise ValueError(f"bgemm: out {tuple(y.shape)} != {(batch, M, N)}")
    if residual is not None:
        if residual.dim() == 2:
            residual = residual.unsqueeze(0)
        if tuple(residual.shape) != (batch, M, N) or residual.stride() != y.stride():
            raise ValueError("bgemm: residual must have out's shape and strides")

    def strides(t, nb):
        sb = t.stride(0) if t.shape[0] == nb and nb > 1 else 0
        return sb, t.stride(1), t.stride(2)

    sa, sb_, sc = strides(a, batch), strides(b, batch), strides(y, batch)
    if M > 1 and K > 1 and 1 not in sa[1:] or N > 1 and K > 1 and 1 not in sb_[1:]:
        raise ValueError(f"bgemm: each operand needs a unit stride in its last two dims (got {a.stride()}, {b.stride()})")
    # a size-1 dim's stride is arbitrary: give the kernel a consistent unit stride
    sa = (sa[0], 1 if M == 1 and sa[2] != 1 else sa[1], 1 if K == 1 and sa[1] != 1 else sa[2])
    sb_ = (sb_[0], 1 if K == 1 and sb_[2] != 1 else sb_[1], 1 if N == 1 and sb_[1] != 1 else sb_[2])
    d = _lib.GemmDesc(M, N, K, batch, *sa, *sb_, *sc, float(alpha), float(beta), int(act), ptr(bias_m), ptr(bias_n),
                      ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None, ptr(ln[2]) if ln else None, ptr(residual))
    if ln is not None:
        require_gpu(*ln)
        if ln[0].numel() != M or ln[1].numel() != batch * N or ln[2].numel() != batch * N:
            raise ValueError("bgemm: LayerNorm fold vectors must be u[M], mu[batch*N], rs[batch*N]")
    check(_lib.load().advhip_bgemm_f32(C.byref(d), ptr(a), ptr(b), ptr(y), stream()), "bgemm")
    return y if out is None or out.dim() == 3 else out


def softmax_rows(x: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """softmax(x * scale) over the last (contiguous) dim, one wavefront per row; out may be x."""
    require_gpu(x, out)
    y = out if out is not None else torch.empty_like(x)
    n = x.shape[-1]
    check(_lib.load().advhip_softmax_rows_f32(ptr(x), ptr(y), x.numel() // n, n, C.c_float(scale), stream()), "softmax_rows")
    return y


# (M, N) -> (tile id, K slices) of advhip_gemm_nt_rowsum_f32 at K = 10 240, measured on one MI355X (tools/tune_gemm_nt.py,
# profiles/r03_gemm_nt_tune.txt): the weight-gradient shapes of the MGFN scorer at its training batch.  Other shapes: heuristic.
GEMM_NT_TUNED: Dict[Tuple[int, int, int], Tuple[int, int]] = {
    (4096, 1024, 10240): (2, 2), (1024, 4096, 10240): (3, 3), (1024, 1024, 10240): (1, 4), (1024, 3072, 10240): (3, 4),
}


def gemm_nt_choice(M: int, N: int, K: int) -> Tuple[int, int]:
    hit = GEMM_NT_TUNED.get((M, N, K))
    if hit is not None:
        return hit
    tiles = -(-M // 64) * -(-N // 64)
    if tiles < 64:  # few output tiles (the 64- / 128-channel layers): 16 K slices to slabs measured best for every such shape
        return 1, max(1, min(NT_SMALL_SPLITS, K // 256))  # (profiles/r03_gemm_nt_tune.txt: 32-35 us vs 36-58 for 40)
    return 0, max(1, min(64, 1024 // max(tiles, 1), K // 256))


NT_SMALL_SPLITS = 16


def gemm_nt_is_small(M: int, N: int) -> bool:
    """gemm_nt takes the slab + one-reduce form for this output (a handful of 64 x 64 tiles): what gemm_nt_group batches."""
    return -(-M // 64) * -(-N // 64) < 64


def gemm_nt_group(items):
    """[(a (M,K), b (N,K), rowsum: bool), ...] -> [(a @ b^T, row sums of a or None), ...]: every small product of the list in ONE
    launch (K slices to one slab matrix) + ONE reduce launch (include/advhip.h: advhip_gemm_nt_group_slabs_f32) -- bit for bit what
    gemm_nt returns for each of them alone.  All items contract over the same K."""
    if not items:
        return []
    K = items[0][0].shape[1]
    dev = items[0][0].device
    offs, total = [], 0
    for a, b, rs in items:
        require_gpu(a, b, contiguous=False)
        if a.dim() != 2 or b.dim() != 2 or a.shape[1] != K or b.shape[1] != K or a.stride(1) != 1 or b.stride(1) != 1:
            raise ValueError(f"gemm_nt_group: need (M,K) and (N,K) operands over one K = {K} with unit inner stride, got {tuple(a.shape)} / {tuple(b.shape)}")
        offs.append(total)
        total += -(-(a.shape[0] * b.shape[0] + (a.shape[0] if rs else 0)) // 64) * 64
    splits = max(1, min(NT_SMALL_SPLITS, K // 256))
    slabs = torch.empty((splits, total), device=dev, dtype=torch.float32)
    res = torch.empty((total,), device=dev, dtype=torch.float32)
    arr = (_lib.NtItem * len(items))()
    base = slabs.data_ptr()
    for it, (a, b, rs), off in zip(arr, items, offs):
        M, N = a.shape[0], b.shape[0]
        it.A, it.B, it.C = a.data_ptr(), b.data_ptr(), base + off * 4
        it.rowsum = base + (off + M * N) * 4 if rs else None
        it.M, it.N, it.lda, it.ldb = M, N, a.stride(0), b.stride(0)
    lib = _lib.load()
    check(lib.advhip_gemm_nt_group_slabs_f32(arr, len(items), K, splits, total, stream(dev)), "gemm_nt_group")
    check(lib.advhip_sum_slabs_f32(ptr(slabs), ptr(res), total, splits, total, stream(dev)), "sum_slabs")
    out = []
    for (a, b, rs), off in zip(items, offs):
        M, N = a.shape[0], b.shape[0]
        out.append((res[off : off + M * N].view(M, N), res[off + M * N : off + M * N + M] if rs else None))
    return out


def gemm_nt(a: torch.Tensor, b: torch.Tensor, splits: int = 0, rowsum: bool = False, tile: int = 0,
            reduce_in_kernel: Optional[bool] = None):
    """a (M, K) @ b (N, K)^T -> (M, N) for two k-contiguous operands (row pitch = stride(0)); K % 16 == 0.  The weight
    gradient of a GEMM-shaped layer with (channel, position) activations (include/advhip.h: advhip_gemm_nt_rowsum_f32).
    `splits`: K slices (0 = the measured / heuristic choice), summed inside the launch by the last-arriving workgroup of
    every tile (slice order: run-to-run bit-identical).  `rowsum`: also return the row sums of `a` (M,) -- the bias gradient
    of the same layer, out of the same launch."""
    require_gpu(a, b, contiguous=False)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1] or a.stride(1) != 1 or b.stride(1) != 1:
        raise ValueError(f"gemm_nt: need (M,K) and (N,K) with unit inner stride, got {tuple(a.shape)} {a.stride()} / {tuple(b.shape)} {b.stride()}")
    M, K = a.shape
    N = b.shape[0]
    if splits <= 0:
        t, splits = gemm_nt_choice(M, N, K)
        tile = tile or t
    lib = _lib.load()
    if splits > 1 and reduce_in_kernel is None:
        reduce_in_kernel = -(-M // 64) * -(-N // 64) >= 64
    if splits > 1 and not reduce_in_kernel:
        # few output tiles: slices to slabs, product and row sums reduced by ONE further launch (the in-kernel form would
        # leave the whole sum to the last arriver of each of a handful of tiles)
        n = M * N + (M if rowsum else 0)
        slabs = torch.empty((splits, n), device=a.device, dtype=torch.float32)
        res = torch.empty((n,), device=a.device, dtype=torch.float32)
        check(lib.advhip_gemm_nt_slabs_f32(ptr(a), ptr(b), ptr(slabs), M, N, K, a.stride(0), b.stride(0), splits, tile, int(rowsum), stream(a)),
              "gemm_nt_slabs")
        check(lib.advhip_sum_slabs_f32(ptr(slabs), ptr(res), n, splits, n, stream(a)), "sum_slabs")
        out = res[: M * N].view(M, N)
        return (out, res[M * N :]) if rowsum else out
    out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    rs = torch.empty((M,), device=a.device, dtype=torch.float32) if rowsum else None
    need = lib.advhip_gemm_nt_workspace_bytes(M, N, splits, tile) if splits > 1 else 0
    ws = zeroed_workspace(a.device, need)  # (arrival counters: zero on entry, left zero by the launch)
    check(lib.advhip_gemm_nt_reduced_f32(ptr(a), ptr(b), ptr(out), ptr(rs), M, N, K, a.stride(0), b.stride(0), N, splits, tile, ptr(ws), need,
                                         stream(a)), "gemm_nt")
    return (out, rs) if rowsum else out
