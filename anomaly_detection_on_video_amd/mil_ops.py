"""Autograd bindings of the MIL head / loss HIP kernels (csrc/mil.hip, csrc/loss.hip).

Three differentiable ops, each one C-ABI call forward and one backward:

    mil_magnitude(features, scores, bs, ncrops)          -> mag (bs,T), sc (bs,T)
    mil_topk_select(mag, keep, sc, features, ncrops, k)  -> idx (n,k), sel (ncrops*n,k,F), score (n,1)
    mgfn_loss(sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels) -> total, terms(8)

CUDA tensors only; no fallback.  Reference semantics: modeling_mgfn.py:302-374, loss/*.py.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream
from .ops import resolve_clip_stride, resolve_frame_step
from .ops import PIXEL_MEAN, PIXEL_STD, normalize_permute_u8, tencrop_normalize_u8  # noqa: F401  (their callers' name for them)


class _MilMagnitude(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features: torch.Tensor, scores: torch.Tensor, bs: int, ncrops: int):
        ctx.set_materialize_grads(False)  # (unused output gradients arrive as None, not as zero-filled tensors)
        features = features.contiguous()
        scores = scores.contiguous()
        require_gpu(features, scores)
        rows, T, F = features.shape
        if rows != bs * ncrops or scores.numel() != rows * T:
            raise ValueError(f"mil_magnitude: features {tuple(features.shape)} / scores {tuple(scores.shape)} vs bs={bs} ncrops={ncrops}")
        mag = torch.empty((bs, T), device=features.device, dtype=torch.float32)
        sc = torch.empty_like(mag)
        check(_lib.load().advhip_mil_magnitude_f32(ptr(features), ptr(scores), ptr(mag), ptr(sc), bs, ncrops, T, F, stream()), "mil_magnitude")
        ctx.save_for_backward(features)
        ctx.dims = (bs, ncrops, T, F, scores.shape)
        ctx.mark_non_differentiable(mag)  # only feeds topk indices (modeling_mgfn.py:345-346)
        return mag, sc

    @staticmethod
    def backward(ctx, _d_mag, d_sc):
        (features,) = ctx.saved_tensors
        bs, ncrops, T, F, sshape = ctx.dims
        d_scores = None
        if d_sc is not None and ctx.needs_input_grad[1]:
            d_sc = d_sc.contiguous()
            d_scores = torch.zeros((bs * ncrops, T), device=features.device, dtype=torch.float32)
            check(_lib.load().advhip_mil_magnitude_bwd_f32(ptr(features), None, ptr(d_sc), None, ptr(d_scores), bs, ncrops, T, F, stream()), "mil_magnitude_bwd")
            d_scores = d_scores.view(sshape)
        return None, d_scores, None, None


class _MilTopkSelect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mag, keep, sc, features, ncrops: int, k: int):
        ctx.set_materialize_grads(False)  # (unused output gradients arrive as None, not as zero-filled tensors)
        mag, sc, features = mag.contiguous(), sc.contiguous(), features.contiguous()
        keep = None if keep is None else keep.contiguous()
        require_gpu(mag, keep, sc, features)
        n, T = mag.shape
        rows, T2, F = features.shape
        if rows != n * ncrops or T2 != T or sc.shape != mag.shape or (keep is not None and keep.shape != mag.shape):
            raise ValueError("mil_topk_select: inconsistent shapes")
        dev = mag.device
        idx = torch.empty((n, k), device=dev, dtype=torch.int64)
        sel = torch.empty((ncrops * n, k, F), device=dev, dtype=torch.float32)
        score = torch.empty((n,), device=dev, dtype=torch.float32)
        check(_lib.load().advhip_mil_topk_select_f32(ptr(mag), ptr(keep), ptr(sc), ptr(features), ptr(idx), ptr(sel), ptr(score),
                                                     n, ncrops, T, F, k, stream()), "mil_topk_select")
        ctx.save_for_backward(idx)
        ctx.dims = (n, ncrops, T, F, k)
        ctx.mark_non_differentiable(idx)
        return idx, sel, score.view(n, 1)

    @staticmethod
    def backward(ctx, _d_idx, d_sel, d_score):
        (idx,) = ctx.saved_tensors
        n, ncrops, T, F, k = ctx.dims
        dev = idx.device
        d_feat = d_sc = None
        want_f, want_s = ctx.needs_input_grad[3], ctx.needs_input_grad[2]
        if want_f:
            d_feat = torch.zeros((n * ncrops, T, F), device=dev, dtype=torch.float32)
        if want_s:
            d_sc = torch.zeros((n, T), device=dev, dtype=torch.float32)
        ds = d_sel.contiguous() if (d_sel is not None and want_f) else None
        dscore = d_score.contiguous() if (d_score is not None and want_s) else None
        if ds is not None or dscore is not None:
            check(_lib.load().advhip_mil_topk_select_bwd_f32(ptr(idx), ptr(ds), ptr(dscore), ptr(d_feat), ptr(d_sc), n, ncrops, T, F, k, stream()),
                  "mil_topk_select_bwd")
        return None, None, d_sc, d_feat, None, None


class _MilTopkSelectSplit(torch.autograd.Function):
    """mil_topk_select of the normal half (videos [0, h)) and of the abnormal half (videos [h, 2h)) of one batch
    (modeling_mgfn.py:324-332, 364-372) as ONE autograd node: the two halves' feature gradients are scattered into one
    zero-filled (bs*ncrops, T, F) buffer -- two separate nodes on slices of `features` make autograd zero-fill and add two
    full-size tensors (five launches over 42 MB at the training batch)."""

    @staticmethod
    def forward(ctx, mag, keep_a, keep_n, sc, features, ncrops: int, k: int):
        ctx.set_materialize_grads(False)  # (unused output gradients arrive as None, not as zero-filled tensors)
        mag, sc, features = mag.contiguous(), sc.contiguous(), features.contiguous()
        require_gpu(mag, keep_a, keep_n, sc, features)
        bs, T = mag.shape
        rows, T2, F = features.shape
        h = bs // 2
        if bs != 2 * h or rows != bs * ncrops or T2 != T or sc.shape != mag.shape:
            raise ValueError("mil_topk_select_split: inconsistent shapes")
        dev = mag.device
        lib = _lib.load()
        outs = []
        for half, keep in ((1, keep_a), (0, keep_n)):  # abnormal first, as the reference calls them
            keep = None if keep is None else keep.contiguous()
            if keep is not None and tuple(keep.shape) != (h, T):
                raise ValueError("mil_topk_select_split: keep mask must be (bs/2, T)")
            idx = torch.empty((h, k), device=dev, dtype=torch.int64)
            sel = torch.empty((ncrops * h, k, F), device=dev, dtype=torch.float32)
            score = torch.empty((h,), device=dev, dtype=torch.float32)
            lo = half * h
            check(lib.advhip_mil_topk_select_f32(ptr(mag[lo : lo + h]), ptr(keep), ptr(sc[lo : lo + h]), ptr(features[lo * ncrops : (lo + h) * ncrops]),
                                                 ptr(idx), ptr(sel), ptr(score), h, ncrops, T, F, k, stream()), "mil_topk_select")
            outs += [idx, sel, score.view(h, 1)]
        ctx.save_for_backward(outs[0], outs[3])
        ctx.dims = (h, ncrops, T, F, k)
        ctx.mark_non_differentiable(outs[0], outs[3])
        return tuple(outs)  # idx_a, sel_a, score_a, idx_n, sel_n, score_n

    @staticmethod
    def backward(ctx, _dia, d_sel_a, d_score_a, _din, d_sel_n, d_score_n):
        idx_a, idx_n = ctx.saved_tensors
        h, ncrops, T, F, k = ctx.dims
        dev = idx_a.device
        want_f, want_s = ctx.needs_input_grad[4], ctx.needs_input_grad[3]
        d_feat = torch.zeros((2 * h * ncrops, T, F), device=dev, dtype=torch.float32) if want_f else None
        d_sc = torch.zeros((2 * h, T), device=dev, dtype=torch.float32) if want_s else None
        lib = _lib.load()
        for half, idx, d_sel, d_score in ((1, idx_a, d_sel_a, d_score_a), (0, idx_n, d_sel_n, d_score_n)):
            ds = d_sel.contiguous() if (d_sel is not None and want_f) else None
            dscore = d_score.contiguous() if (d_score is not None and want_s) else None
            if ds is None and dscore is None:
                continue
            lo = half * h
            check(lib.advhip_mil_topk_select_bwd_f32(ptr(idx), ptr(ds), ptr(dscore), ptr(d_feat[lo * ncrops : (lo + h) * ncrops]) if want_f else None,
                                                     ptr(d_sc[lo : lo + h]) if want_s else None, h, ncrops, T, F, k, stream()), "mil_topk_select_bwd")
        return None, None, None, d_sc, d_feat, None, None


def mil_topk_select_split(mag, keep_a: Optional[torch.Tensor], keep_n: Optional[torch.Tensor], sc, features, ncrops: int, k: int):
    """-> (idx_a, sel_a, score_a, idx_n, sel_n, score_n): videos [bs/2, bs) are the abnormal half, [0, bs/2) the normal one."""
    return _MilTopkSelectSplit.apply(mag, keep_a, keep_n, sc, features, ncrops, k)


class _MgfnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels, ncrops: int):
        ctx.set_materialize_grads(False)  # (unused output gradients arrive as None, not as zero-filled tensors)
        args = [t.contiguous().float() for t in (sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels)]
        require_gpu(*args)
        sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels = args
        bs, T = sc.shape[0], sc.shape[1]
        R, k, F = a_feat.shape
        n = bs // 2
        if R != n * ncrops or n_feat.shape != a_feat.shape or abn_score.numel() != n or nor_score.numel() != n:
            raise ValueError("mgfn_loss: inconsistent shapes")
        if abn_labels.numel() != n or nor_labels.numel() != n:
            raise ValueError("mgfn_loss: need bs/2 labels per class")
        lib = _lib.load()
        ws = torch.empty((lib.advhip_mgfn_loss_ws_floats(n, ncrops, k),), device=sc.device, dtype=torch.float32)
        out = torch.empty((8,), device=sc.device, dtype=torch.float32)
        check(lib.advhip_mgfn_loss_fwd_f32(ptr(sc), ptr(abn_score), ptr(nor_score), ptr(a_feat), ptr(n_feat), ptr(abn_labels), ptr(nor_labels),
                                           ptr(ws), ptr(out), bs, T, ncrops, k, F, stream()), "mgfn_loss_fwd")
        ctx.save_for_backward(sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels, ws)
        ctx.dims = (bs, T, ncrops, k, F)
        terms = out.detach().clone()
        ctx.mark_non_differentiable(terms)
        return out[0].clone(), terms

    @staticmethod
    def backward(ctx, d_loss, _d_terms):
        sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels, ws = ctx.saved_tensors
        bs, T, ncrops, k, F = ctx.dims
        d_loss = d_loss.contiguous().float().reshape(1)
        d_sc = torch.empty_like(sc)
        d_abn = torch.empty_like(abn_score)
        d_nor = torch.empty_like(nor_score)
        d_a = torch.empty_like(a_feat)
        d_n = torch.empty_like(n_feat)
        check(_lib.load().advhip_mgfn_loss_bwd_f32(ptr(d_loss), ptr(sc), ptr(abn_score), ptr(nor_score), ptr(a_feat), ptr(n_feat), ptr(abn_labels),
                                                   ptr(nor_labels), ptr(ws), ptr(d_sc), ptr(d_abn), ptr(d_nor), ptr(d_a), ptr(d_n),
                                                   bs, T, ncrops, k, F, stream()), "mgfn_loss_bwd")
        return d_sc, d_abn, d_nor, d_a, d_n, None, None, None


def mil_magnitude(features: torch.Tensor, scores: torch.Tensor, bs: int, ncrops: int) -> Tuple[torch.Tensor, torch.Tensor]:
    return _MilMagnitude.apply(features, scores, bs, ncrops)


def mil_topk_select(mag, keep: Optional[torch.Tensor], sc, features, ncrops: int, k: int):
    return _MilTopkSelect.apply(mag, keep, sc, features, ncrops, k)


def _device_vec(t, dtype, n: int, what: str) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.dim() == 1 and t.numel() == n and t.is_contiguous()):
        raise _lib.HipExtensionError(f"{what}: expected a contiguous {dtype} device vector of {n}")
    return t


def crop_mean_scatter(scores: torch.Tensor, lens: torch.Tensor, dst_offsets: torch.Tensor, dst: torch.Tensor, n_videos: int, ncrops: int) -> torch.Tensor:
    """The crop mean of a padded batch's per-crop scores (n_videos * ncrops, Tmax) -- mil_magnitude's `sc`, bit for bit -- for the
    lens[v] real clips of every video, written at dst[dst_offsets[v] + t] of a flat fp32 buffer.  lens (int32) and dst_offsets
    (int64) are device vectors whose values the caller has validated: nothing is read back.  No autograd."""
    require_gpu(scores, dst)
    if scores.dtype != torch.float32 or dst.dtype != torch.float32 or scores.numel() % (n_videos * ncrops) or scores.numel() == 0:
        raise _lib.HipExtensionError(f"crop_mean_scatter: scores {scores.dtype} {tuple(scores.shape)} for {n_videos} videos x {ncrops} crops")
    tmax = scores.numel() // (n_videos * ncrops)
    check(_lib.load().advhip_crop_mean_scatter_f32(ptr(scores), ptr(_device_vec(lens, torch.int32, n_videos, "crop_mean_scatter lens")),
                                                   ptr(_device_vec(dst_offsets, torch.int64, n_videos, "crop_mean_scatter dst_offsets")), ptr(dst),
                                                   n_videos, ncrops, tmax, stream()), "crop_mean_scatter")
    return dst


def pack_padded(store: torch.Tensor, src_offsets: torch.Tensor, lens: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """One launch fills a padded batch dst (n_videos, ncrops, Tmax, width): video v, stored (ncrops, lens[v], width) at element
    src_offsets[v] of the flat fp32 `store`, goes to dst[v, :, :lens[v]]; the rows behind stay as they are.  src_offsets (int64) and
    lens (int32) are device vectors whose values the caller has validated against the store and Tmax."""
    require_gpu(store, dst)
    if store.dtype != torch.float32 or dst.dtype != torch.float32 or dst.dim() != 4:
        raise _lib.HipExtensionError(f"pack_padded: fp32 store and (n_videos, ncrops, Tmax, width) fp32 dst, got {store.dtype} and {dst.dtype} {tuple(dst.shape)}")
    n, ncrops, tmax, width = dst.shape
    check(_lib.load().advhip_pack_padded_f32(ptr(store), ptr(_device_vec(src_offsets, torch.int64, n, "pack_padded src_offsets")),
                                             ptr(_device_vec(lens, torch.int32, n, "pack_padded lens")), ptr(dst), n, ncrops, tmax, width, stream()),
          "pack_padded")
    return dst


def _live_arg(t, dtype, shape, what: str, name: str, dev=None) -> torch.Tensor:
    """One argument of the live-scoring launches: a contiguous `dtype` tensor on the GPU (on `dev`, the device of the arguments
    before it) of `shape`, where None stands for any extent."""
    if (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and (dev is None or t.device == dev) and t.dim() == len(shape) and t.numel() > 0
            and all(s is None or s == d for s, d in zip(shape, t.shape)) and t.is_contiguous()):
        return t
    err = _lib.HipExtensionError  # which of them it was, in the order a caller would fix them
    want = "(" + ", ".join("*" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"
    if not torch.is_tensor(t):
        raise err(f"{what}: {name} must be a {dtype} tensor {want} on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise err(f"{what}: {name} is on '{t.device}': this op runs only as a HIP kernel on the GPU (there is no CPU fallback)")
    if dev is not None and t.device != dev:
        raise err(f"{what}: {name} is on {t.device}, the arguments before it are on {dev}")
    if t.dtype != dtype:
        raise err(f"{what}: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous() and t.dim() == len(shape) and all(s is None or s == d for s, d in zip(shape, t.shape)):
        raise err(f"{what}: {name} must be contiguous")
    raise err(f"{what}: {name} must be {want}, got {tuple(t.shape)}")


def ring_push(feats: torch.Tensor, cam_ids: torch.Tensor, ring: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """One new clip for each of n distinct cameras into their rings (include/advhip.h: live scoring): feats (n, ncrops, C) fp32,
    cam_ids int32 (n,), ring (n_cam, ncrops, W, C + 1) fp32, counts int64 (n_cam,), all on the device.  Camera c = cam_ids[i]
    gets ring[c, :, counts[c] % W, :C] = feats[i] and, in the last channel, the clips' L2 magnitudes with numpy's bits
    (`add_magnitude_np`'s rule, C <= 8192); then counts[c] += 1.  An id outside [0, n_cam) writes nothing; the ids' values are
    the caller's (nothing is read back): the same id twice is an error this wrapper cannot see.  Two launches, no autograd."""
    what = "ring_push"
    ring = _live_arg(ring, torch.float32, (None, None, None, None), what, "ring")
    n_cam, ncrops, W, C1 = ring.shape
    if C1 < 2:
        raise _lib.HipExtensionError(f"{what}: ring must be (n_cam, ncrops, W, C + 1) with C >= 1, got {tuple(ring.shape)}")
    feats = _live_arg(feats, torch.float32, (None, ncrops, C1 - 1), what, "feats", ring.device)
    cam_ids = _live_arg(cam_ids, torch.int32, (feats.shape[0],), what, "cam_ids", ring.device)
    counts = _live_arg(counts, torch.int64, (n_cam,), what, "counts", ring.device)
    require_gpu(ring)  # (the current device)
    check(_lib.load().advhip_ring_push_f32(ptr(feats), ptr(cam_ids), ptr(ring), ptr(counts), feats.shape[0], n_cam, ncrops, W, C1 - 1, stream()), what)
    return ring


def ring_windows(ring: torch.Tensor, counts: torch.Tensor, cam_ids: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """The windows of the listed cameras as a padded batch, one launch: dst (nb, ncrops, Tmax, C + 1) fp32, cam_ids int32 (nb,);
    dst[v, :, t] for t < len = min(counts[c], W, Tmax), c = cam_ids[v], is the camera's last len clips, oldest first (entry t in
    slot (counts[c] - len + t) % W); the rows behind stay as they are (`pack_padded`'s contract), a camera at count 0 writes
    nothing.  A copy of bits.  No autograd."""
    what = "ring_windows"
    ring = _live_arg(ring, torch.float32, (None, None, None, None), what, "ring")
    n_cam, ncrops, W, C1 = ring.shape
    counts = _live_arg(counts, torch.int64, (n_cam,), what, "counts", ring.device)
    dst = _live_arg(dst, torch.float32, (None, ncrops, None, C1), what, "dst", ring.device)
    cam_ids = _live_arg(cam_ids, torch.int32, (dst.shape[0],), what, "cam_ids", ring.device)
    require_gpu(ring)
    check(_lib.load().advhip_ring_windows_f32(ptr(ring), ptr(counts), ptr(cam_ids), ptr(dst), dst.shape[0], n_cam, ncrops, W, dst.shape[2], C1, stream()), what)
    return dst


def crop_mean_last(scores: torch.Tensor, lens: torch.Tensor, cam_ids: torch.Tensor, latest: torch.Tensor, ncrops: int) -> torch.Tensor:
    """latest[cam_ids[v]] = the crop mean of the per-crop scores (nb * ncrops, Tmax[, 1]) at clip lens[v] - 1 of listed camera v --
    `crop_mean_scatter`'s bits at the newest clip.  lens and cam_ids are device int32 (nb,) vectors whose values the caller has
    validated (1 .. Tmax; distinct indices of `latest`); nothing else of latest (fp32, one entry per camera) is written."""
    what = "crop_mean_last"
    lens = _live_arg(lens, torch.int32, (None,), what, "lens")
    nb = lens.shape[0]
    if isinstance(ncrops, bool) or int(ncrops) != ncrops or ncrops < 1:
        raise _lib.HipExtensionError(f"{what}: ncrops {ncrops!r} is not a positive integer")
    if not torch.is_tensor(scores) or scores.numel() == 0 or scores.numel() % (nb * int(ncrops)) or scores.dim() < 2 or scores.shape[0] != nb * int(ncrops):
        raise _lib.HipExtensionError(f"{what}: scores must be ({nb * int(ncrops)}, Tmax) for {nb} cameras x {ncrops} crops, got "
                                     f"{tuple(getattr(scores, 'shape', ()))}")
    tmax = scores.numel() // (nb * int(ncrops))
    scores = _live_arg(scores, torch.float32, (nb * int(ncrops), tmax) + (1,) * (scores.dim() - 2), what, "scores", lens.device)
    cam_ids = _live_arg(cam_ids, torch.int32, (nb,), what, "cam_ids", lens.device)
    latest = _live_arg(latest, torch.float32, (None,), what, "latest", lens.device)
    require_gpu(scores)
    check(_lib.load().advhip_crop_mean_last_f32(ptr(scores), ptr(lens), ptr(cam_ids), ptr(latest), nb, int(ncrops), tmax, stream()), what)
    return latest


FRAME_RING_CHUNK = 1024  # elements of the access width (16, 4 or 1 bytes) one workgroup of the two launches below copies (csrc/live.hip: FRAME_CHUNK)


def _frame_ring(ring, what: str):
    """(ring, n_cam, R, frame_bytes) of a frame ring: uint8 (n_cam, R, ...) with any trailing dims (a frame is what lies behind R)."""
    if not torch.is_tensor(ring) or ring.dim() < 3:
        raise _lib.HipExtensionError(f"{what}: ring must be a torch.uint8 tensor (n_cam, R, frame_bytes) or (n_cam, R, FH, FW, 3) on the GPU, got "
                                     f"{tuple(getattr(ring, 'shape', ())) or type(ring).__name__}")
    ring = _live_arg(ring, torch.uint8, (None,) * ring.dim(), what, "ring")
    n_cam, R = ring.shape[:2]
    return ring, n_cam, R, ring.numel() // (n_cam * R)


def frame_ring_push(frames: torch.Tensor, cam_ids: torch.Tensor, ring: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """One new frame for each of n distinct cameras into their frame rings (include/advhip.h: live frames): ring uint8 (n_cam, R,
    frame_bytes) -- or (n_cam, R, FH, FW, 3), a frame is what lies behind R --, frames uint8 (n,) + the ring's frame shape, cam_ids
    int32 (n,), counts int64 (n_cam,), all on the device.  Camera c = cam_ids[i] gets ring[c, counts[c] % R] = frames[i]; then
    counts[c] += 1.  An id outside [0, n_cam) writes nothing; the same id twice is an error this wrapper cannot see.  A copy of
    bits by 16-, 4- or 1-byte accesses, whichever the pointers and the frame size allow.  Two launches, no autograd."""
    what = "frame_ring_push"
    ring, n_cam, R, fb = _frame_ring(ring, what)
    frames = _live_arg(frames, torch.uint8, (None,) + tuple(ring.shape[2:]), what, "frames", ring.device)
    cam_ids = _live_arg(cam_ids, torch.int32, (frames.shape[0],), what, "cam_ids", ring.device)
    counts = _live_arg(counts, torch.int64, (n_cam,), what, "counts", ring.device)
    require_gpu(ring)  # (the current device)
    check(_lib.load().advhip_frame_ring_push_u8(ptr(frames), ptr(cam_ids), ptr(ring), ptr(counts), frames.shape[0], n_cam, R, fb, stream()), what)
    return ring


def frame_ring_windows(ring: torch.Tensor, counts: torch.Tensor, cam_ids: torch.Tensor, dst: torch.Tensor, frames_per_clip: int,
                       frame_step: int) -> torch.Tensor:
    """The newest windows of the nb listed cameras as back-to-back clips, one launch: dst uint8 (nb * frames_per_clip,) + the ring's
    frame shape, cam_ids int32 (nb,); rows [v * fpc, (v + 1) * fpc) are entries t = 0 .. fpc - 1 of camera c = cam_ids[v], entry t
    from slot (counts[c] + t * frame_step) % R, oldest first (R = frames_per_clip * frame_step, anything else is refused).  The rows
    of a camera below R frames, or of an id outside [0, n_cam), stay as they are.  A copy of bits.  No autograd."""
    what = "frame_ring_windows"
    ring, n_cam, R, fb = _frame_ring(ring, what)
    for name, v in (("frames_per_clip", frames_per_clip), ("frame_step", frame_step)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise _lib.HipExtensionError(f"{what}: {name} {v!r} is not a positive integer")
    counts = _live_arg(counts, torch.int64, (n_cam,), what, "counts", ring.device)
    cam_ids = _live_arg(cam_ids, torch.int32, (None,), what, "cam_ids", ring.device)
    dst = _live_arg(dst, torch.uint8, (cam_ids.shape[0] * frames_per_clip,) + tuple(ring.shape[2:]), what, "dst", ring.device)
    require_gpu(ring)
    check(_lib.load().advhip_frame_ring_windows_u8(ptr(ring), ptr(counts), ptr(cam_ids), ptr(dst), cam_ids.shape[0], n_cam, R, fb, frames_per_clip,
                                                   frame_step, stream()), what)
    return dst


GATE_STATE_INIT = (-1, 0, -1, 0)  # a camera's state row {still, epoch, changed, peak} before its first frame (include/advhip.h: motion gate)


def frame_gate_scratch(n_cam: int, frame_bytes: int) -> int:
    """int32 entries of `frame_gate_update`'s scratch: one per camera and chunk of a frame at single-byte accesses."""
    return int(n_cam) * ((int(frame_bytes) + FRAME_RING_CHUNK - 1) // FRAME_RING_CHUNK)


def frame_gate_update(frames: torch.Tensor, cam_ids: torch.Tensor, anchor: torch.Tensor, state: torch.Tensor, scratch: torch.Tensor,
                      pixel_delta: int, limit: int) -> torch.Tensor:
    """The motion gate's update for one new frame of each of n distinct cameras (include/advhip.h: live frames: motion gate):
    anchor uint8 (n_cam, frame_bytes) -- or (n_cam, FH, FW, 3), a frame is what lies behind n_cam --, frames uint8 (n,) + the
    anchor's frame shape with n <= n_cam, cam_ids int32 (n,), state int32 (n_cam, 4) = {still, epoch, changed, peak} per camera,
    scratch int32 with at least `frame_gate_scratch(n_cam, frame_bytes)` entries, all on the device.  For c = cam_ids[i]: n =
    the bytes of frames[i] more than pixel_delta (0 .. 255) away from anchor[c]; without an anchor (still == -1) or with n >
    limit (0 .. frame_bytes) the frame moves -- anchor[c] = frames[i], still = 0, epoch += 1 --, else still += 1.  An id outside
    [0, n_cam) writes nothing; the same id twice is an error this wrapper cannot see.  Integers only, 16-, 4- or 1-byte accesses
    as `frame_ring_push`.  Three launches, nothing is read back, no autograd.  -> state."""
    what = "frame_gate_update"
    if not torch.is_tensor(anchor) or anchor.dim() < 2:
        raise _lib.HipExtensionError(f"{what}: anchor must be a torch.uint8 tensor (n_cam, frame_bytes) or (n_cam, FH, FW, 3) on the GPU, got "
                                     f"{tuple(getattr(anchor, 'shape', ())) or type(anchor).__name__}")
    anchor = _live_arg(anchor, torch.uint8, (None,) * anchor.dim(), what, "anchor")
    n_cam = anchor.shape[0]
    fb = anchor.numel() // n_cam
    frames = _live_arg(frames, torch.uint8, (None,) + tuple(anchor.shape[1:]), what, "frames", anchor.device)
    n = frames.shape[0]
    if n > n_cam:
        raise _lib.HipExtensionError(f"{what}: {n} frames for {n_cam} cameras: one frame per camera and call")
    cam_ids = _live_arg(cam_ids, torch.int32, (n,), what, "cam_ids", anchor.device)
    state = _live_arg(state, torch.int32, (n_cam, 4), what, "state", anchor.device)
    scratch = _live_arg(scratch, torch.int32, (None,), what, "scratch", anchor.device)
    if scratch.shape[0] < frame_gate_scratch(n_cam, fb):
        raise _lib.HipExtensionError(f"{what}: scratch holds {scratch.shape[0]} entries, {n_cam} cameras x {fb} bytes need "
                                     f"{frame_gate_scratch(n_cam, fb)} (frame_gate_scratch)")
    for name, v, hi in (("pixel_delta", pixel_delta, 255), ("limit", limit, fb)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= hi:
            raise _lib.HipExtensionError(f"{what}: {name} {v!r} is not an integer in [0, {hi}]")
    if fb >= 1 << 31:
        raise _lib.HipExtensionError(f"{what}: frames of {fb} bytes: the counts are int32 (frame_bytes < 2^31)")
    require_gpu(anchor)  # (the current device)
    check(_lib.load().advhip_frame_gate_update_u8(ptr(frames), ptr(cam_ids), ptr(anchor), ptr(state), ptr(scratch), n, n_cam, fb, pixel_delta, limit,
                                                  stream()), what)
    return state


def ring_repeat(cam_ids: torch.Tensor, ring: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """The newest clip of each of n distinct cameras again (include/advhip.h: motion gate, holding): cam_ids int32 (n,), ring
    (n_cam, ncrops, W, C + 1) fp32, counts int64 (n_cam,).  Camera c = cam_ids[i] with counts[c] >= 1 gets ring[c, :, counts[c] %
    W] = ring[c, :, (counts[c] - 1) % W] bit for bit, magnitude channel included (at W == 1 nothing is copied); then counts[c] +=
    1.  A camera at count 0 or an id outside [0, n_cam) writes nothing and advances nothing.  Two launches, no autograd."""
    what = "ring_repeat"
    ring = _live_arg(ring, torch.float32, (None, None, None, None), what, "ring")
    n_cam, ncrops, W, C1 = ring.shape
    cam_ids = _live_arg(cam_ids, torch.int32, (None,), what, "cam_ids", ring.device)
    counts = _live_arg(counts, torch.int64, (n_cam,), what, "counts", ring.device)
    require_gpu(ring)  # (the current device)
    check(_lib.load().advhip_ring_repeat_f32(ptr(cam_ids), ptr(ring), ptr(counts), cam_ids.shape[0], n_cam, ncrops, W, C1, stream()), what)
    return ring


LIVE_EVENTS_STATE = ("ring", "samples", "cand_int", "cand_peak", "cand_sum", "alert", "open_start", "log_int", "log_f", "emitted")


def live_events_state(n_cam: int, smooth: int, log: int, device) -> dict:
    """The per-camera state of `live_events_update` for n_cam cameras, a window of `smooth` samples and a log of `log` events per
    camera, as include/advhip.h ("live events") lays it out: nothing fed, nothing open, generation 0."""
    dev, z = torch.device(device), torch.zeros
    cand_int = z((n_cam, _lib.LIVE_EVENTS_CAND_INTS), dtype=torch.int32)
    cand_int[:, :3] = -1
    return {"ring": z((n_cam, smooth), dtype=torch.float32, device=dev), "samples": z((n_cam,), dtype=torch.int64, device=dev),
            "cand_int": cand_int.to(dev), "cand_peak": z((n_cam,), dtype=torch.float32, device=dev),
            "cand_sum": z((n_cam, 2), dtype=torch.float64, device=dev), "alert": z((n_cam,), dtype=torch.int32, device=dev),
            "open_start": torch.full((n_cam,), -1, dtype=torch.int32).to(dev), "log_int": z((n_cam, log, 4), dtype=torch.int32, device=dev),
            "log_f": z((n_cam, log, 2), dtype=torch.float32, device=dev), "emitted": z((n_cam,), dtype=torch.int64, device=dev)}


def live_events_update(scores: Optional[torch.Tensor], cam_ids: torch.Tensor, state: dict, low: float, high: float, smooth: int = 1,
                       merge_gap: int = 0, min_len: int = 1, by_camera: bool = False, mode: int = _lib.LIVE_EVENTS_UPDATE) -> dict:
    """One launch of the streaming event rule (include/advhip.h: live events) for the nb distinct cameras of cam_ids (int32 (nb,)
    on the device).  `state`: the tensors of `live_events_state` (ring (n_cam, smooth) fp32, samples int64, cand_int int32
    (n_cam, 5), cand_peak fp32, cand_sum float64 (n_cam, 2), alert and open_start int32, log_int int32 (n_cam, K, 4), log_f fp32
    (n_cam, K, 2), emitted int64), written in place for the listed cameras only.  mode LIVE_EVENTS_UPDATE feeds one sample each:
    scores[cam_ids[v]] of an fp32 (n_cam,) tensor with by_camera (LiveScorer.latest as it is), else scores[v] of an fp32 (nb,)
    one.  LIVE_EVENTS_FINISH / LIVE_EVENTS_RESET take scores = None.  The ids' values are the caller's (nothing is read back):
    an id outside [0, n_cam) writes nothing, the same id twice is an error this wrapper cannot see.  No autograd."""
    what, err = "live_events_update", _lib.HipExtensionError
    if not isinstance(state, dict) or sorted(state) != sorted(LIVE_EVENTS_STATE):
        raise err(f"{what}: state must be a dict of the tensors {list(LIVE_EVENTS_STATE)} (mil_ops.live_events_state)")
    ring = _live_arg(state["ring"], torch.float32, (None, None), what, "ring")
    n_cam, dev = ring.shape[0], ring.device
    if isinstance(smooth, bool) or int(smooth) != smooth or int(smooth) != ring.shape[1]:
        raise err(f"{what}: ring must be (n_cam, smooth = {smooth!r}), got {tuple(ring.shape)}")
    log_int = _live_arg(state["log_int"], torch.int32, (n_cam, None, 4), what, "log_int", dev)
    K = log_int.shape[1]
    rest = [_live_arg(state[name], dtype, shape, what, name, dev) for name, dtype, shape in (
        ("samples", torch.int64, (n_cam,)), ("cand_int", torch.int32, (n_cam, _lib.LIVE_EVENTS_CAND_INTS)), ("cand_peak", torch.float32, (n_cam,)),
        ("cand_sum", torch.float64, (n_cam, 2)), ("alert", torch.int32, (n_cam,)), ("open_start", torch.int32, (n_cam,)))]
    log_f = _live_arg(state["log_f"], torch.float32, (n_cam, K, 2), what, "log_f", dev)
    emitted = _live_arg(state["emitted"], torch.int64, (n_cam,), what, "emitted", dev)
    cam_ids = _live_arg(cam_ids, torch.int32, (None,), what, "cam_ids", dev)
    nb = cam_ids.shape[0]
    if mode not in (_lib.LIVE_EVENTS_UPDATE, _lib.LIVE_EVENTS_FINISH, _lib.LIVE_EVENTS_RESET):
        raise err(f"{what}: mode {mode!r} is not LIVE_EVENTS_UPDATE, LIVE_EVENTS_FINISH or LIVE_EVENTS_RESET")
    if mode == _lib.LIVE_EVENTS_UPDATE:
        scores = _live_arg(scores, torch.float32, (n_cam if by_camera else nb,), what, "scores", dev)
    elif scores is not None:
        raise err(f"{what}: finish and reset feed no sample: scores must be None")
    for name, v, lo in (("merge_gap", merge_gap, 0), ("min_len", min_len, 1)):
        if isinstance(v, bool) or int(v) != v or not lo <= int(v) < 1 << 31:
            raise err(f"{what}: {name} {v!r} is not an integer in [{lo}, 2^31)")
    require_gpu(ring)  # (the current device)
    check(_lib.load().advhip_live_events_update_f32(ptr(scores), ptr(cam_ids), ptr(ring), *(ptr(t) for t in rest), ptr(log_int), ptr(log_f), ptr(emitted),
                                                    nb, n_cam, K, int(smooth), float(low), float(high), int(merge_gap), int(min_len),
                                                    1 if by_camera else 0, int(mode), stream()), what)
    return state


def _gather_side(store, idx, labels, dst_labels, what: str):
    """Checks of one store of `gather_batch` -> (n, R, b)."""
    err = _lib.HipExtensionError
    if not (torch.is_tensor(store) and store.dtype == torch.float32 and store.dim() >= 1 and store.numel() > 0 and store.is_contiguous()):
        raise err(f"{what}: the store must be a non-empty contiguous fp32 tensor (n, ...), got "
                  f"{getattr(store, 'dtype', type(store))} {tuple(getattr(store, 'shape', ()))}")
    if not (torch.is_tensor(idx) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.numel() > 0 and idx.is_contiguous()
            and idx.device == store.device):
        raise err(f"{what}: the index must be a non-empty contiguous int64 vector on {store.device}, got "
                  f"{getattr(idx, 'dtype', type(idx))} {tuple(getattr(idx, 'shape', ()))} on {getattr(idx, 'device', None)}")
    n, b = store.shape[0], idx.numel()
    if (labels is None) != (dst_labels is None):
        raise err(f"{what}: labels need both a source and a destination")
    if labels is not None:
        for t, k, name in ((labels, n, "labels"), (dst_labels, b, "label destination")):
            if not (torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == (k,) and t.is_contiguous() and t.device == store.device):
                raise err(f"{what}: the {name} must be a contiguous fp32 ({k},) vector on {store.device}")
    return n, store.numel() // n, b


def gather_batch(store0: torch.Tensor, idx0: torch.Tensor, store1: Optional[torch.Tensor], idx1: Optional[torch.Tensor], dst: torch.Tensor,
                 labels0: Optional[torch.Tensor] = None, labels1: Optional[torch.Tensor] = None, dst_labels0: Optional[torch.Tensor] = None,
                 dst_labels1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One launch fills dst (b0 + b1, *row) fp32: dst[i] = store0[idx0[i]] for i < b0, dst[b0 + i] = store1[idx1[i]], for contiguous
    fp32 stores (n, *row) of one row shape and device int64 index vectors (nothing is read back); with labels, dst_labels0[i] =
    labels0[idx0[i]] and dst_labels1[i] = labels1[idx1[i]].  `store1` / `idx1` None: one store.  A copy of bits.  An index outside
    [0, n) gives a NaN row and a NaN label.  Stores and dst may be views at any 4-byte boundary.  No autograd."""
    err = _lib.HipExtensionError
    require_gpu(store0, idx0, store1, idx1, dst, labels0, labels1, dst_labels0, dst_labels1)
    n0, R, b0 = _gather_side(store0, idx0, labels0, dst_labels0, "gather_batch")
    n1 = b1 = 0
    if store1 is not None or idx1 is not None:
        n1, R1, b1 = _gather_side(store1, idx1, labels1, dst_labels1, "gather_batch (second store)")
        if tuple(store1.shape[1:]) != tuple(store0.shape[1:]) or store1.device != store0.device:
            raise err(f"gather_batch: the stores' rows differ: {tuple(store0.shape[1:])} on {store0.device} and {tuple(store1.shape[1:])} on {store1.device}")
    elif labels1 is not None or dst_labels1 is not None:
        raise err("gather_batch: labels of a second store that is not given")
    want = (b0 + b1,) + tuple(store0.shape[1:])
    if not (torch.is_tensor(dst) and dst.dtype == torch.float32 and tuple(dst.shape) == want and dst.device == store0.device):
        raise err(f"gather_batch: dst must be fp32 {want} on {store0.device}, got {getattr(dst, 'dtype', type(dst))} "
                  f"{tuple(getattr(dst, 'shape', ()))} on {getattr(dst, 'device', None)}")
    check(_lib.load().advhip_gather_batch_f32(ptr(store0), ptr(idx0), ptr(labels0), n0, b0, ptr(store1), ptr(idx1), ptr(labels1), n1, b1, ptr(dst),
                                              ptr(dst_labels0), ptr(dst_labels1), R, stream()), "gather_batch")
    return dst


def gather_rows(store: torch.Tensor, idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """store[idx] for a contiguous fp32 store (n, *row) and a device int64 index vector, bit for bit, as one HIP launch (`gather_batch`
    with one store).  `out`: a contiguous fp32 (len(idx), *row) tensor on the same device to write into.  An index outside [0, n)
    gives a NaN row (torch indexing would wrap a negative one and fault on a large one)."""
    require_gpu(store, idx, out)
    if out is None and torch.is_tensor(store) and torch.is_tensor(idx) and idx.dim() == 1:
        out = torch.empty((idx.numel(),) + tuple(store.shape[1:]), device=store.device, dtype=torch.float32)
    return gather_batch(store, idx, None, None, out)


LOSS_TERMS = ("total", "bce", "con", "con_a", "con_n", "smooth", "sparse", "mgfn")


def mgfn_loss(sc, abn_score, nor_score, a_feat, n_feat, abn_labels, nor_labels, ncrops: int):
    """-> (total loss [differentiable], terms tensor(8) in LOSS_TERMS order)."""
    if sc.dim() == 3:
        sc = sc.squeeze(-1)
    return _MgfnLoss.apply(sc, abn_score.reshape(-1), nor_score.reshape(-1), a_feat, n_feat, abn_labels, nor_labels, ncrops)


# ------------------------------------------------------------------- feature post-processing
def segment_features(feats: torch.Tensor, seg_length: int = 32) -> torch.Tensor:
    """(n_clips, ncrops, C) -> (ncrops, seg_length, C), extract_features.py:171-183, on device."""
    feats = feats.contiguous()
    require_gpu(feats)
    n, ncrops, C = feats.shape
    out = torch.empty((ncrops, seg_length, C), device=feats.device, dtype=torch.float32)
    check(_lib.load().advhip_segment_features_f32(ptr(feats), ptr(out), n, ncrops, C, seg_length, stream()), "segment_features")
    return out


def add_magnitude(feats: torch.Tensor) -> torch.Tensor:
    """(..., C) -> (..., C+1) with the L2 norm appended (dataset.py:121-124), on device."""
    feats = feats.contiguous()
    require_gpu(feats)
    C = feats.shape[-1]
    rows = feats.numel() // C
    out = torch.empty(feats.shape[:-1] + (C + 1,), device=feats.device, dtype=torch.float32)
    check(_lib.load().advhip_add_magnitude_f32(ptr(feats), ptr(out), rows, C, stream()), "add_magnitude")
    return out


ADD_MAGNITUDE_NP_MAX_C = 8192  # numpy reduces in chunks of 8192 elements: the order of its sum changes above that


def add_magnitude_np(feats: torch.Tensor, transpose: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(a, b, C) fp32 -> (a, b, C+1), or (b, a, C+1) with `transpose`: FeatureDataset.add_magnitude on the device with numpy's
    bits -- out[..., C] equals np.linalg.norm(feats, axis=2) bit for bit (`add_magnitude` agrees with it to 1e-6), out[..., :C]
    is the input.  `out`: a contiguous fp32 tensor of that shape on the same device to write into (a slot of a resident store).
    C <= 8192."""
    require_gpu(feats, out)
    if feats.dtype != torch.float32 or feats.dim() != 3:
        raise ValueError(f"add_magnitude_np: expected fp32 (a, b, C), got {feats.dtype} {tuple(feats.shape)}")
    a, b, C = feats.shape
    shape = (b, a, C + 1) if transpose else (a, b, C + 1)
    if out is None:
        out = torch.empty(shape, device=feats.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != feats.device:
        raise ValueError(f"add_magnitude_np: out must be fp32 {shape} on {feats.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    check(_lib.load().advhip_add_magnitude_np_f32(ptr(feats), ptr(out), a, b, C, int(bool(transpose)), stream()), "add_magnitude_np")
    return out


def add_magnitude_np_leaves(C: int):
    """[(start, len, adds)]: the blocks of at most 128 elements `add_magnitude_np` sums a row of C by, in order, and after how
    many of them a pending partial sum is added (host arithmetic only; nothing is launched)."""
    import ctypes

    buf = (ctypes.c_int32 * (3 * 128))()
    n = ctypes.c_int32()
    check(_lib.load().advhip_add_magnitude_np_leaves(int(C), buf, ctypes.byref(n)), "add_magnitude_np_leaves")
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n.value)]


def frame_scores(scores: torch.Tensor, frames_per_clip: int = 16, clip_stride: Optional[int] = None,
                 n_frames: Optional[int] = None, frame_step: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-window scores (n,) -> per-frame scores (n_frames,) on the device.  Window w covers frames [w * clip_stride,
    w * clip_stride + frames_per_clip); a frame's score is the mean of the scores of the windows covering it (fp32, ascending
    window order, one division by the count).  n_frames defaults to (n - 1) * clip_stride + frames_per_clip; clip_stride =
    frames_per_clip gives np.repeat(scores, frames_per_clip) (src/runner.py:66-76) bit for bit.
    `frame_step` d: the windows are spans of frames_per_clip * d frames -- window w covers [w * clip_stride, w * clip_stride +
    frames_per_clip * d), clip_stride defaults to the span: the same kernel at that clip length; the default stride gives
    np.repeat(scores, frames_per_clip * d).  `out`: a contiguous fp32 (n_frames,) tensor on the same device to write into."""
    d = resolve_frame_step(frame_step)
    s = resolve_clip_stride(frames_per_clip, clip_stride, d)
    frames_per_clip = frames_per_clip * d
    scores = scores.contiguous()
    require_gpu(scores)
    if scores.dtype != torch.float32 or scores.dim() != 1 or scores.numel() == 0:
        raise ValueError(f"frame_scores: expected a non-empty fp32 (n_windows,) tensor, got {scores.dtype} {tuple(scores.shape)}")
    n = scores.shape[0]
    covered = (n - 1) * s + frames_per_clip
    nf = covered if n_frames is None else int(n_frames)
    if not 0 < nf <= covered:
        raise ValueError(f"frame_scores: {nf} frames, but {n} windows of {frames_per_clip} at stride {s} cover {covered}")
    if out is None:
        out = torch.empty((nf,), device=scores.device, dtype=torch.float32)
    else:
        require_gpu(out)
        if out.dtype != torch.float32 or tuple(out.shape) != (nf,) or out.device != scores.device:
            raise ValueError(f"frame_scores: out must be fp32 ({nf},) on {scores.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    check(_lib.load().advhip_frame_scores_f32(ptr(scores), ptr(out), n, frames_per_clip, s, nf, stream()), "frame_scores")
    return out


def roc_counts_workspace(m: int, device) -> torch.Tensor:
    """The scratch buffer `roc_counts` needs for m items (uint8; reusable across calls of that size or smaller)."""
    nbytes = _lib.load().advhip_roc_counts_ws_bytes(int(m))
    if nbytes < 0:
        check(int(nbytes), "roc_counts_ws_bytes")
    return torch.empty((nbytes,), device=device, dtype=torch.uint8)


def roc_counts(scores: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
               workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Items (score fp32, pos int32, neg int32), each standing for pos positive and neg negative frames of that score, ->
    (thresholds fp32 (G,), tps int64 (G,), fps int64 (G,)) on the device: entry g is the g-th distinct score in descending order
    with the numbers of positive / negative frames scored at or above it -- what metrics._ranked computes from the expanded
    frames, integer for integer (metrics.roc_auc_from_counts / pr_auc_from_counts turn them into the two areas).  Equal floats
    are one entry: -0.0 and +0.0 together (the threshold carries either sign), denormals on their own; an item with pos = neg = 0
    still makes or joins the entry of its score.  One read-back of four
    integers is the only synchronisation.  ValueError for NaN / inf scores (with their number), as sklearn refuses them.
    `workspace`: a buffer from roc_counts_workspace(m >= len(scores), device) to reuse."""
    if scores.dtype != torch.float32 or scores.dim() != 1 or scores.numel() == 0:
        raise ValueError(f"roc_counts: scores must be a non-empty fp32 (M,) tensor, got {scores.dtype} {tuple(scores.shape)}")
    m = scores.shape[0]
    for name, t in (("pos", pos), ("neg", neg)):
        if t.dtype != torch.int32 or tuple(t.shape) != (m,):
            raise ValueError(f"roc_counts: {name} must be int32 ({m},) like the scores, got {t.dtype} {tuple(t.shape)}")
    if m >= 1 << 31:
        raise ValueError(f"roc_counts: {m} items, the limit is 2^31 - 1")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.dim() != 1):
        raise ValueError(f"roc_counts: workspace must be a uint8 (bytes,) tensor, got {workspace.dtype} {tuple(workspace.shape)}")
    require_gpu(scores, pos, neg, workspace)
    lib = _lib.load()
    if workspace is None:
        workspace = roc_counts_workspace(m, scores.device)
    dev = scores.device
    thresholds = torch.empty((m,), device=dev, dtype=torch.float32)
    tps = torch.empty((m,), device=dev, dtype=torch.int64)
    fps = torch.empty((m,), device=dev, dtype=torch.int64)
    meta = torch.empty((4,), device=dev, dtype=torch.int64)
    check(lib.advhip_roc_counts(ptr(scores), ptr(pos), ptr(neg), m, ptr(thresholds), ptr(tps), ptr(fps), ptr(meta), ptr(workspace),
                                workspace.numel(), stream()), "roc_counts")
    g, bad, _, _ = meta.tolist()  # the one synchronisation
    if bad:
        raise ValueError(f"roc_counts: {bad} non-finite scores (NaN or inf) among {m}: the curve is undefined")
    return thresholds[:g], tps[:g], fps[:g]


def _ragged_checks(what: str, scores: torch.Tensor, offsets: torch.Tensor) -> Tuple[int, int]:
    if scores.dtype != torch.float32 or scores.dim() != 1 or scores.numel() == 0:
        raise ValueError(f"{what}: scores must be a non-empty fp32 (N,) tensor, got {scores.dtype} {tuple(scores.shape)}")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError(f"{what}: offsets must be an int64 (V + 1,) tensor with V >= 1, got {offsets.dtype} {tuple(offsets.shape)}")
    if scores.shape[0] >= 1 << 31:
        raise ValueError(f"{what}: {scores.shape[0]} positions, the limit is 2^31 - 1")
    require_gpu(scores, offsets)
    return scores.shape[0], offsets.shape[0] - 1


def _host_offsets(what: str, offsets: torch.Tensor, offsets_host, n: int):
    """The offsets as a host int64 array (`offsets_host`, or one read-back of the device tensor), checked: non-decreasing from 0
    to n."""
    import numpy as np

    host = offsets.cpu().numpy() if offsets_host is None else np.asarray(offsets_host)
    if host.dtype.kind not in "iu" or host.shape != (offsets.shape[0],):
        raise ValueError(f"{what}: the host copy of the offsets must hold {offsets.shape[0]} integers, got {host.dtype} {host.shape}")
    host = host.astype(np.int64)
    if host[0] != 0 or host[-1] != n or (np.diff(host) < 0).any():
        raise ValueError(f"{what}: offsets must be non-decreasing from 0 to N = {n}, got {host[0]} .. {host[-1]}"
                         + (" with a decreasing step" if (np.diff(host) < 0).any() else ""))
    return host


def smooth_scores(scores: torch.Tensor, offsets: torch.Tensor, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Centred moving average of a ragged batch of score curves on the device: `scores` fp32 (N,) holds V videos back to back,
    video v = scores[offsets[v]:offsets[v + 1]] (`offsets` int64 (V + 1,) on the same device, non-decreasing from 0 to N; a
    length of 0 is allowed).  `window` w is odd, 1 <= w <= 1023: y[t] = sum(x[max(0, t - h) .. min(L - 1, t + h)]) / count with
    h = (w - 1) / 2, never across a video boundary; the sum is fp32 in ascending order from +0.0, one division by the count
    (frame_scores' convention), so w = 1 returns the input's bits (-0.0 becomes +0.0) and NaN / inf propagate as IEEE does.
    `out`: a contiguous fp32 (N,) tensor on the same device, not `scores` itself.  One launch, nothing synchronises."""
    n, v = _ragged_checks("smooth_scores", scores, offsets)
    w = int(window)
    if w != window or not 1 <= w <= 1023 or w % 2 == 0:
        raise ValueError(f"smooth_scores: window {window!r} is not an odd integer in [1, 1023]")
    if out is None:
        out = torch.empty_like(scores)
    else:
        require_gpu(out)
        if out.dtype != torch.float32 or tuple(out.shape) != (n,) or out.device != scores.device:
            raise ValueError(f"smooth_scores: out must be fp32 ({n},) on {scores.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if out.data_ptr() == scores.data_ptr():
            raise ValueError("smooth_scores: out must not be the scores themselves (a frame reads its neighbours)")
    check(_lib.load().advhip_smooth_scores_f32(ptr(scores), ptr(offsets), v, n, w, ptr(out), stream()), "smooth_scores")
    return out


def score_events_workspace(n: int, v: int, device) -> torch.Tensor:
    """The scratch buffer `score_events` needs for n positions in v videos (uint8; reusable for that size or smaller ones)."""
    nbytes = _lib.load().advhip_score_events_ws_bytes(int(n), int(v))
    if nbytes < 0:
        check(int(nbytes), "score_events_ws_bytes")
    return torch.empty((nbytes,), device=device, dtype=torch.uint8)


def score_events(smoothed: torch.Tensor, offsets: torch.Tensor, low: float, high: float, merge_gap: int = 0, min_len: int = 1,
                 workspace: Optional[torch.Tensor] = None, offsets_host=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Events of a ragged batch of (smoothed) score curves on the device, laid out as for `smooth_scores`.  A frame is active iff
    y >= low and strong iff y >= high (low <= high, finite; a NaN is neither).  Candidates are the maximal runs of active frames,
    two runs at most `merge_gap` inactive frames apart being one (as a chain); a candidate is an event iff it holds a strong
    frame and is at least `min_len` frames long.  -> (ev_int int32 (E, 4) = video, start, end, peak_frame; ev_f fp32 (E, 2) =
    peak, mean; counts int32 (V,)), in (video, start) order, frames local to the video and `end` exclusive; peak = the largest y
    of the interval (NaN ignored) at its first frame, mean = the float64 sum over [start, end) / length rounded to fp32 (gap
    frames included: a NaN there shows).  Identical bits in every run.  One read-back of two integers is the only
    synchronisation.  `offsets_host`: the host copy of the offsets (any integer sequence), from which the wrapper checks them and
    sizes the event list (sum of ceil(L_v / 2) rows: nothing can overflow); without it the device tensor is read back once more.
    `workspace`: a buffer from score_events_workspace(n >= N, v >= V, device) to reuse."""
    import math

    n, v = _ragged_checks("score_events", smoothed, offsets)
    low, high = float(low), float(high)
    if not (math.isfinite(low) and math.isfinite(high)) or low > high:
        raise ValueError(f"score_events: thresholds low = {low}, high = {high}: finite, low <= high")
    if int(merge_gap) != merge_gap or not 0 <= merge_gap < 1 << 31:
        raise ValueError(f"score_events: merge_gap {merge_gap!r} is not an integer in [0, 2^31)")
    if int(min_len) != min_len or not 1 <= min_len < 1 << 31:
        raise ValueError(f"score_events: min_len {min_len!r} is not an integer in [1, 2^31)")
    if workspace is not None and (workspace.dtype != torch.uint8 or workspace.dim() != 1):
        raise ValueError(f"score_events: workspace must be a uint8 (bytes,) tensor, got {workspace.dtype} {tuple(workspace.shape)}")
    require_gpu(workspace)
    host = _host_offsets("score_events", offsets, offsets_host, n)
    lengths = host[1:] - host[:-1]
    cap = max(1, int(((lengths + 1) // 2).sum()))
    lib = _lib.load()
    if workspace is None:
        workspace = score_events_workspace(n, v, smoothed.device)
    dev = smoothed.device
    ev_int = torch.empty((cap, 4), device=dev, dtype=torch.int32)
    ev_f = torch.empty((cap, 2), device=dev, dtype=torch.float32)
    counts = torch.empty((v,), device=dev, dtype=torch.int32)
    meta = torch.empty((2,), device=dev, dtype=torch.int64)
    check(lib.advhip_score_events(ptr(smoothed), ptr(offsets), v, n, low, high, int(merge_gap), int(min_len), ptr(ev_int), ptr(ev_f), cap,
                                  ptr(counts), ptr(meta), ptr(workspace), workspace.numel(), stream()), "score_events")
    found, written = meta.tolist()  # the one synchronisation
    if found > written:
        raise _lib.HipExtensionError(f"score_events: {found} events for {cap} rows: the offsets on the device are not the host's")
    return ev_int[:written], ev_f[:written], counts
