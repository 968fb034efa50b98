"""Batched validation: score videos of unequal length in padded, length-sorted buckets.

A validation pass over a test set is one forward pass per video (the reference's DataLoader(batch_size=1)); at a few hundred
clips per video each pass is a chain of small launches that pays launch latency, not arithmetic.  Here the videos are sorted by
length and cut into buckets of `batch_videos`; a bucket is one (nb, ncrops, Tmax, C+1) tensor plus a length per video, scored
by MGFNForVideoAnomalyDetection.score_padded in ONE pass (the four operators that look along time take the lengths, see
DESIGN.md "Batched validation").  Sorting keeps the padding small: 290 videos of U[50, 500] clips in buckets of 16 are 19 passes
with about 4 % padded positions.

    plan_buckets(lengths, batch_videos, ncrops)      pure Python: which videos share a pass
    ScoreBatchPlan(dataset_or_videos, batch_videos)  built once: input buffer, per-bucket device arrays; .run(model, out)
    score_videos(model, videos, batch_videos)        the convenience form for a list of device tensors
"""
from __future__ import annotations

from typing import List, Sequence

DEFAULT_MAX_ROWS = 163_840  # 16 videos x 10 crops x 1024 clips: 1.34 GB of fp32 input at width 2049, far inside the kernels' 32-bit row limit


def plan_buckets(lengths: Sequence[int], batch_videos: int, ncrops: int, max_rows: int = DEFAULT_MAX_ROWS) -> List[List[int]]:
    """Index lists, one per scoring pass: the videos sorted by length (stable: ties keep their order), consecutive groups of at
    most `batch_videos`; a group closes early when one more video would make n * ncrops * Tmax pass `max_rows` (Tmax = the
    group's longest = its last), so a video that alone exceeds `max_rows` is a bucket of one."""
    batch_videos, ncrops, max_rows = int(batch_videos), int(ncrops), int(max_rows)
    if batch_videos < 1 or ncrops < 1 or max_rows < 1:
        raise ValueError(f"plan_buckets: batch_videos={batch_videos}, ncrops={ncrops}, max_rows={max_rows} must all be at least 1")
    lengths = [int(n) for n in lengths]
    if any(n < 1 for n in lengths):
        raise ValueError("plan_buckets: every video needs at least one clip")
    buckets: List[List[int]] = []
    cur: List[int] = []
    for i in sorted(range(len(lengths)), key=lengths.__getitem__):
        if cur and (len(cur) >= batch_videos or (len(cur) + 1) * ncrops * lengths[i] > max_rows):
            buckets.append(cur)
            cur = []
        cur.append(i)
    if cur:
        buckets.append(cur)
    return buckets


def padding_ratio(lengths: Sequence[int], buckets: Sequence[Sequence[int]]) -> float:
    """Positions the passes compute over the positions the videos have."""
    return sum(len(b) * max(lengths[i] for i in b) for b in buckets) / float(sum(lengths))


class _Bucket:
    __slots__ = ("videos", "tmax", "lens", "src_offsets", "dst_offsets", "oversize")


class ScoreBatchPlan:
    """Everything a batched scoring pass over one fixed set of videos needs, built once: the buckets, ONE input buffer sized for
    the largest of them, and per bucket the device arrays of its lengths and offsets (uploaded here).  `run(model, out)` then
    launches, per bucket, one pack (videos -> padded buffer), the scoring pass and one scatter (crop mean -> each video's slot of
    `out`): no host synchronisation and no host-to-device copy.

    `dataset_or_videos`: a resident test dataset (dataset.ResidentFeatureDataset: its flat `store` is read in place) or a list of
    (ncrops, T_i, C+1) fp32 tensors on `device` (copied into one flat store).  `out` is a flat fp32 device buffer with video i
    at [offsets[i], offsets[i+1]), offsets = the running sum of the clip counts -- metrics.FrameAucPlan.scores' layout."""

    def __init__(self, dataset_or_videos, batch_videos: int, device=None, max_rows: int = DEFAULT_MAX_ROWS):
        import torch

        from ._lib import HipExtensionError
        from .models.mgfn.modeling_mgfn import PaddedLens

        videos = getattr(dataset_or_videos, "videos", dataset_or_videos)
        store = getattr(dataset_or_videos, "store", None)
        src = getattr(dataset_or_videos, "offsets", None)
        if videos is None or len(videos) == 0:
            raise ValueError("ScoreBatchPlan: no videos (a resident TEST dataset or a list of (ncrops, T, C+1) tensors)")
        videos = list(videos)
        self.device = torch.device(device if device is not None else videos[0].device)
        if self.device.type == "cuda" and self.device.index is None and torch.is_tensor(videos[0]):
            self.device = videos[0].device  # ("cuda": the videos' own index)
        shape = tuple(videos[0].shape)
        for i, v in enumerate(videos):
            if not (torch.is_tensor(v) and v.is_cuda and v.device == self.device and v.dtype == torch.float32 and v.dim() == 3 and v.is_contiguous()):
                raise HipExtensionError(f"ScoreBatchPlan: video {i}: expected a contiguous fp32 (ncrops, T, C+1) tensor on {self.device} (there is no CPU fallback)")
            if (v.shape[0], v.shape[2]) != (shape[0], shape[2]) or v.shape[1] < 1:
                raise ValueError(f"ScoreBatchPlan: video {i} is {tuple(v.shape)}, video 0 is {shape}: crops and channels must agree")
        self.ncrops, self.width = int(shape[0]), int(shape[2])
        self.lengths = [int(v.shape[1]) for v in videos]
        if store is None:
            store = torch.cat([v.reshape(-1) for v in videos])
            src = [0]
            for v in videos:
                src.append(src[-1] + v.numel())
        self.store, self.videos = store, videos
        self.offsets = [0]
        for n in self.lengths:
            self.offsets.append(self.offsets[-1] + n)
        self.total = self.offsets[-1]
        self.batch_videos, self.max_rows = int(batch_videos), int(max_rows)
        self.index_lists = plan_buckets(self.lengths, self.batch_videos, self.ncrops, self.max_rows)
        self.buckets: List[_Bucket] = []
        floats = 0
        for idx in self.index_lists:
            b = _Bucket()
            b.videos, b.tmax = idx, max(self.lengths[i] for i in idx)
            b.oversize = len(idx) * self.ncrops * b.tmax > self.max_rows  # (a bucket of one, by plan_buckets: the per-video pass takes it)
            b.lens = b.src_offsets = b.dst_offsets = None
            if not b.oversize:
                b.lens = PaddedLens([self.lengths[i] for i in idx], self.ncrops, b.tmax, self.device)
                b.src_offsets = torch.tensor([int(src[i]) for i in idx], dtype=torch.int64).to(self.device)
                b.dst_offsets = torch.tensor([self.offsets[i] for i in idx], dtype=torch.int64).to(self.device)
                floats = max(floats, len(idx) * self.ncrops * b.tmax * self.width)
            self.buckets.append(b)
        # (never initialised: a bucket's tails hold whatever the bucket before left there, which score_padded never reads as values)
        self.buffer = torch.empty((floats,), dtype=torch.float32, device=self.device)
        self.padding_ratio = padding_ratio(self.lengths, self.index_lists)

    @property
    def buffer_bytes(self) -> int:
        return int(self.buffer.numel() * self.buffer.element_size())

    def new_scores(self):
        """A zero-filled flat score buffer of this plan's layout."""
        import torch

        return torch.zeros((self.total,), dtype=torch.float32, device=self.device)

    def slot(self, scores, i: int):
        return scores[self.offsets[i]:self.offsets[i + 1]]

    def run(self, model, out):
        """Score every bucket into `out` (flat fp32, `total` elements, on the plan's device); the model in eval mode."""
        import torch

        from . import mil_ops
        from ._lib import HipExtensionError

        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.device and out.dtype == torch.float32 and out.dim() == 1
                and out.numel() == self.total and out.is_contiguous()):
            raise HipExtensionError(f"ScoreBatchPlan.run: out must be a contiguous fp32 ({self.total},) tensor on {self.device}")
        with torch.no_grad():
            for b in self.buckets:
                if b.oversize:
                    i = b.videos[0]
                    self.slot(out, i).copy_(model(video=self.videos[i].unsqueeze(0)).scores.reshape(-1), non_blocking=True)
                    continue
                nb = len(b.videos)
                video = self.buffer[: nb * self.ncrops * b.tmax * self.width].view(nb, self.ncrops, b.tmax, self.width)
                mil_ops.pack_padded(self.store, b.src_offsets, b.lens.video_lens, video)
                scores, _ = model._score_padded_rows(video, b.lens)  # score_padded up to the per-crop scores ...
                mil_ops.crop_mean_scatter(scores, b.lens.video_lens, b.dst_offsets, out, nb, self.ncrops)  # ... whose crop mean goes straight to the slots
        return out


def score_videos(model, videos, batch_videos: int = 16, max_rows: int = DEFAULT_MAX_ROWS):
    """Frame scores of a list of (ncrops, T_i, C+1) fp32 device tensors, `batch_videos` of them per pass: a list of (T_i,) tensors
    (views of one buffer), video i's what `model(video=videos[i][None]).scores` holds."""
    plan = ScoreBatchPlan(videos, batch_videos, max_rows=max_rows)
    out = plan.run(model, plan.new_scores())
    return [plan.slot(out, i) for i in range(len(plan.lengths))]
