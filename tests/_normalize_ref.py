"""The three normalisers of the reference's src/gtransforms.py:57-112, restated in numpy on fp32 arrays, and the TenCrop passes
with them.  tests/test_normalize_host.py pins the restatement against tests/golden/normalize.npz (the reference's own outputs,
NaN positions included); the GPU tests compare the kernels with it bit for bit."""
import numpy as np

# fixture key -> the normalisation in the package's spelling (ops.resolve_normalize)
CASES = {
    "std_default": None,
    "std_channels": ("standardize", (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)),
    "pix_0_1": "pixel_minmax",
    "pix_m1_1": ("pixel_minmax", -1.0, 1.0),
    "pix_01_07": ("pixel_minmax", 0.1, 0.7),
    "ch_0_1": "channel_minmax",
    "ch_m1_1": ("channel_minmax", -1.0, 1.0),
    "ch_01_07": ("channel_minmax", 0.1, 0.7),
    "ch_lists": ("channel_minmax", (0.0, -1.0, 0.1), (1.0, 1.0, 0.7)),
}


def golden_input() -> np.ndarray:
    """uint8 (3, 10, 3, 8, 8) = (frames, crops, C, H, W) with one constant crop and one constant channel planted."""
    x = np.random.default_rng(20).integers(0, 256, size=(3, 10, 3, 8, 8), dtype=np.uint8)
    x[1, 4] = 77        # a constant crop: pixel_minmax and every channel of channel_minmax give 0 / 0 there
    x[2, 7, 1] = 200    # a constant channel: channel_minmax gives 0 / 0 in that channel only
    return x


def normalize_ref(x: np.ndarray, kind: str, a, b) -> np.ndarray:
    """`x` fp32 (..., C, H, W), C = 3; every leading index is one (frame, crop) of its own.  `a`, `b`: three Python floats each,
    (mean, std) or (lo, hi).  One separately rounded fp32 operation per step, in the reference's order."""
    x = np.asarray(x, dtype=np.float32)
    col = lambda v: np.asarray(v, dtype=np.float32).reshape(3, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "standardize":  # t.sub_(m).div_(s)
            return (x - col(a)) / col(b)
        if kind == "pixel_minmax":  # min / max over the whole (C, H, W); r = float32 of the double hi - lo
            mn, mx = x.min(axis=(-3, -2, -1), keepdims=True), x.max(axis=(-3, -2, -1), keepdims=True)
            q = (x - mn) / (mx - mn)
            return q * np.float32(b[0] - a[0]) + np.float32(a[0])
        if kind == "channel_minmax":  # per channel; r = float32(hi) - float32(lo)
            mn, mx = x.min(axis=(-2, -1), keepdims=True), x.max(axis=(-2, -1), keepdims=True)
            q = (x - mn) / (mx - mn)
            return q * (col(b) - col(a)) + col(a)
    raise ValueError(kind)


def tencrop_ref(frames: np.ndarray, normalize, frames_per_clip: int = 16, crop: int = 224, clip_stride=None, frame_step=None,
                crops=None) -> np.ndarray:
    """uint8 (F, H, W, 3) -> fp32 (n_windows * len(crops), 3, frames_per_clip, crop, crop): every window as a one-clip video of
    the frames ops.window_frame_indices names (a LoopPad copy carries the statistics of the frame it copies), TenCrop geometry from
    the host oracle (mean 0, std 1: the raw pixels as floats), each (frame, crop) normalised by normalize_ref."""
    from anomaly_detection_on_video_amd import ops
    from oracle.host_oracle import ten_crop_clips

    kind, a, b = ops.resolve_normalize(normalize)
    s, crops, d = ops.resolve_sampling(frames_per_clip, clip_stride, crops, frame_step)
    F = frames.shape[0]
    rows = []
    for w in range(ops.n_windows(F, frames_per_clip, s, d)):
        clip = frames[list(ops.window_frame_indices(F, w, frames_per_clip, s, d))]
        raw = ten_crop_clips(clip, frames_per_clip, crop, mean=0.0, std=1.0)[0]  # (10, C, T, crop, crop)
        out = normalize_ref(raw.transpose(0, 2, 1, 3, 4), kind, a, b).transpose(0, 2, 1, 3, 4)
        rows.append(out[list(crops)])
    return np.concatenate(rows, axis=0).astype(np.float32)


def crop_minmax_ref(frames: np.ndarray, crop: int, pitch: int = 1) -> np.ndarray:
    """uint8 (F, H, W, C) -> uint8 (ceil(F / pitch), 6, C, 2): (min, max) per channel of the six windows that hold the pixels of
    TenCrop's ten crops: the five of five_crop, and the centre crop of the mirrored frame seen in the frame's own columns."""
    F, H, W, C = frames.shape
    top_c, left_c = int(round((H - crop) / 2.0)), int(round((W - crop) / 2.0))
    offs = [(0, 0), (0, W - crop), (H - crop, 0), (H - crop, W - crop), (top_c, left_c), (top_c, W - crop - left_c)]
    sub = frames[::pitch]
    out = np.empty((sub.shape[0], 6, C, 2), dtype=np.uint8)
    for j, (t, l) in enumerate(offs):
        win = sub[:, t : t + crop, l : l + crop]
        out[:, j, :, 0] = win.min(axis=(1, 2))
        out[:, j, :, 1] = win.max(axis=(1, 2))
    return out
