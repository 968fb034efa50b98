"""numpy restatement of the 4:2:0 -> RGB conversion (include/advhip.h, resize.yuv_coefficients): the layouts unpacked into
planes, nearest chroma, and the 2^16 fixed-point integer formula -- written from the definition, with its own copy of the
coefficient table, not through resize.py.  The CPU reference the HIP kernels are tested against."""
import numpy as np

# (matrix, full_range) -> (yoff, cy, crv, cgu, cgv, cbu)
TABLE = {
    ("bt601", False): (16, 76309, 104597, 25675, 53279, 132201),
    ("bt601", True): (0, 65536, 91881, 22553, 46802, 116130),
    ("bt709", False): (16, 76309, 117489, 13975, 34925, 138438),
    ("bt709", True): (0, 65536, 103206, 12276, 30679, 121609),
}
MODES = tuple(TABLE)
LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def unpack(frames: np.ndarray, layout: str):
    """uint8 (F, 3H/2, W) -> Y (F, H, W), Cb (F, H/2, W/2), Cr (F, H/2, W/2)."""
    F, rows, W = frames.shape
    H = rows // 3 * 2
    assert rows * 2 == H * 3 and H % 2 == 0 and W % 2 == 0
    y = frames[:, :H]
    c = frames[:, H:].reshape(F, -1)
    if layout == "nv12":
        c = c.reshape(F, H // 2, W // 2, 2)
        return y, c[..., 0], c[..., 1]
    assert layout == "i420"
    c = c.reshape(F, 2, H // 2, W // 2)
    return y, c[:, 0], c[:, 1]


def pack(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, layout: str) -> np.ndarray:
    """The inverse of unpack."""
    F, H, W = y.shape
    if layout == "nv12":
        c = np.stack([cb, cr], axis=-1).reshape(F, H // 2, W)
    else:
        c = np.concatenate([cb.reshape(F, -1), cr.reshape(F, -1)], axis=1).reshape(F, H // 2, W)
    return np.ascontiguousarray(np.concatenate([y, c], axis=1).astype(np.uint8))


def convert(y, cb, cr, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """Same-shaped Y, Cb, Cr (chroma already at the luma's resolution) -> uint8 (..., 3) by the integer formula."""
    yoff, cy, crv, cgu, cgv, cbu = TABLE[(matrix, full_range)]
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    yi = cy * (y - yoff) + (1 << 15)
    u, v = cb - 128, cr - 128
    rgb = np.stack([(yi + crv * v) >> 16, (yi - cgu * u - cgv * v) >> 16, (yi + cbu * u) >> 16], axis=-1)  # (>> floors: arithmetic)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def exact(y, cb, cr, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """The real-valued conversion in float64, rounded half up and clipped: what the integer formula approximates."""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs, yoff = (1.0, 1.0, 0.0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16.0)
    y, u, v = ys * (np.asarray(y, dtype=np.float64) - yoff), cs * (np.asarray(cb, dtype=np.float64) - 128.0), cs * (np.asarray(cr, dtype=np.float64) - 128.0)
    rgb = np.stack([y + 2 * (1 - kr) * v, y - 2 * (1 - kb) * kb / kg * u - 2 * (1 - kr) * kr / kg * v, y + 2 * (1 - kb) * u], axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def yuv420_to_rgb(frames: np.ndarray, layout: str, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """uint8 (F, 3H/2, W) -> (F, H, W, 3): pixel (y, x) takes chroma sample (y >> 1, x >> 1)."""
    y, cb, cr = unpack(frames, layout)
    up = lambda c: c.repeat(2, axis=1).repeat(2, axis=2)  # noqa: E731
    return convert(y, up(cb), up(cr), matrix, full_range)


def noise(h: int, w: int, n: int, seed: int) -> np.ndarray:
    """Seeded uint8 (n, 3h/2, w) white noise over the whole range (either layout reads it as a frame)."""
    return np.random.default_rng(seed).integers(0, 256, (n, h // 2 * 3, w), dtype=np.uint8)
