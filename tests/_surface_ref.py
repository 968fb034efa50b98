"""numpy restatement of 4:2:0 decoder surfaces (include/advhip.h, resize.Surface): a frame as a run of bytes plus the byte
geometry (height, width, bits, shift, y_offset, y_pitch, cb_offset, cr_offset, chroma_pitch, chroma_step), 8-bit samples or
little-endian 16-bit words holding ten bits at `shift`, nearest chroma, and the 2^(8 + bits) fixed-point integer formula --
written from the definition, with its own copy of the 10-bit coefficient table and its own geometry arithmetic, not through
resize.py.  The CPU reference the surface kernels are tested against."""
import numpy as np

import _yuv_ref

# (matrix, full_range) -> (yoff, cy, crv, cgu, cgv, cbu) at 10 bits
TABLE10 = {
    ("bt601", False): (64, 76309, 104597, 25675, 53279, 132201),
    ("bt601", True): (0, 65344, 91612, 22487, 46664, 115789),
    ("bt709", False): (64, 76309, 117489, 13975, 34925, 138438),
    ("bt709", True): (0, 65344, 102903, 12240, 30589, 121252),
}
TABLES = {8: _yuv_ref.TABLE, 10: TABLE10}
MODES = _yuv_ref.MODES
FIELDS = ("height", "width", "bits", "shift", "y_offset", "y_pitch", "cb_offset", "cr_offset", "chroma_pitch", "chroma_step")


def geometry(layout, h, w, pitch=None, rows=None, chroma_pitch=None, bits=8, shift=None, order="uv", y_offset=0):
    """The geometry tuple (FIELDS) of the usual allocations: luma rows of `pitch` bytes, `rows` allocated rows, chroma behind them."""
    sb = 1 if bits == 8 else 2
    pitch = w * sb if pitch is None else pitch
    rows = h if rows is None else rows
    if shift is None:
        shift = 6 if (bits == 10 and layout == "nv12") else 0
    c0 = y_offset + pitch * rows
    if layout == "nv12":
        cp = pitch if chroma_pitch is None else chroma_pitch
        a, b, step = c0, c0 + sb, 2 * sb
    else:
        cp = (pitch // (2 * sb)) * sb if chroma_pitch is None else chroma_pitch
        a, b, step = c0, c0 + cp * ((rows + 1) // 2), sb
    cb, cr = (a, b) if order == "uv" else (b, a)
    return (h, w, bits, shift, y_offset, pitch, cb, cr, cp, step)


def _indices(geo):
    """Byte index of every luma sample (H, W) and of every Cb / Cr sample (H/2, W/2)."""
    h, w, bits, _shift, y_off, y_pitch, cb_off, cr_off, c_pitch, c_step = geo
    sb = 1 if bits == 8 else 2
    yy, xx = np.mgrid[:h, :w]
    r, c = np.mgrid[: h // 2, : w // 2]
    chroma = r * c_pitch + c * c_step
    return y_off + yy * y_pitch + xx * sb, cb_off + chroma, cr_off + chroma


def frame_bytes_min(geo) -> int:
    sb = 1 if geo[2] == 8 else 2
    return int(max(i.max() for i in _indices(geo))) + sb


def pack(y, cb, cr, geo, frame_bytes=None, seed=0) -> np.ndarray:
    """Planes Y (F, H, W), Cb, Cr (F, H/2, W/2) of sample values -> uint8 (F, frame_bytes) surfaces: seeded noise in every byte
    that holds no sample and, at 10 bits, in the six bits of each word that the sample does not use."""
    bits, shift = geo[2], geo[3]
    F = y.shape[0]
    n = frame_bytes_min(geo) if frame_bytes is None else frame_bytes
    buf = np.random.default_rng(seed).integers(0, 256, (F, n), dtype=np.uint8)
    for plane, idx in zip((y, cb, cr), _indices(geo)):
        idx = idx.reshape(-1)
        v = np.asarray(plane).reshape(F, -1).astype(np.uint16)
        if bits == 8:
            buf[:, idx] = v.astype(np.uint8)
        else:
            word = buf[:, idx].astype(np.uint16) | buf[:, idx + 1].astype(np.uint16) << 8  # the noise already there
            word = (word & np.uint16(~(1023 << shift) & 0xFFFF)) | (v << shift).astype(np.uint16)
            buf[:, idx] = (word & 255).astype(np.uint8)
            buf[:, idx + 1] = (word >> 8).astype(np.uint8)
    return buf


def unpack(buf: np.ndarray, geo):
    """uint8 (F, frame_bytes) -> sample values Y (F, H, W), Cb, Cr (F, H/2, W/2)."""
    bits, shift = geo[2], geo[3]
    out = []
    for idx in _indices(geo):
        if bits == 8:
            out.append(buf[:, idx].astype(np.int64))
        else:
            word = buf[:, idx].astype(np.int64) | buf[:, idx + 1].astype(np.int64) << 8
            out.append((word >> shift) & 1023)
    return tuple(out)


def convert(y, cb, cr, matrix="bt601", full_range=False, bits=8) -> np.ndarray:
    """Same-shaped sample values (chroma already at the luma's resolution) -> uint8 (..., 3) by the integer formula at that depth."""
    yoff, cy, crv, cgu, cgv, cbu = TABLES[bits][(matrix, full_range)]
    S, mid = 8 + bits, 1 << (bits - 1)
    y, cb, cr = (np.asarray(v).astype(np.int64) for v in (y, cb, cr))
    yi = cy * (y - yoff) + (1 << (S - 1))
    u, v = cb - mid, cr - mid
    rgb = np.stack([(yi + crv * v) >> S, (yi - cgu * u - cgv * v) >> S, (yi + cbu * u) >> S], axis=-1)  # (>> floors: arithmetic)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def exact(y, cb, cr, matrix="bt601", full_range=False, bits=8) -> np.ndarray:
    """The real-valued conversion in float64, rounded half up and clipped: what the integer formula approximates."""
    kr, kb = _yuv_ref.LUMA[matrix]
    kg = 1.0 - kr - kb
    up = float(1 << (bits - 8))
    ys, cs, yoff = (255.0 / ((1 << bits) - 1),) * 2 + (0.0,) if full_range else (255.0 / (219.0 * up), 255.0 / (224.0 * up), 16.0 * up)
    mid = float(1 << (bits - 1))
    y, u, v = ys * (np.asarray(y, dtype=np.float64) - yoff), cs * (np.asarray(cb, dtype=np.float64) - mid), cs * (np.asarray(cr, dtype=np.float64) - mid)
    rgb = np.stack([y + 2 * (1 - kr) * v, y - 2 * (1 - kb) * kb / kg * u - 2 * (1 - kr) * kr / kg * v, y + 2 * (1 - kb) * u], axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


def up2(c: np.ndarray) -> np.ndarray:
    """Chroma (F, H/2, W/2) at the luma's resolution: pixel (y, x) takes sample (y >> 1, x >> 1)."""
    return c.repeat(2, axis=1).repeat(2, axis=2)


def to_rgb(buf: np.ndarray, geo, matrix="bt601", full_range=False) -> np.ndarray:
    """uint8 (F, frame_bytes) surfaces -> (F, H, W, 3)."""
    y, cb, cr = unpack(buf, geo)
    return convert(y, up2(cb), up2(cr), matrix, full_range, geo[2])


def noise_planes(h, w, n, bits, seed):
    """Seeded sample values over the whole range of the depth: Y (n, h, w), Cb, Cr (n, h/2, w/2)."""
    g = np.random.default_rng(seed)
    top = 1 << bits
    return g.integers(0, top, (n, h, w)), g.integers(0, top, (n, h // 2, w // 2)), g.integers(0, top, (n, h // 2, w // 2))
