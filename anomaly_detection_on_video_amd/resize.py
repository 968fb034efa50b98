"""GroupResize on the device: the reference's `GroupResize(256, Image.BILINEAR)` (src/gtransforms.py:9-18, applied in
src/dataset.py:175-183) on decoded uint8 frames, bit-exact with Pillow.

Host side (this module): torchvision's `Resize(int)` output-size rule and Pillow's fixed-point resampling tables
(Resample.c: `precompute_coeffs` + `normalize_coeffs_8bpc`), restated in double precision with Pillow's order of operations.
Device side (csrc/resize.hip, `advhip_resize_u8`): Pillow's two passes, horizontal into a uint8 workspace then vertical,
each `clamp((2**21 + sum(pixel * coef)) >> 22, 0, 255)` in int32.  NEAREST and HAMMING are not supported.

Decoded frames as a decoder has them, 8-bit Y'CbCr 4:2:0 (NV12 / I420), go in through `pixel_format` (resolve_pixel_format):
the colour conversion is the integer formula of `yuv_coefficients`, on the device, inside the horizontal pass.  That formula is
this package's own definition, not ffmpeg swscale's bytes (the reference's RGB comes out of decord, i.e. swscale, which is not
available to pin against): packed RGB frames remain the reference-parity path.

A decoder's surface as it is -- a row pitch above W, aligned rows, plane offsets, NV21 / YV12 chroma order, 10-bit samples (P010,
yuv420p10le) -- goes in through `surface=` (Surface, surface, resolve_surface) next to `pixel_format`: the frames are then uint8
(F, frame_bytes) and the same kernels read them in place by byte geometry.

A part of the picture -- PIL's `Image.resize(size, resample, box=(left, top, right, bottom))`, float boxes -- goes through
`box_coefficients` (Pillow's `precompute_coeffs` with the box held as C floats), `roi_tables` (K stacked table sets on the device)
and `resize_rois_u8` (a source frame and a table per output frame, two launches: advhip_resize_roi_u8 and its 4:2:0 forms);
`resize_u8(box=)` is the one-box case.
"""
from __future__ import annotations

import math
from typing import Dict, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import HipExtensionError, check, ptr, require_gpu, stream

PRECISION_BITS = 22  # Pillow: 32 - 8 - 2

LAYOUTS = {"nv12": 0, "i420": 1}  # ADVHIP_YUV420_*
_LAYOUT_ALIASES = {"yuv420p": "i420"}
LUMA_WEIGHTS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}  # matrix -> (Kr, Kb)
YUV_BITS = 16


class PixelFormat(NamedTuple):
    """How decoded 4:2:0 frames are laid out and which Y'CbCr they hold."""
    layout: str  # "nv12" | "i420"
    matrix: str  # "bt601" | "bt709"
    full_range: bool


_PF_ACCEPTED = ('None (packed RGB), "nv12", "i420" (or "yuv420p"), (layout, "bt601" | "bt709"), (layout, matrix, "limited" | "full") '
                "or a PixelFormat")


def resolve_pixel_format(spec) -> Optional[PixelFormat]:
    """`pixel_format` of the frame entry points -> PixelFormat, or None for packed RGB (F, H, W, 3).  Accepted: None, "nv12",
    "i420" (also spelt "yuv420p"; defaults bt601, limited range), (layout, matrix), (layout, matrix, "limited" | "full") and a
    PixelFormat.  Anything else raises ValueError."""
    if spec is None:
        return None
    parts = (spec,) if isinstance(spec, str) else spec
    bad = ValueError(f"pixel_format {spec!r} is not supported: accepted are {_PF_ACCEPTED}")
    if not isinstance(parts, (tuple, list)) or not 1 <= len(parts) <= 3:
        raise bad
    layout, matrix, rng = (list(parts) + ["bt601", "limited"][len(parts) - 1:])[:3]
    if isinstance(rng, bool):  # (a PixelFormat's own field)
        rng = "full" if rng else "limited"
    if not all(isinstance(v, str) for v in (layout, matrix, rng)):
        raise bad
    layout = _LAYOUT_ALIASES.get(layout, layout)
    if layout not in LAYOUTS or matrix not in LUMA_WEIGHTS or rng not in ("limited", "full"):
        raise bad
    return PixelFormat(layout, matrix, rng == "full")


def frame_hw(shape) -> Tuple[int, int]:
    """(H, W) of 4:2:0 frames shaped (..., 3H/2, W): both layouts store a frame as 3H/2 rows of W bytes (Y, then chroma)."""
    if len(shape) < 2:
        raise ValueError(f"4:2:0 frames are (F, 3H/2, W), got shape {tuple(shape)}")
    rows, w = int(shape[-2]), int(shape[-1])
    if rows < 3 or rows % 3:
        raise ValueError(f"4:2:0 frames have 3H/2 rows: {rows} is not a positive multiple of 3")
    if w < 2 or w % 2:
        raise ValueError(f"4:2:0 frames need an even W, got W={w}")
    return rows // 3 * 2, w  # (an odd H has no whole chroma rows: its 3H/2 is not a multiple of 3)


def yuv_coefficients(pixel_format, bits: int = 8) -> Tuple[int, int, int, int, int, int]:
    """(yoff, cy, crv, cgu, cgv, cbu) of a pixel format at a sample depth of `bits` (8 or 10): round(real * 2**S), S = 8 + bits,
    of the Y'CbCr -> RGB matrix that the luma weights (Kr, Kb), the range and the depth give (limited range: yoff = 16 * 2**(bits -
    8), luma scale 255 / (219 * 2**(bits - 8)), chroma scale 255 / (224 * 2**(bits - 8)); full range: yoff = 0, both scales 255 /
    (2**bits - 1)).  The conversion, on the device and in any restatement, is with mid = 2**(bits - 1)
        yi = cy * (Y - yoff) + 2**(S - 1)
        R = clip8((yi + crv * (Cr - mid)) >> S)
        G = clip8((yi - cgu * (Cb - mid) - cgv * (Cr - mid)) >> S)        (arithmetic shifts)
        B = clip8((yi + cbu * (Cb - mid)) >> S)
    At 8 bits this is within 1 of the rounded real formula for every (Y, Cb, Cr) and differs from it on fewer than 0.03 % of the
    values; at 10 bits within 1 and on at most 0.110 % of the lattice of tests/test_surface_host.py."""
    pf = resolve_pixel_format(pixel_format)
    if pf is None:
        raise ValueError("yuv_coefficients: packed RGB has no conversion")
    if bits not in (8, 10):
        raise ValueError(f"yuv_coefficients: bits {bits!r} is neither 8 nor 10")
    kr, kb = LUMA_WEIGHTS[pf.matrix]
    kg = 1.0 - kr - kb
    up = 1 << (bits - 8)
    ys, cs, yoff = (255.0 / ((1 << bits) - 1),) * 2 + (0,) if pf.full_range else (255.0 / (219.0 * up), 255.0 / (224.0 * up), 16 * up)
    real = (ys, 2.0 * (1.0 - kr) * cs, 2.0 * (1.0 - kb) * kb / kg * cs, 2.0 * (1.0 - kr) * kr / kg * cs, 2.0 * (1.0 - kb) * cs)
    return (yoff,) + tuple(int(round(v * (1 << (8 + bits)))) for v in real)


class Surface(NamedTuple):
    """Where the samples of one 4:2:0 frame are inside its `frame_bytes` bytes: every offset, pitch and step in bytes from the
    frame's first byte (what VAImage.offsets / pitches or an AVFrame's planes and linesizes give).  A sample is a byte at `bits`
    8, a little-endian 16-bit word with the value (word >> shift) & 1023 at `bits` 10 (shift 6: P010, 0: yuv420p10le).  Luma (y, x)
    is at y_offset + y * y_pitch + x * sb; chroma sample (r, c) of Cb at cb_offset + r * chroma_pitch + c * chroma_step, of Cr the
    same from cr_offset.  `surface` builds the common cases; resolve_surface states the rules."""
    height: int
    width: int
    bits: int
    shift: int
    y_offset: int
    y_pitch: int
    cb_offset: int
    cr_offset: int
    chroma_pitch: int
    chroma_step: int

    @property
    def sample_bytes(self) -> int:
        return 2 if self.bits == 10 else 1

    @property
    def frame_bytes_min(self) -> int:
        """The end of the last plane: the fewest bytes a frame of this surface can have."""
        sb = self.sample_bytes
        c_last = (self.height // 2 - 1) * self.chroma_pitch + (self.width // 2 - 1) * self.chroma_step + sb
        return max(self.y_offset + (self.height - 1) * self.y_pitch + self.width * sb, self.cb_offset + c_last, self.cr_offset + c_last)


def surface(pixel_format, height: int, width: int, *, pitch: Optional[int] = None, rows: Optional[int] = None,
            chroma_pitch: Optional[int] = None, bits: int = 8, shift: Optional[int] = None, chroma_order: str = "uv",
            y_offset: int = 0) -> Surface:
    """The Surface of the usual allocations of `pixel_format`'s layout ("nv12" or "i420"): luma rows of `pitch` bytes (default
    W * sb), `rows` allocated luma rows (default H; a hardware decoder aligns them), chroma directly behind them at y_offset +
    pitch * rows.  "nv12": interleaved pairs, rows of `chroma_pitch` bytes (default `pitch`); "i420": two planes of (rows + 1) // 2
    rows of `chroma_pitch` bytes (default half the luma pitch, in whole samples).  `chroma_order` "vu" puts Cr first (NV21, YV12).
    `shift` defaults to 6 for "nv12" at 10 bits (P010) and to 0 otherwise (yuv420p10le).  The defaults are the compact frame."""
    layout = resolve_pixel_format(pixel_format).layout if pixel_format is not None else None
    if layout is None:
        raise ValueError("surface: packed RGB has no surface; the layout is \"nv12\" or \"i420\"")
    if chroma_order not in ("uv", "vu"):
        raise ValueError(f"surface: chroma_order {chroma_order!r} is neither \"uv\" nor \"vu\"")
    if bits not in (8, 10):
        raise ValueError(f"surface: bits {bits!r} is neither 8 nor 10")
    h, w, sb = int(height), int(width), 2 if bits == 10 else 1
    pitch = w * sb if pitch is None else int(pitch)
    rows = h if rows is None else int(rows)
    if rows < h:
        raise ValueError(f"surface: {rows} allocated rows are fewer than the frame's {h}")
    if shift is None:
        shift = 6 if bits == 10 and layout == "nv12" else 0
    c0 = int(y_offset) + pitch * rows
    if layout == "nv12":
        cp = pitch if chroma_pitch is None else int(chroma_pitch)
        first, second, step = c0, c0 + sb, 2 * sb
    else:
        cp = pitch // (2 * sb) * sb if chroma_pitch is None else int(chroma_pitch)
        first, second, step = c0, c0 + cp * ((rows + 1) // 2), sb
    cb, cr = (first, second) if chroma_order == "uv" else (second, first)
    return Surface(h, w, int(bits), int(shift), int(y_offset), pitch, cb, cr, cp, step)


def resolve_surface(surface: Surface, pixel_format, frame_bytes: int) -> Surface:
    """A Surface checked against `pixel_format`'s layout and frames of `frame_bytes` bytes, as plain ints; ValueError names the
    rule it breaks."""
    pf = resolve_pixel_format(pixel_format)
    if pf is None:
        raise ValueError("surface= describes 4:2:0 frames: it needs a pixel_format (for the layout, the matrix and the range)")
    if not isinstance(surface, Surface):
        if not isinstance(surface, (tuple, list)) or len(surface) != len(Surface._fields):
            raise ValueError(f"surface {surface!r} is not a resize.Surface {Surface._fields}")
        surface = Surface(*surface)
    try:
        sf = Surface(*(int(v) for v in surface))
    except (TypeError, ValueError):
        raise ValueError(f"surface {surface!r}: every field is an integer")
    bad = lambda rule: ValueError(f"surface {tuple(sf)}: {rule}")  # noqa: E731
    if sf.height < 2 or sf.width < 2 or sf.height % 2 or sf.width % 2:
        raise bad(f"4:2:0 frames need even H and W >= 2, got {sf.height} x {sf.width}")
    if sf.bits not in (8, 10):
        raise bad(f"bits {sf.bits} is neither 8 nor 10")
    sb = sf.sample_bytes
    if not 0 <= sf.shift <= 6 or (sf.bits == 8 and sf.shift):
        raise bad(f"shift {sf.shift} outside [0, 6], or not 0 at 8 bits")
    if min(sf.y_offset, sf.cb_offset, sf.cr_offset) < 0:
        raise bad("negative offset")
    if sf.bits == 10 and any(v % 2 for v in sf[4:] + (int(frame_bytes),)):
        raise bad(f"at 10 bits every offset, pitch and step and the frame's {frame_bytes} bytes must be even (16-bit samples)")
    if sf.y_pitch < sf.width * sb:
        raise bad(f"y_pitch {sf.y_pitch} below a row of {sf.width} samples ({sf.width * sb} bytes)")
    if sf.chroma_step not in (sb, 2 * sb):
        raise bad(f"chroma_step {sf.chroma_step} is neither {sb} (planar) nor {2 * sb} (interleaved)")
    if sf.chroma_pitch < sf.width // 2 * sf.chroma_step:
        raise bad(f"chroma_pitch {sf.chroma_pitch} shorter than a chroma row ({sf.width // 2 * sf.chroma_step} bytes)")
    if pf.layout == "nv12" and (sf.chroma_step != 2 * sb or abs(sf.cb_offset - sf.cr_offset) != sb):
        raise bad(f"contradicts pixel_format \"nv12\": interleaved chroma has chroma_step {2 * sb} and Cb, Cr offsets {sb} apart")
    if pf.layout == "i420" and sf.chroma_step != sb:
        raise bad(f"contradicts pixel_format \"i420\": planar chroma has chroma_step {sb}")
    if sf.frame_bytes_min > int(frame_bytes):
        raise bad(f"a plane ends at byte {sf.frame_bytes_min}, beyond the frame's {frame_bytes} bytes")
    return sf


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x: float) -> float:
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:  # a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (support, filter)
FILTERS = {"box": (0.5, _box), "bilinear": (1.0, _bilinear), "bicubic": (2.0, _bicubic), "lanczos": (3.0, _lanczos)}
PIL_CODES = {1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box"}  # PIL.Image.Resampling values
_REFUSED = {0: "nearest", 5: "hamming"}


def filter_name(resample: Union[int, str]) -> str:
    """A PIL resampling code (LANCZOS 1, BILINEAR 2, BICUBIC 3, BOX 4) or a lowercase name -> the filter's name."""
    if isinstance(resample, str):
        if resample in FILTERS:
            return resample
    elif isinstance(resample, (int, np.integer)) and not isinstance(resample, bool):
        if int(resample) in PIL_CODES:
            return PIL_CODES[int(resample)]
        if int(resample) in _REFUSED:
            resample = _REFUSED[int(resample)]
    raise ValueError(f"resize: resampling filter {resample!r} is not supported (box, bilinear, bicubic, lanczos or PIL codes 1-4)")


def output_size(h: int, w: int, size: Union[int, Tuple[int, int]]) -> Tuple[int, int]:
    """(out_h, out_w) of torchvision's `Resize(size)` for an (h, w) frame: an int sets the short side and scales the long
    side to int(size * long / short) (a frame already at that size stays as it is); an (h, w) pair is used as given."""
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"resize: size must be an int or (h, w), got {size!r}")
        oh, ow = int(size[0]), int(size[1])
    else:
        size = int(size)
        short, long = (w, h) if w <= h else (h, w)
        if short == size:
            return h, w
        new_short, new_long = size, int(size * long / short)
        ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    if oh < 1 or ow < 1:
        raise ValueError(f"resize: output size ({oh}, {ow}) must be at least 1 x 1")
    return oh, ow


def coefficients(in_size: int, out_size: int, resample: Union[int, str] = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's tables for one axis: bounds int32 (out, 2) = (first source index, tap count) and the 2**22 fixed-point
    coefficients int32 (out, ksize), zero past each output's tap count."""
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize: sizes must be >= 1 (in {in_size}, out {out_size})")
    return _coefficients(in_size, 0.0, float(in_size) / out_size, out_size, resample)


def box_coefficients(in_size: int, in0: float, in1: float, out_size: int,
                     resample: Union[int, str] = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """`coefficients` for the source interval [in0, in1) of an axis of `in_size` samples: Pillow's `precompute_coeffs` with a
    box (`Image.resize(..., box=)`), in the shape `coefficients` returns.  Pillow holds the box as C floats, so the order of the
    roundings is part of the rule: in0 and in1 are rounded to float32 first, the extent in1 - in0 is subtracted IN float32, and
    only then scale = double(extent) / out_size; everything behind that is `coefficients`' double arithmetic with the centres
    moved by in0.  box_coefficients(n, 0, n, m) is coefficients(n, m)."""
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize: sizes must be >= 1 (in {in_size}, out {out_size})")
    lo, hi = np.float32(in0), np.float32(in1)
    extent = np.float32(hi - lo)
    if not (np.isfinite(lo) and np.isfinite(hi)) or lo < 0 or hi > in_size or not extent > 0:
        raise ValueError(f"resize: the interval [{in0!r}, {in1!r}) is not a non-empty part of [0, {in_size}] (as float32: [{lo!r}, {hi!r}))")
    return _coefficients(in_size, float(lo), float(extent) / out_size, out_size, resample)


def _coefficients(in_size: int, in0: float, scale: float, out_size: int, resample) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc in double: output i is centred at in0 + (i + 0.5) * scale."""
    support0, filt = FILTERS[filter_name(resample)]
    fs = max(scale, 1.0)
    support = support0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for i in range(out_size):
        center = in0 + (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((j + xmin - center + 0.5) * ss) for j in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[i] = (xmin, n)
        coef[i, :n] = [int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w]
    return bounds, coef


class Plan(NamedTuple):
    """Host tables of one resize (in_h, in_w) -> (out_h, out_w): which passes run, and each axis' tables.  The horizontal
    pass computes source rows [row0, row0 + rows) only (the rows the vertical pass reads)."""
    out_h: int
    out_w: int
    horizontal: bool
    vertical: bool
    xbounds: np.ndarray
    xcoef: np.ndarray
    ybounds: np.ndarray
    ycoef: np.ndarray
    row0: int
    rows: int


def plan(in_h: int, in_w: int, out_h: int, out_w: int, resample: Union[int, str] = "bilinear") -> Plan:
    xb, xk = coefficients(in_w, out_w, resample)
    yb, yk = coefficients(in_h, out_h, resample)
    row0 = int(yb[0, 0])
    rows = int(yb[-1, 0] + yb[-1, 1]) - row0
    return Plan(out_h, out_w, out_w != in_w, out_h != in_h, xb, xk, yb, yk, row0, rows)


class _Tables(NamedTuple):
    plan: Plan
    buf: torch.Tensor  # int32 [xbounds | xcoef | ybounds | ycoef] on the device
    offsets: Tuple[int, int, int, int]


_TABLES: Dict[tuple, _Tables] = {}


def tables(in_h: int, in_w: int, out_h: int, out_w: int, resample: Union[int, str], device: torch.device) -> _Tables:
    """The device tables of one resize, built on the current stream on first use and cached per
    (in_h, in_w, out_h, out_w, filter, device) (like the conv gather tables: a caller about to fork streams builds them first)."""
    key = (in_h, in_w, out_h, out_w, filter_name(resample), torch.device(device))
    t = _TABLES.get(key)
    if t is None:
        p = plan(in_h, in_w, out_h, out_w, resample)
        parts = [p.xbounds, p.xcoef, p.ybounds, p.ycoef]
        offsets = tuple(int(o) for o in np.cumsum([0] + [a.size for a in parts[:-1]]))
        host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in parts]))
        if host.device.type == "cpu" and torch.cuda.is_available():
            host = host.pin_memory()  # an asynchronous copy on the current stream (the pinned block outlives it)
        buf = host.to(device, non_blocking=True)
        t = _TABLES[key] = _Tables(p, buf, offsets)
    return t


# ---- regions of interest: a source box per frame (PIL Image.resize(size, resample, box=(l, t, r, b))) ---------------------------

def resolve_box(who: str, box, in_h: int, in_w: int) -> Tuple[float, float, float, float]:
    """`box` = (left, top, right, bottom) in source pixels, as Pillow's `box=` -> the four numbers as Pillow holds them (float32
    values, as Python floats); None is the whole frame.  Refused by name: anything but four finite host numbers, a box that
    leaves the frame (Pillow raises too) and an extent that is not positive after the float32 rounding."""
    if box is None:
        return 0.0, 0.0, float(in_w), float(in_h)
    if torch.is_tensor(box) or isinstance(box, (str, bytes)) or not hasattr(box, "__len__") or len(box) != 4:
        raise ValueError(f"{who}: box {box!r} is not (left, top, right, bottom): four host numbers")
    for v in box:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"{who}: box {tuple(box)!r}: {v!r} is not a finite host number")
    l, t, r, b = (np.float32(v) for v in box)
    if l < 0 or t < 0 or r > in_w or b > in_h:
        raise ValueError(f"{who}: box {tuple(box)!r} leaves the {in_h} x {in_w} frame (left, top >= 0, right <= {in_w}, bottom <= {in_h})")
    if not np.float32(r - l) > 0 or not np.float32(b - t) > 0:
        raise ValueError(f"{who}: box {tuple(box)!r} is empty: right - left and bottom - top must be positive in float32")
    return float(l), float(t), float(r), float(b)


def box_output_size(box, size: Union[int, Tuple[int, int]]) -> Tuple[int, int]:
    """`output_size`'s rule on a box: an (h, w) pair is used as given; an int sets the short side of the box's extents (bottom -
    top, right - left; float32 values subtracted in float32, as the tables see them) and scales the long side to int(size * long /
    short)."""
    if isinstance(size, (tuple, list)):
        return output_size(1, 1, size)
    l, t, r, b = (np.float32(v) for v in box)
    h, w = float(np.float32(b - t)), float(np.float32(r - l))
    if not (h > 0 and w > 0):
        raise ValueError(f"resize: box {tuple(box)!r} is empty")
    size = int(size)
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(size * long / short)
    oh, ow = (new_long, size) if w <= h else (size, new_long)
    if oh < 1 or ow < 1:
        raise ValueError(f"resize: output size ({oh}, {ow}) must be at least 1 x 1")
    return oh, ow


def _identity(n: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of an axis Pillow does not resample: output i is source i, with the coefficient 1."""
    return (np.stack([np.arange(n), np.ones(n, dtype=np.int64)], axis=1).astype(np.int32),
            np.full((n, 1), 1 << PRECISION_BITS, dtype=np.int32))


def box_plan(in_h: int, in_w: int, out_h: int, out_w: int, box=None, resample: Union[int, str] = "bilinear") -> Plan:
    """`plan` with a box: Pillow's pass rule (the horizontal pass iff out_w != in_w or left != 0 or right != in_w, the vertical
    one iff out_h != in_h or top != 0 or bottom != in_h), box_coefficients for an axis that is resampled and the explicit
    identity table for one that is not.  row0 / rows: the source rows the vertical table reads."""
    l, t, r, b = resolve_box("resize", box, in_h, in_w)
    if out_h < 1 or out_w < 1:
        raise ValueError(f"resize: output size ({out_h}, {out_w}) must be at least 1 x 1")
    horizontal = out_w != in_w or l != 0 or r != in_w
    vertical = out_h != in_h or t != 0 or b != in_h
    xb, xk = box_coefficients(in_w, l, r, out_w, resample) if horizontal else _identity(in_w)
    yb, yk = box_coefficients(in_h, t, b, out_h, resample) if vertical else _identity(in_h)
    filter_name(resample)  # (refused even where both tables are identities)
    row0 = int(yb[0, 0])
    return Plan(out_h, out_w, horizontal, vertical, xb, xk, yb, yk, row0, int(yb[-1, 0] + yb[-1, 1]) - row0)


class RoiTables(NamedTuple):
    """K stacked table sets for frames of one geometry and one output size, one per box, on the device (roi_tables).  Every set
    has both axes (box_plan's identity where Pillow skips a pass), each axis padded with zero coefficients to the largest ksize
    of that axis over the K boxes.  The host arrays are kept for whoever wants to look: xbounds (K, OW, 2), xcoef (K, OW,
    xksize), ybounds (K, OH, 2), ycoef (K, OH, yksize), rowspan (K, 2) = (row0, rows) of each set's horizontal pass."""
    in_h: int
    in_w: int
    out_h: int
    out_w: int
    boxes: Tuple[Tuple[float, float, float, float], ...]
    resample: str
    xbounds: np.ndarray
    xcoef: np.ndarray
    ybounds: np.ndarray
    ycoef: np.ndarray
    rowspan: np.ndarray
    ws_rows: int  # max rows: the rows per frame of the workspace between the passes
    buf: torch.Tensor  # int32 [xbounds | xcoef | ybounds | ycoef | rowspan] on the device
    offsets: Tuple[int, int, int, int, int]

    @property
    def n_tables(self) -> int:
        return len(self.boxes)


def roi_tables(in_h: int, in_w: int, out_hw, boxes, resample: Union[int, str] = "bilinear", device="cuda") -> RoiTables:
    """The stacked device tables of K >= 1 boxes of (in_h, in_w) frames, all resized to `out_hw` = (h, w) (box_output_size gives
    the pair of an int size): one upload on the current stream, from pinned memory, as `tables` does.  `boxes`: a sequence of
    (left, top, right, bottom) boxes; None stands for the whole frame."""
    in_h, in_w = int(in_h), int(in_w)
    if in_h < 1 or in_w < 1:
        raise ValueError(f"roi_tables: frames of {in_h} x {in_w}")
    if not isinstance(out_hw, (tuple, list)) or len(out_hw) != 2:
        raise ValueError(f"roi_tables: out_hw {out_hw!r} is not an (h, w) pair (box_output_size gives the pair of an int size)")
    oh, ow = output_size(in_h, in_w, tuple(out_hw))
    name = filter_name(resample)
    if boxes is None or isinstance(boxes, (str, bytes)) or torch.is_tensor(boxes) or not hasattr(boxes, "__len__") or len(boxes) < 1:
        raise ValueError(f"roi_tables: boxes must be a sequence of at least one box (None: the whole frame), got {boxes!r}")
    resolved = tuple(resolve_box("roi_tables", bx, in_h, in_w) for bx in boxes)  # (every refusal before any table is built)
    distinct = {bx: box_plan(in_h, in_w, oh, ow, bx, name) for bx in dict.fromkeys(resolved)}  # (many cameras often share a few boxes)
    plans = [distinct[bx] for bx in resolved]
    kx, ky = max(p.xcoef.shape[1] for p in plans), max(p.ycoef.shape[1] for p in plans)
    pad = lambda k, n: np.pad(k, ((0, 0), (0, n - k.shape[1])))  # noqa: E731
    xb, yb = np.stack([p.xbounds for p in plans]), np.stack([p.ybounds for p in plans])
    xk, yk = np.stack([pad(p.xcoef, kx) for p in plans]), np.stack([pad(p.ycoef, ky) for p in plans])
    rowspan = np.array([(p.row0, p.rows) for p in plans], dtype=np.int32)
    parts = [xb, xk, yb, yk, rowspan]
    offsets = tuple(int(o) for o in np.cumsum([0] + [a.size for a in parts[:-1]]))
    host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in parts]).astype(np.int32))
    if torch.cuda.is_available():
        host = host.pin_memory()  # an asynchronous copy on the current stream (the pinned block outlives it)
    return RoiTables(in_h, in_w, oh, ow, resolved, name, xb, xk, yb, yk, rowspan, int(rowspan[:, 1].max()), host.to(device, non_blocking=True), offsets)


class RoiSpec(NamedTuple):
    """What LiveFrames(rois=) takes: the geometry (H, W) of the cameras' decoded frames and a box per camera -- a sequence of
    n_cameras boxes or a {camera: box} dict; a camera without one (None, or absent from the dict) gets the whole frame."""
    source_hw: Tuple[int, int]
    boxes: object
    resample: Union[int, str] = "bilinear"


_ROI_TABLES: Dict[tuple, RoiTables] = {}


def _box_tables(in_h: int, in_w: int, oh: int, ow: int, box, name: str, device: torch.device) -> RoiTables:
    """The one-box RoiTables of resize_u8(box=), cached per (geometry, box, filter, device) as `tables` caches."""
    key = (in_h, in_w, oh, ow, box, name, torch.device(device))
    t = _ROI_TABLES.get(key)
    if t is None:
        t = _ROI_TABLES[key] = roi_tables(in_h, in_w, (oh, ow), [box], name, device)
    return t


def _index_vector(who: str, name: str, v, device) -> Optional[torch.Tensor]:
    """`table_of` / `src_of`: None, an int32 device vector, or a host sequence of ints (uploaded once, here)."""
    if v is None:
        return None
    if torch.is_tensor(v):
        if v.dtype != torch.int32 or v.dim() != 1 or not v.is_contiguous() or v.device != device or v.numel() < 1:
            raise HipExtensionError(f"{who}: {name} must be a contiguous int32 vector on {device}, got {v.dtype} {tuple(v.shape)} on {v.device}")
        return v
    try:
        host = [int(i) for i in v if not isinstance(i, bool) and float(i).is_integer()]
        ok = len(host) == len(v) >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok or any(not -(1 << 31) <= i < 1 << 31 for i in host):
        raise HipExtensionError(f"{who}: {name} must be a non-empty sequence of host integers or an int32 device vector, got {v!r}")
    return torch.tensor(host, dtype=torch.int32).to(device, non_blocking=True)


def resize_rois_u8(frames: torch.Tensor, rois: RoiTables, table_of=None, src_of=None, frame_step: Optional[int] = None,
                   out: Optional[torch.Tensor] = None, pixel_format=None, surface: Optional[Surface] = None,
                   ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frames on the GPU in any form resize_u8 takes -> uint8 (N, OH, OW, 3): output frame i is PIL's
    `Image.resize((OW, OH), resample, box=rois.boxes[table_of[i]])` of source frame src_of[i], bit for bit, in two launches on
    the current stream whatever the boxes are (advhip_resize_roi_u8 and its 4:2:0 forms).  `table_of` / `src_of`: int32 device
    vectors, or host sequences (uploaded here, once); without `table_of` every frame uses table 0, without `src_of` output i reads
    source frame i * frame_step.  N is their length, else the sampled frame count ceil(F / frame_step).  An output frame whose
    source or table index is out of range is left as it is.  `out` as in resize_u8; `ws`: a caller-owned uint8 workspace of at
    least N * rois.ws_rows * OW * 3 bytes (default: allocated here)."""
    who = "resize_rois_u8"
    if not isinstance(rois, RoiTables):
        raise HipExtensionError(f"{who}: rois must be a RoiTables (resize.roi_tables), got {type(rois).__name__}")
    d = _frame_step(who, frame_step)
    pf = resolve_pixel_format(pixel_format)
    if pf is None and surface is not None:
        raise ValueError(f"{who}: surface= describes 4:2:0 frames and needs a pixel_format")
    src = _source(who, frames, pf, surface)
    if (src.H, src.W) != (rois.in_h, rois.in_w):
        raise HipExtensionError(f"{who}: the tables are for {rois.in_h} x {rois.in_w} frames, these are {src.H} x {src.W}")
    if rois.buf.device != frames.device:
        raise HipExtensionError(f"{who}: the tables are on {rois.buf.device}, the frames on {frames.device}")
    table_of = _index_vector(who, "table_of", table_of, frames.device)
    src_of = _index_vector(who, "src_of", src_of, frames.device)
    if src_of is not None and frame_step is not None:
        raise ValueError(f"{who}: src_of names every source frame itself: frame_step has no meaning next to it")
    if table_of is not None and src_of is not None and table_of.numel() != src_of.numel():
        raise HipExtensionError(f"{who}: table_of has {table_of.numel()} entries, src_of {src_of.numel()}")
    N = src_of.numel() if src_of is not None else table_of.numel() if table_of is not None else -(-src.F_src // d)
    if src_of is None and (N - 1) * d >= src.F_src:
        raise HipExtensionError(f"{who}: table_of has {N} entries, but {src.F_src} frames at frame_step {d} are {-(-src.F_src // d)}")
    oh, ow = rois.out_h, rois.out_w
    if out is None:
        out = torch.empty((N, oh, ow, 3), device=frames.device, dtype=torch.uint8)
    else:
        _check_out(who, frames, out, (N, oh, ow, 3))
    ws_bytes = N * rois.ws_rows * ow * 3
    if ws is None:
        ws = torch.empty((ws_bytes,), device=frames.device, dtype=torch.uint8)
    elif ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < ws_bytes or ws.device != frames.device:
        raise HipExtensionError(f"{who}: ws must be a contiguous uint8 tensor of at least {ws_bytes} bytes on {frames.device}")
    b, (o_xb, o_xk, o_yb, o_yk, o_rs) = rois.buf, rois.offsets
    fn = getattr(_lib.load(), src.resize_roi)
    check(fn(ptr(frames), ptr(out), ptr(ws), src.F_src, N, ptr(src_of), d, ptr(table_of), rois.n_tables, *src.before, src.H, src.W, 3, oh, ow,
             ptr(b[o_xb:]), ptr(b[o_xk:]), rois.xcoef.shape[2], ptr(b[o_yb:]), ptr(b[o_yk:]), rois.ycoef.shape[2], ptr(b[o_rs:]), rois.ws_rows,
             *src.after, stream(frames)), who)
    return out


def _check_out(who: str, frames: torch.Tensor, out: torch.Tensor, shape: tuple) -> None:
    require_gpu(frames, out)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape:
        raise HipExtensionError(f"{who}: out must be uint8 {shape}, got {out.dtype} {tuple(out.shape)}")
    a0, a1 = frames.data_ptr(), frames.data_ptr() + frames.numel()
    if out.data_ptr() < a1 and a0 < out.data_ptr() + out.numel():
        raise HipExtensionError(f"{who}: out overlaps the input frames")


def _frame_step(who: str, frame_step) -> int:
    d = 1 if frame_step is None else int(frame_step)
    if d < 1:
        raise ValueError(f"{who}: frame_step {frame_step!r} must be an integer >= 1")
    return d


class _Source(NamedTuple):
    """What `frames` are: their sizes, the entry points of that kind of frame (`convert` is None for packed RGB, which has
    nothing to convert) and the arguments those take before (H, W) and behind the resize arguments."""
    F_src: int
    H: int
    W: int
    convert: Optional[str]
    resize: str
    resize_roi: str
    before: tuple
    after: tuple


def _source(who: str, frames: torch.Tensor, pf: Optional[PixelFormat], surface) -> _Source:
    """Packed RGB (F, H, W, 3) (`pf` None), compact 4:2:0 frames (F, 3H/2, W) or surfaces (F, frame_bytes): uint8, on the GPU."""
    require_gpu(frames)
    if pf is None:
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise HipExtensionError(f"{who} wants uint8 (F,H,W,3) RGB frames, got {frames.dtype} {tuple(frames.shape)}")
        return _Source(*frames.shape[:3], None, "advhip_resize_u8_sampled", "advhip_resize_roi_u8", (), ())
    if surface is None:
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise HipExtensionError(f"{who} wants uint8 (F, 3H/2, W) {pf.layout} frames, got {frames.dtype} {tuple(frames.shape)}")
        h, w = frame_hw(frames.shape)
        return _Source(frames.shape[0], h, w, "advhip_yuv420_to_rgb_u8", "advhip_resize_yuv420_u8", "advhip_resize_roi_yuv420_u8", (),
                       (LAYOUTS[pf.layout],) + yuv_coefficients(pf))
    if frames.dtype != torch.uint8 or frames.dim() != 2:
        raise HipExtensionError(f"{who} with surface= wants uint8 (F, frame_bytes) frames, got {frames.dtype} {tuple(frames.shape)}")
    sf = resolve_surface(surface, pf, frames.shape[1])
    geometry = (sf.bits, sf.shift, sf.y_offset, sf.y_pitch, sf.cb_offset, sf.cr_offset, sf.chroma_pitch, sf.chroma_step)
    return _Source(frames.shape[0], sf.height, sf.width, "advhip_yuv420_surface_to_rgb_u8", "advhip_resize_yuv420_surface_u8", "advhip_resize_roi_surface_u8",
                   (frames.shape[1],),
                   geometry + yuv_coefficients(pf, sf.bits))


def yuv420_to_rgb_u8(frames: torch.Tensor, pixel_format, out: Optional[torch.Tensor] = None,
                     frame_step: Optional[int] = None, surface: Optional[Surface] = None) -> torch.Tensor:
    """uint8 (F, 3H/2, W) 4:2:0 frames on the GPU (NV12 or I420, see resolve_pixel_format) -> packed RGB (F', H, W, 3), one
    launch on the current stream: the integer conversion of `yuv_coefficients` with nearest chroma (pixel (y, x) uses chroma
    sample (y >> 1, x >> 1)).  `frame_step` d: source frames 0, d, 2 d, ... only, F' = ceil(F / d).  `out` as in resize_u8.
    Not ffmpeg swscale's bytes (the module docstring): the contract is the formula.
    `surface` (a Surface; default None = the compact frames above): `frames` are uint8 (F, frame_bytes), each frame laid out as
    the surface says and read in place -- pitch, offsets, chroma order and 10-bit samples included (advhip_yuv420_surface_to_rgb_u8)."""
    pf = resolve_pixel_format(pixel_format)
    if pf is None:
        raise ValueError("yuv420_to_rgb_u8: pixel_format None is packed RGB, there is nothing to convert")
    d = _frame_step("yuv420_to_rgb_u8", frame_step)
    src = _source("yuv420_to_rgb_u8", frames, pf, surface)
    shape = (-(-src.F_src // d), src.H, src.W, 3)
    if out is None:
        out = torch.empty(shape, device=frames.device, dtype=torch.uint8)
    else:
        _check_out("yuv420_to_rgb_u8", frames, out, shape)
    check(getattr(_lib.load(), src.convert)(ptr(frames), ptr(out), src.F_src, d, *src.before, src.H, src.W, *src.after, stream(frames)),
          "yuv420_to_rgb_u8")
    return out


def resize_u8(frames: torch.Tensor, size: Union[int, Tuple[int, int]] = 256, resample: Union[int, str] = "bilinear",
              out: Optional[torch.Tensor] = None, frame_step: Optional[int] = None, pixel_format=None,
              surface: Optional[Surface] = None, box=None) -> torch.Tensor:
    """uint8 (F, H, W, 3) frames on the GPU -> (F, OH, OW, 3), what `GroupResize(size, resample)` gives frame by frame (PIL
    `Image.resize`, bit for bit), on the current stream with no host synchronisation.  `out` places the result in a
    caller-owned contiguous (F, OH, OW, 3) uint8 tensor (e.g. a view of a larger buffer).  Without `out`, frames already at
    the output size are returned as they are (torchvision returns the image itself).
    `frame_step` d (default 1): only source frames 0, d, 2 d, ... are resized, into a compact (ceil(F / d), OH, OW, 3) result --
    resize_u8(frames[::d].contiguous()) byte for byte, read in place (a source frame pitch in the kernels; the workspace holds
    the sampled frames only).  Frames already at the output size come back as the view frames[::d] (without `out`).
    `pixel_format` (resolve_pixel_format; default None = packed RGB): `frames` are 4:2:0 frames (F, 3H/2, W) and the result is
    resize_u8(yuv420_to_rgb_u8(frames, pixel_format), ...) byte for byte without the full-size RGB frames: the horizontal pass
    converts each tap's pixel as it reads it.  Frames already at the output size come back converted.
    `surface` (with `pixel_format`; default None = the compact frames): `frames` are uint8 (F, frame_bytes) decoder surfaces, as
    in yuv420_to_rgb_u8, and the result is again resize_u8(yuv420_to_rgb_u8(frames, pixel_format, surface=surface), ...).
    `box` (left, top, right, bottom) in source pixels, floats allowed (default None = this call as it always was): every frame is
    PIL's `Image.resize(size, resample, box=box)` bit for bit, taps at the box's edge reading the pixels beside it, from any of
    the source forms above and with `frame_step`.  An int `size` is the short side of the box (box_output_size).  One table set
    through resize_rois_u8's entry points, cached per (geometry, box, filter, device); always a new tensor (or `out`)."""
    d = _frame_step("resize_u8", frame_step)
    pf = resolve_pixel_format(pixel_format)
    if pf is None and surface is not None:
        raise ValueError("resize_u8: surface= describes 4:2:0 frames and needs a pixel_format")
    src = _source("resize_u8", frames, pf, surface)
    F, H, W, yuv = -(-src.F_src // d), src.H, src.W, pf is not None
    name = filter_name(resample)
    if box is not None:
        box = resolve_box("resize_u8", box, H, W)
        oh, ow = box_output_size(box, size)
        return resize_rois_u8(frames, _box_tables(H, W, oh, ow, box, name, frames.device), frame_step=d, out=out, pixel_format=pf, surface=surface)
    oh, ow = output_size(H, W, size)
    if out is None:
        if not yuv and (oh, ow) == (H, W):  # (4:2:0 frames always come back converted)
            return frames if d == 1 else frames[::d]
        out = torch.empty((F, oh, ow, 3), device=frames.device, dtype=torch.uint8)
    else:
        _check_out("resize_u8", frames, out, (F, oh, ow, 3))
    t = tables(H, W, oh, ow, name, frames.device)
    p, b, (o_xb, o_xk, o_yb, o_yk) = t.plan, t.buf, t.offsets
    ws = None
    if p.vertical and (p.horizontal or yuv):  # the horizontal pass's rows, or (a vertical-only resize of 4:2:0) the converted frames
        ws = torch.empty((F * p.rows * ow * 3 if p.horizontal else F * H * W * 3,), device=frames.device, dtype=torch.uint8)
    resize_args = (3, oh, ow, ptr(b[o_xb:]), ptr(b[o_xk:]), p.xcoef.shape[1], ptr(b[o_yb:]), ptr(b[o_yk:]), p.ycoef.shape[1], p.row0, p.rows)
    check(getattr(_lib.load(), src.resize)(ptr(frames), ptr(out), ptr(ws), src.F_src, d, *src.before, H, W, *resize_args, *src.after, stream(frames)),
          "resize_u8")
    return out
