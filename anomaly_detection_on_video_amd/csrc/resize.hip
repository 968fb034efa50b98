// GroupResize on the device (src/gtransforms.py:9-18 of the reference, src/dataset.py:175-183): Pillow's 8-bit two-pass
// resampler (Resample.c, ImagingResampleInner) on uint8 (F, H, W, 3) frames.  The tables (bounds + 2^22 fixed-point
// coefficients per output index) come from the host (resize.py); each pass is clamp((2^21 + sum pixel * coef) >> 22, 0, 255)
// in int32, so the result is Pillow's byte for byte.  Integer VALU work with the lanes along the output row: the pass is a
// few microseconds of memory traffic per clip, so neither LDS staging nor a fusion with the TenCrop pass is worth its code.
#include <algorithm>

#include "common.h"

namespace advhip {

constexpr int RESIZE_BITS = 22;

__device__ __forceinline__ uint8_t clip8(int s) {
  s >>= RESIZE_BITS;  // arithmetic shift, as Pillow's clip8
  return (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// The pass bodies: what one wave does with the row it was given.  The kernels differ in how a row finds its source frame and its
// tables only -- one table set and a frame pitch (the three kernels below), or a lookup per output frame (the roi kernels) -- so
// each body is written once and inlined into both.

// One row of the horizontal pass: out pixel x < OW <- the taps of source row `in` (W pixels) that xb / xk name; a lane per output
// pixel (three channels).  Bounds and coefficients of a pixel are read once for its three channels.
__device__ __forceinline__ void resize_h_row(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int W, int OW, const int* __restrict__ xb,
                                             const int* __restrict__ xk, int ksize, int lane) {
  for (int x = lane; x < OW; x += 64) {
    const int x0 = xb[2 * x];
    int n = min(xb[2 * x + 1], ksize);
    if (x0 < 0 || x0 + n > W) n = 0;  // (never for tables from resize.py: a guard against a foreign table)
    const int* k = xk + (long long)x * ksize;
    const uint8_t* p = in + x0 * 3;
    int s0 = 1 << (RESIZE_BITS - 1), s1 = s0, s2 = s0;
    for (int j = 0; j < n; ++j) {
      const int w = k[j];
      s0 += (int)p[3 * j] * w;
      s1 += (int)p[3 * j + 1] * w;
      s2 += (int)p[3 * j + 2] * w;
    }
    out[3 * x] = clip8(s0);
    out[3 * x + 1] = clip8(s1);
    out[3 * x + 2] = clip8(s2);
  }
}

// One row of the vertical pass: out byte q < rowbytes <- n rows of rowbytes bytes from `in` on, with the row's coefficients k (the
// same for every lane); a lane per output byte.
__device__ __forceinline__ void resize_v_row(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int rowbytes, const int* __restrict__ k, int n,
                                             int lane) {
  for (int q = lane; q < rowbytes; q += 64) {
    int s = 1 << (RESIZE_BITS - 1);
    for (int j = 0; j < n; ++j) s += (int)in[(long long)j * rowbytes + q] * k[j];
    out[q] = clip8(s);
  }
}

// Horizontal pass: dst row r = (f, y) of `rows` rows per frame <- src row (f, row0 + y); one wave per output row.  Output frame f
// reads the source frame at byte f * fpitch: H * W * 3 for every frame, frame_step times that for every frame_step-th one.
__global__ __launch_bounds__(256) void resize_h_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int W,
                                                         int OW, int row0, int rows, const int* __restrict__ xb,
                                                         const int* __restrict__ xk, int ksize, long long nrows) {
  const int lane = threadIdx.x & 63;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / rows;
    const int y = (int)(r - f * rows);
    const uint8_t* in = src + f * fpitch + (row0 + y) * (long long)W * 3;
    uint8_t* out = dst + r * OW * 3;
    resize_h_row(in, out, W, OW, xb, xk, ksize, lane);
  }
}

// Vertical pass: dst row (f, oy) <- rows [yb[oy].first - ybase, + count) of the IH-row source frame f; one wave per output row.
// Source frame f starts at byte f * fpitch.
__global__ __launch_bounds__(256) void resize_v_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int IH, int OH,
                                                         int rowbytes, int ybase, const int* __restrict__ yb,
                                                         const int* __restrict__ yk, int ksize, long long nrows) {
  const int lane = threadIdx.x & 63;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / OH;
    const int oy = (int)(r - f * OH);
    const int y0 = yb[2 * oy] - ybase;
    int n = min(yb[2 * oy + 1], ksize);
    if (y0 < 0 || y0 + n > IH) n = 0;  // (as above)
    const int* k = yk + (long long)oy * ksize;
    const uint8_t* in = src + f * fpitch + y0 * (long long)rowbytes;
    uint8_t* out = dst + r * rowbytes;
    resize_v_row(in, out, rowbytes, k, n, lane);
  }
}

// --- regions of interest: a table set per output frame (include/advhip.h).  The tables of set t start t * OW (or OH) entries into
// the stacked arrays; rowspan[t] = (row0, rows) are the source rows its vertical table reads.  Where a row's frame is, which set it
// uses and whether it is computed at all is decided once per row and is the same for the whole wave.
struct RoiArgs {
  const int *src_of, *table_of, *rowspan;  // device; the first two may be null
  long long F_src, N;
  int frame_step, n_tables, H, ws_rows;
};

struct RoiFrame {
  long long src;  // the source frame
  int table, row0, rows;
  bool ok;  // both indices in range: the frame is computed
};

__device__ __forceinline__ RoiFrame roi_frame(const RoiArgs& A, long long i) {
  RoiFrame f;
  f.src = A.src_of ? (long long)A.src_of[i] : i * A.frame_step;
  f.table = A.table_of ? A.table_of[i] : 0;
  f.ok = f.src >= 0 && f.src < A.F_src && f.table >= 0 && f.table < A.n_tables;
  f.row0 = f.rows = 0;
  if (f.ok) {
    f.row0 = A.rowspan[2 * f.table], f.rows = A.rowspan[2 * f.table + 1];
    // (never for tables from resize.py: rowspan is device memory the host cannot check, so a span outside the frame or the
    // workspace counts no rows here and no taps in the vertical pass)
    if (f.row0 < 0 || f.rows < 0 || f.rows > A.ws_rows || f.row0 > A.H - f.rows) f.rows = 0;
  }
  return f;
}

// the row of this wave, the same number in every lane and known to be so
__device__ __forceinline__ long long wave_row() { return (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Horizontal pass with a table set per frame: ws row (i, y), y < rows of frame i's set <- row row0 + y of its source frame.  The
// workspace is (N, ws_rows, OW, 3); a frame's slab is written from its first row on.
__global__ __launch_bounds__(256) void resize_h_roi_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ ws, RoiArgs A, int W, int OW,
                                                             const int* __restrict__ xb, const int* __restrict__ xk, int ksize) {
  const int lane = threadIdx.x & 63;
  const long long nrows = A.N * A.ws_rows;
  for (long long r = wave_row(); r < nrows; r += (long long)gridDim.x * 4) {
    const long long i = r / A.ws_rows;
    const int y = (int)(r - i * A.ws_rows);
    const RoiFrame f = roi_frame(A, i);
    if (!f.ok || y >= f.rows) continue;
    const uint8_t* in = src + (f.src * A.H + f.row0 + y) * (long long)W * 3;
    resize_h_row(in, ws + r * OW * 3, W, OW, xb + (long long)f.table * OW * 2, xk + (long long)f.table * OW * ksize, ksize, lane);
  }
}

// Vertical pass with a table set per frame: dst row (i, oy) <- rows [yb[oy].first - row0, + count) of the `rows` rows of frame i's
// slab of the workspace.
__global__ __launch_bounds__(256) void resize_v_roi_u8_kernel(const uint8_t* __restrict__ ws, uint8_t* __restrict__ dst, RoiArgs A, int OH, int rowbytes,
                                                             const int* __restrict__ yb, const int* __restrict__ yk, int ksize) {
  const int lane = threadIdx.x & 63;
  const long long nrows = A.N * OH;
  for (long long r = wave_row(); r < nrows; r += (long long)gridDim.x * 4) {
    const long long i = r / OH;
    const int oy = (int)(r - i * OH);
    const RoiFrame f = roi_frame(A, i);
    if (!f.ok) continue;
    const int* b = yb + ((long long)f.table * OH + oy) * 2;
    const int y0 = b[0] - f.row0;
    int n = min(b[1], ksize);
    if (y0 < 0 || y0 + n > f.rows) n = 0;  // (as above)
    const int* k = yk + ((long long)f.table * OH + oy) * ksize;
    resize_v_row(ws + (i * A.ws_rows + y0) * (long long)rowbytes, dst + r * rowbytes, rowbytes, k, n, lane);
  }
}

// --- Y'CbCr 4:2:0 frames (NV12 / I420), uint8 (F, 3H/2, W): rows [0, H) are Y; NV12 then holds H/2 rows of interleaved (Cb, Cr)
// pairs, I420 the (H/2, W/2) Cb plane followed by the Cr plane.  Pixel (y, x) uses chroma sample (y >> 1, x >> 1) (nearest).  The
// conversion is the integer formula of include/advhip.h with the caller's 2^16 fixed-point coefficients, all in int32.
struct YuvCoef {
  int yoff, cy, crv, cgu, cgv, cbu;
};

// the three chroma terms of a sample, formed once for the pixels that share it (BITS: the sample depth, 8 or 10; the chroma
// midpoint is 2^(BITS - 1) and the coefficients are 2^(8 + BITS) fixed point)
template <int BITS>
struct ChromaTerms {
  int rv, guv, bu;
  __device__ __forceinline__ ChromaTerms(int cb, int cr, const YuvCoef& k)
      : rv(k.crv * (cr - (1 << (BITS - 1)))),
        guv(-k.cgu * (cb - (1 << (BITS - 1))) - k.cgv * (cr - (1 << (BITS - 1)))),
        bu(k.cbu * (cb - (1 << (BITS - 1)))) {}
};

// clip8(v >> S) with the arithmetic shift of the definition: below 0 -> 0, from 2^(8 + S) on -> 255 (S = 16 at 8 bits, 18 at 10
// bits).  The clamp comes BEFORE the shift on purpose.  Written as clamp(v >> 16, 0, 255), two of these OR-ed into one word became
// gfx950's v_ashr_pk_u8_i32 with ROCm 7.2.0 (AMD clang 22.0.0git, roc-7.2.0), into a register that still held a 32-bit sum; on the
// MI355X the bytes OR-ed in above its 16-bit result then came out as that sum's high half, so the instruction kept it where the
// compiler counted on zero.  Observed with that compiler only, and another one may fuse this form as well: tests/test_hip_yuv420.py's
// test_conversion_is_the_restatement_for_every_triple (every triple, clamped ones included, through the packing kernel) is the guard,
// and the every-value tests of tests/test_hip_surface.py are the guard of the surface kernels' instantiations.
template <int S>
__device__ __forceinline__ int sat8_shr(int v) {
  return min(max(v, 0), (1 << (8 + S)) - 1) >> S;
}

template <int BITS>
__device__ __forceinline__ void yuv_rgb(int y, const ChromaTerms<BITS>& c, const YuvCoef& k, int& r, int& g, int& b) {
  constexpr int S = 8 + BITS;
  const int yi = k.cy * (y - k.yoff) + (1 << (S - 1));
  r = sat8_shr<S>(yi + c.rv);
  g = sat8_shr<S>(yi + c.guv);
  b = sat8_shr<S>(yi + c.bu);
}

// R | G << 8 | B << 16
template <int BITS>
__device__ __forceinline__ uint32_t yuv_rgb_packed(int y, const ChromaTerms<BITS>& c, const YuvCoef& k) {
  int r, g, b;
  yuv_rgb(y, c, k, r, g, b);
  return (uint32_t)(r | g << 8 | b << 16);
}

template <class T>
__device__ __forceinline__ T load_as(const uint8_t* p) {
  T v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, alignof(T)), sizeof(T));
  return v;
}

template <class T>
__device__ __forceinline__ void store_as(uint8_t* p, const T& v) {
  __builtin_memcpy(__builtin_assume_aligned(p, alignof(T)), &v, sizeof(T));
}

struct alignas(4) Rgb4 {  // four packed RGB pixels
  uint32_t a, b, c;
};

// --- decoder surfaces (include/advhip.h): 4:2:0 frames described by byte geometry and sample depth.  A sample
// is a byte (BITS 8) or a little-endian 16-bit word whose value is (word >> shift) & 1023 (BITS 10); every offset, pitch and
// step is in bytes from the frame's first byte.  NV12 / NV21 / I420 / YV12 / P010 / yuv420p10le are nothing but these numbers.
struct YuvSurface {
  long long y_off, y_pitch, cb_off, cr_off, c_pitch;
  int c_step, shift;
};

struct alignas(8) Word2 {
  uint32_t lo, hi;
};

template <int BITS>
__device__ __forceinline__ int yuv_sample(const uint8_t* p, int shift) {
  if constexpr (BITS == 8) return *p;
  else return (load_as<uint16_t>(p) >> shift) & 1023;
}

// two / four adjacent samples from one load of their bytes (p aligned to the load's size)
template <int BITS>
__device__ __forceinline__ void yuv_sample2(const uint8_t* p, int shift, int& a, int& b) {
  if constexpr (BITS == 8) {
    const uint32_t w = load_as<uint16_t>(p);
    a = w & 255, b = w >> 8;
  } else {
    const uint32_t w = load_as<uint32_t>(p);
    a = (w >> shift) & 1023, b = (w >> (16 + shift)) & 1023;
  }
}

template <int BITS>
__device__ __forceinline__ void yuv_sample4(const uint8_t* p, int shift, int (&v)[4]) {
  if constexpr (BITS == 8) {
    const uint32_t w = load_as<uint32_t>(p);
    v[0] = w & 255, v[1] = (w >> 8) & 255, v[2] = (w >> 16) & 255, v[3] = w >> 24;
  } else {
    const Word2 w = load_as<Word2>(p);
    v[0] = (w.lo >> shift) & 1023, v[1] = (w.lo >> (16 + shift)) & 1023;
    v[2] = (w.hi >> shift) & 1023, v[3] = (w.hi >> (16 + shift)) & 1023;
  }
}

// --- where a kernel reads its 4:2:0 samples: one of two sources, built in the kernel from its arguments (Arg, and the frame's size)
// and used by value.  Both answer the same questions -- the rows of source row y, one luma sample, one chroma pair, and the four
// luma samples and two chroma pairs of four adjacent pixels from whole loads -- so each kernel below is written once; the compact
// frames keep their own instantiation with its compile-time addressing.  `Size` is what the horizontal pass
// carries of the frame's size: each source names what it reads, so each instantiation keeps the argument block it had.
struct YuvRow {
  const uint8_t *y, *cb, *cr;
};

// the compact 8-bit frame (3H/2, W): int pitches from H, W and the layout, byte loads, no shift.  Cb of sample (c, xc) is at
// chroma[c * cw + xc * cs], Cr cr_off bytes behind it.
struct CompactSource {
  using Arg = int;  // the layout
  static constexpr int BITS = 8;
  struct Size {
    int H, W;  // (the chroma rows start behind H * W bytes of luma)
  };
  int layout, H, W, cw, cs;
  long long cr_off;
  __device__ CompactSource(int layout, Size s) : CompactSource(layout, s.H, s.W) {}
  __device__ CompactSource(int layout, int H, int W)
      : layout(layout), H(H), W(W), cw(layout == 0 ? W : W / 2), cs(layout == 0 ? 2 : 1), cr_off(layout == 0 ? 1 : (long long)(H / 2) * (W / 2)) {}
  __device__ __forceinline__ YuvRow row(const uint8_t* frame, int y) const {
    const uint8_t* yrow = frame + (long long)y * W;
    const uint8_t* cb = frame + (long long)H * W + (long long)(y >> 1) * cw;
    return {yrow, cb, cb + cr_off};
  }
  __device__ __forceinline__ int luma(const YuvRow& r, int x) const { return r.y[x]; }
  __device__ __forceinline__ void chroma_pair(const YuvRow& r, int xc, int& cb, int& cr) const { cb = r.cb[xc * cs], cr = r.cr[xc * cs]; }
  // pixels 4 q .. 4 q + 3: yy from one 4-byte load, c = Cb0, Cr0, Cb1, Cr1 from one 4-byte (NV12) or two 2-byte (I420) loads
  __device__ __forceinline__ void quad(const YuvRow& r, int q, int (&yy)[4], int (&c)[4]) const {
    const uint32_t yw = load_as<uint32_t>(r.y + 4 * q);
    uint32_t cc;  // Cb0 | Cr0 << 8 | Cb1 << 16 | Cr1 << 24
    if (layout == 0) {
      cc = load_as<uint32_t>(r.cb + 4 * q);
    } else {
      const uint32_t u = load_as<uint16_t>(r.cb + 2 * q), v = load_as<uint16_t>(r.cr + 2 * q);
      cc = (u & 255) | (v & 255) << 8 | (u >> 8) << 16 | (v >> 8) << 24;
    }
    yy[0] = yw & 255, yy[1] = (yw >> 8) & 255, yy[2] = (yw >> 16) & 255, yy[3] = yw >> 24;
    c[0] = cc & 255, c[1] = (cc >> 8) & 255, c[2] = (cc >> 16) & 255, c[3] = cc >> 24;
  }
};

// a decoder surface: 64-bit byte geometry by value, samples of BITS bits
template <int BITS_>
struct SurfaceSource {
  using Arg = YuvSurface;
  static constexpr int BITS = BITS_, SB = BITS == 8 ? 1 : 2;  // SB: bytes per sample
  struct Size {
    int W;
  };
  YuvSurface S;
  __device__ SurfaceSource(const YuvSurface& S, Size) : S(S) {}
  __device__ SurfaceSource(const YuvSurface& S, int, int) : S(S) {}
  __device__ __forceinline__ YuvRow row(const uint8_t* frame, int y) const {
    return {frame + S.y_off + y * S.y_pitch, frame + S.cb_off + (y >> 1) * S.c_pitch, frame + S.cr_off + (y >> 1) * S.c_pitch};
  }
  // (the column widened by the caller: the byte offset is formed in 64 bits, as every other offset of a surface)
  __device__ __forceinline__ int luma(const YuvRow& r, long long x) const { return yuv_sample<BITS>(r.y + x * SB, S.shift); }
  __device__ __forceinline__ void chroma_pair(const YuvRow& r, int xc, int& cb, int& cr) const {
    cb = yuv_sample<BITS>(r.cb + (long long)xc * S.c_step, S.shift), cr = yuv_sample<BITS>(r.cr + (long long)xc * S.c_step, S.shift);
  }
  // pixels 4 q .. 4 q + 3: yy from one load of four samples, c = Cb0, Cr0, Cb1, Cr1 from one load of two pairs (interleaved chroma,
  // in either order) or two loads of two samples (planar)
  __device__ __forceinline__ void quad(const YuvRow& r, int q, int (&yy)[4], int (&c)[4]) const {
    yuv_sample4<BITS>(r.y + 4 * SB * q, S.shift, yy);
    if (S.c_step == 2 * SB) {  // interleaved pairs: the two offsets are one sample apart
      yuv_sample4<BITS>((S.cb_off < S.cr_off ? r.cb : r.cr) + 4 * SB * q, S.shift, c);
      if (S.cr_off < S.cb_off) {
        const int c0 = c[0], c2 = c[2];
        c[0] = c[1], c[1] = c0, c[2] = c[3], c[3] = c2;
      }
    } else {
      yuv_sample2<BITS>(r.cb + 2 * SB * q, S.shift, c[0], c[2]);
      yuv_sample2<BITS>(r.cr + 2 * SB * q, S.shift, c[1], c[3]);
    }
  }
};

// two packed pixels (R | G << 8 | B << 16 each) -> their six bytes at o, as three 2-byte pieces (`even`: o is 2-byte aligned) or bytes
__device__ __forceinline__ void store_rgb_pair(uint8_t* o, uint32_t p0, uint32_t p1, int even) {
  if (even) {
    store_as(o, (uint16_t)p0);
    store_as(o + 2, (uint16_t)(p0 >> 16 | p1 << 8));
    store_as(o + 4, (uint16_t)(p1 >> 8));
  } else {
    o[0] = (uint8_t)p0, o[1] = (uint8_t)(p0 >> 8), o[2] = (uint8_t)(p0 >> 16);
    o[3] = (uint8_t)p1, o[4] = (uint8_t)(p1 >> 8), o[5] = (uint8_t)(p1 >> 16);
  }
}

// The conversion alone: dst row r = (f, y) <- source frame f (at byte f * fpitch); one wave per output row.  QUAD is chosen on the
// host (launch_to_rgb) from the alignment of everything that enters an address: a lane converts four adjacent pixels = two chroma
// samples from one load of four Y samples and the source's load of two (Cb, Cr) pairs, and stores their 12 bytes at once.  Otherwise
// a lane converts the pair that shares one chroma sample and stores six bytes (store_rgb_pair; rows and pairs are 2-byte aligned
// where dst is, as W is even).
template <class Src, bool QUAD>
__global__ __launch_bounds__(256) void yuv420_to_rgb_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int H,
                                                              int W, typename Src::Arg arg, YuvCoef k, int even, long long nrows) {
  using Terms = ChromaTerms<Src::BITS>;
  const int lane = threadIdx.x & 63;
  const Src S(arg, H, W);
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / H;
    const int y = (int)(r - f * H);
    const YuvRow in = S.row(src + f * fpitch, y);
    uint8_t* out = dst + r * W * 3;
    if constexpr (QUAD) {
      for (int q = lane; q < W / 4; q += 64) {
        int yy[4], c[4];
        S.quad(in, q, yy, c);
        const Terms c0(c[0], c[1], k), c1(c[2], c[3], k);
        const uint32_t p0 = yuv_rgb_packed(yy[0], c0, k), p1 = yuv_rgb_packed(yy[1], c0, k);
        const uint32_t p2 = yuv_rgb_packed(yy[2], c1, k), p3 = yuv_rgb_packed(yy[3], c1, k);
        store_as(out + 12 * q, Rgb4{p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8});
      }
    } else {
      for (int p = lane; p < W / 2; p += 64) {
        int cb, cr;
        S.chroma_pair(in, p, cb, cr);
        const Terms c(cb, cr, k);
        store_rgb_pair(out + 6 * p, yuv_rgb_packed(S.luma(in, 2 * p), c, k), yuv_rgb_packed(S.luma(in, 2 * p + 1), c, k), even);
      }
    }
  }
}

// resize_h_u8_kernel on 4:2:0 frames: every tap's pixel is converted to its three bytes first and accumulated as there, so the
// output is byte for byte that kernel's on the converted frame.  The taps [x0, x0 + n) are walked chroma sample by chroma sample:
// one chroma read and one set of products for the (up to) two taps that share it.
template <class Src>
__device__ __forceinline__ void resize_h_yuv420_row(const Src& S, const YuvRow& in, uint8_t* __restrict__ out, int W, int OW,
                                                    const int* __restrict__ xb, const int* __restrict__ xk, int ksize, const YuvCoef& k, int lane) {
  for (int x = lane; x < OW; x += 64) {
    int x0 = xb[2 * x];
    int n = min(xb[2 * x + 1], ksize);
    if (x0 < 0 || x0 + n > W) x0 = 0, n = 0;  // (never for tables from resize.py: a guard against a foreign table)
    const int xe = x0 + n;
    const int* w = xk + (long long)x * ksize - x0;  // indexed by the source column
    int s0 = 1 << (RESIZE_BITS - 1), s1 = s0, s2 = s0;
    for (int xc = x0 >> 1; 2 * xc < xe; ++xc) {
      int cb, cr;
      S.chroma_pair(in, xc, cb, cr);
      const ChromaTerms<Src::BITS> c(cb, cr, k);
#pragma unroll
      for (int xs = 2 * xc; xs < 2 * xc + 2; ++xs) {
        if (xs >= x0 && xs < xe) {
          int pr, pg, pb;
          yuv_rgb(S.luma(in, xs), c, k, pr, pg, pb);
          const int wk = w[xs];
          s0 += pr * wk;
          s1 += pg * wk;
          s2 += pb * wk;
        }
      }
    }
    out[3 * x] = clip8(s0);
    out[3 * x + 1] = clip8(s1);
    out[3 * x + 2] = clip8(s2);
  }
}

template <class Src>
__global__ __launch_bounds__(256) void resize_h_yuv420_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch,
                                                                typename Src::Size size, int OW, int row0, int rows, const int* __restrict__ xb,
                                                                const int* __restrict__ xk, int ksize, typename Src::Arg arg, YuvCoef k,
                                                                long long nrows) {
  const int lane = threadIdx.x & 63, W = size.W;
  const Src S(arg, size);
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / rows;
    const int y = row0 + (int)(r - f * rows);
    const YuvRow in = S.row(src + f * fpitch, y);
    uint8_t* out = dst + r * OW * 3;
    resize_h_yuv420_row(S, in, out, W, OW, xb, xk, ksize, k, lane);
  }
}

// resize_h_roi_u8_kernel on 4:2:0 frames, source frame s at byte s * fpitch: the row body above with the lookup of that kernel.
template <class Src>
__global__ __launch_bounds__(256) void resize_h_roi_yuv420_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ ws, RoiArgs A,
                                                                    long long fpitch, typename Src::Size size, int OW, const int* __restrict__ xb,
                                                                    const int* __restrict__ xk, int ksize, typename Src::Arg arg, YuvCoef k) {
  const int lane = threadIdx.x & 63, W = size.W;
  const Src S(arg, size);
  const long long nrows = A.N * A.ws_rows;
  for (long long r = wave_row(); r < nrows; r += (long long)gridDim.x * 4) {
    const long long i = r / A.ws_rows;
    const int y = (int)(r - i * A.ws_rows);
    const RoiFrame f = roi_frame(A, i);
    if (!f.ok || y >= f.rows) continue;
    const YuvRow in = S.row(src + f.src * fpitch, f.row0 + y);
    resize_h_yuv420_row(S, in, ws + r * OW * 3, W, OW, xb + (long long)f.table * OW * 2, xk + (long long)f.table * OW * ksize, ksize, k, lane);
  }
}

}  // namespace advhip

using namespace advhip;

static bool mul_ok(long long a, long long b, long long c, long long d, long long* out) {
  long long t;
  return !__builtin_mul_overflow(a, b, &t) && !__builtin_mul_overflow(t, c, &t) && !__builtin_mul_overflow(t, d, out);
}

// every kernel here: a wave per row, four rows per block
static int row_grid(long long nrows) { return (int)std::min<long long>((nrows + 3) / 4, 256 * 256); }

// source frames 0, frame_step, 2 frame_step, ... -> a compact output (F_src < 1 passes through: the caller refuses it)
static int64_t sampled_frames(int64_t F_src, int32_t frame_step) { return F_src < 1 ? F_src : (F_src - 1) / frame_step + 1; }

// bytes from one sampled 4:2:0 source frame to the next -> *pitch, false where the product overflows (never with F > 1 frames whose
// bytes were counted: it lies inside them).  A single frame has no next one: its pitch is 0.
static bool source_pitch(long long frame_bytes, int32_t frame_step, int64_t F, long long* pitch) {
  const bool ok = mul_ok(frame_bytes, frame_step, 1, 1, pitch);
  if (F == 1) *pitch = 0;
  return ok;
}

// the eleven resize arguments of the resize entry points
struct ResizeArgs {
  int32_t C, OH, OW;
  const int32_t *xbounds, *xcoef;
  int32_t xksize;
  const int32_t *ybounds, *ycoef;
  int32_t yksize, row0, rows;
};

// Which passes the resize of F frames H x W -> OH x OW runs, with what they need checked: tables and a ksize per pass, the
// horizontal pass's rows inside the frame (all of them where no vertical pass follows) and the workspace between the passes.
// `converted` (4:2:0 frames): a vertical pass alone reads the converted F x H x W x C frames from the workspace, not the source.
struct PassPlan {
  bool horiz, vert;
  long long ws_bytes;  // of the horizontal pass's rows
};

static int plan_passes(const char* who, int64_t F, int32_t H, int32_t W, const ResizeArgs& R, const uint8_t* ws, bool converted,
                       PassPlan* P) {
  *P = {R.OW != W, R.OH != H, 0};
  ADVHIP_REQUIRE((long long)W * R.C <= INT32_MAX && (long long)R.OW * R.C <= INT32_MAX, "%s: rows of %d / %d pixels are too long", who, W, R.OW);
  if (P->horiz) {
    ADVHIP_REQUIRE(R.xbounds && R.xcoef, "%s: null horizontal tables", who);
    ADVHIP_REQUIRE(R.xksize >= 1, "%s: horizontal ksize %d < 1", who, R.xksize);
    ADVHIP_REQUIRE(R.row0 >= 0 && R.rows >= 1 && (long long)R.row0 + R.rows <= H, "%s: rows [%d, %lld) of the horizontal pass outside the %d-row frames",
                   who, R.row0, (long long)R.row0 + R.rows, H);
    ADVHIP_REQUIRE(P->vert || (R.row0 == 0 && R.rows == H), "%s: without a vertical pass the horizontal pass must compute all %d rows", who, H);
    ADVHIP_REQUIRE(mul_ok(F, R.rows, R.OW, R.C, &P->ws_bytes), "%s: workspace size overflows int64", who);
    ADVHIP_REQUIRE(ws || !P->vert, "%s: null workspace for the horizontal pass (%lld bytes)", who, P->ws_bytes);
  } else if (P->vert && converted) {  // (the caller counted these bytes: no overflow)
    ADVHIP_REQUIRE(ws, "%s: null workspace for the converted frames of a vertical-only resize (%lld bytes)", who, (long long)F * H * W * R.C);
  }
  if (P->vert) {
    ADVHIP_REQUIRE(R.ybounds && R.ycoef, "%s: null vertical tables", who);
    ADVHIP_REQUIRE(R.yksize >= 1, "%s: vertical ksize %d < 1", who, R.yksize);
  }
  return ADVHIP_OK;
}

// the vertical pass of a plan: from the horizontal pass's rows in the workspace, or (no horizontal pass) from whole H-row RGB
// frames at `frames`, `pitch` bytes apart
static int launch_vertical(const char* what, const PassPlan& P, const ResizeArgs& R, const uint8_t* frames, long long pitch, const uint8_t* ws,
                           uint8_t* dst, int64_t F, int32_t H, hipStream_t s) {
  const long long nrows = F * R.OH;
  hipLaunchKernelGGL(resize_v_u8_kernel, dim3(row_grid(nrows)), dim3(256), 0, s, P.horiz ? ws : frames, dst,
                     P.horiz ? (long long)R.rows * R.OW * R.C : pitch, P.horiz ? R.rows : H, R.OH, R.OW * R.C, P.horiz ? R.row0 : 0, R.ybounds, R.ycoef,
                     R.yksize, nrows);
  return check_launch(what);
}

extern "C" int advhip_resize_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F, int32_t H, int32_t W, int32_t C, int32_t OH,
                                int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds,
                                const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, void* stream) {
  return advhip_resize_u8_sampled(src, dst, ws, F, 1, H, W, C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, row0, rows, stream);
}

extern "C" int advhip_resize_u8_sampled(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int32_t H, int32_t W,
                                        int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                                        const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows,
                                        void* stream) {
  const ResizeArgs R{C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, row0, rows};
  ADVHIP_REQUIRE(src && dst, "resize_u8: null frames or output");
  ADVHIP_REQUIRE(frame_step >= 1, "resize_u8: frame step %d", frame_step);
  const int64_t F = sampled_frames(F_src, frame_step);
  ADVHIP_REQUIRE(F >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "resize_u8: sizes must be >= 1 (F=%lld, %d x %d -> %d x %d)",
                 (long long)F, H, W, OH, OW);
  ADVHIP_REQUIRE(C == 3, "resize_u8: frames must have 3 channels (RGB), got C=%d", C);
  long long in_bytes, out_bytes;
  ADVHIP_REQUIRE(mul_ok(F_src, H, W, C, &in_bytes) && mul_ok(F, OH, OW, C, &out_bytes), "resize_u8: frame sizes overflow int64");
  // (F > 1: the product is inside in_bytes; a single frame keeps a pitch that the strided copy below accepts)
  const long long frame_bytes = (long long)H * W * C, src_pitch = F > 1 ? frame_bytes * frame_step : frame_bytes;
  PassPlan P;
  if (const int rc = plan_passes("resize_u8", F, H, W, R, ws, false, &P); rc != ADVHIP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (!P.horiz && !P.vert) {  // Pillow returns a copy
    hipError_t e = hipSuccess;
    if (frame_step > 1) e = hipMemcpy2DAsync(dst, (size_t)frame_bytes, src, (size_t)src_pitch, (size_t)frame_bytes, (size_t)F, hipMemcpyDeviceToDevice, s);
    else if (src != dst) e = hipMemcpyAsync(dst, src, (size_t)in_bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      set_error("resize_u8 copy: %s", hipGetErrorString(e));
      return ADVHIP_ELAUNCH;
    }
    return ADVHIP_OK;
  }
  if (P.horiz) {
    const long long nrows = F * rows;
    hipLaunchKernelGGL(resize_h_u8_kernel, dim3(row_grid(nrows)), dim3(256), 0, s, src, P.vert ? ws : dst, src_pitch, W, OW, row0, rows, xbounds, xcoef,
                       xksize, nrows);
    const int rc = check_launch("resize_u8 horizontal pass");
    if (rc != ADVHIP_OK) return rc;
  }
  return P.vert ? launch_vertical("resize_u8 vertical pass", P, R, src, src_pitch, ws, dst, F, H, s) : ADVHIP_OK;
}

// where the 4:2:0 samples of a frame are: a surface by its numbers, with the frame pitch the caller gave
struct Yuv420Source {
  int bits;               // 8 | 10
  long long frame_pitch;  // bytes from one source frame to the next
  YuvSurface S;
};

// the compact 8-bit frame (3H/2, W) of the first two entry points as a surface (for the checks; its launches stay its own kernels)
static Yuv420Source compact_source(int H, int W, int layout) {
  const long long y = (long long)H * W, c = (long long)(H / 2) * (W / 2);
  const bool nv12 = layout == ADVHIP_YUV420_NV12;
  return {8, y + 2 * c, {0, W, y, nv12 ? y + 1 : y + c, nv12 ? W : W / 2, nv12 ? 2 : 1, 0}};
}

// coefficients that keep every int32 sum exact at that depth (Y < 2^bits, |chroma - mid| <= 2^(bits - 1), bits <= 10: below 2^30)
static int check_yuv_coef(const char* who, const YuvCoef& k, int bits) {
  ADVHIP_REQUIRE(k.yoff == 0 || k.yoff == 16 << (bits - 8), "%s: luma offset %d is neither 0 (full range) nor %d (limited range)", who, k.yoff,
                 16 << (bits - 8));
  const int lim = 1 << 18;
  ADVHIP_REQUIRE(k.cy > 0 && k.cy < lim, "%s: luma coefficient %d outside (0, 2^18)", who, k.cy);
  ADVHIP_REQUIRE(k.crv >= 0 && k.crv < lim && k.cgu >= 0 && k.cgu < lim && k.cgv >= 0 && k.cgv < lim && k.cbu >= 0 && k.cbu < lim,
                 "%s: chroma coefficients (%d, %d, %d, %d) outside [0, 2^18)", who, k.crv, k.cgu, k.cgv, k.cbu);
  return ADVHIP_OK;
}

// the checks both compact 4:2:0 entry points share: even geometry, a known layout, the coefficients
static int check_yuv420(const char* who, int32_t H, int32_t W, int32_t layout, const YuvCoef& k) {
  ADVHIP_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 frames need even H and W >= 2, got %d x %d", who, H, W);
  ADVHIP_REQUIRE(layout == ADVHIP_YUV420_NV12 || layout == ADVHIP_YUV420_I420, "%s: layout %d is neither NV12 (0) nor I420 (1)", who, layout);
  return check_yuv_coef(who, k, 8);
}

// the checks both surface entry points share: the rules of include/advhip.h, every plane inside the frame, the coefficients
static int check_surface(const char* who, const uint8_t* src, int32_t H, int32_t W, const Yuv420Source& Y, const YuvCoef& k) {
  const YuvSurface& S = Y.S;
  ADVHIP_REQUIRE(Y.bits == 8 || Y.bits == 10, "%s: %d-bit samples (8 or 10)", who, Y.bits);
  const int sb = Y.bits == 8 ? 1 : 2;
  ADVHIP_REQUIRE(S.shift >= 0 && S.shift <= 6 && (Y.bits == 10 || S.shift == 0), "%s: shift %d outside [0, 6], or not 0 at 8 bits", who, S.shift);
  ADVHIP_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 frames need even H and W >= 2, got %d x %d", who, H, W);
  ADVHIP_REQUIRE(Y.frame_pitch >= 1 && S.y_off >= 0 && S.cb_off >= 0 && S.cr_off >= 0, "%s: frame pitch %lld < 1 or a negative plane offset (%lld, %lld, %lld)",
                 who, Y.frame_pitch, S.y_off, S.cb_off, S.cr_off);
  ADVHIP_REQUIRE(S.c_step == sb || S.c_step == 2 * sb, "%s: chroma step %d is neither %d (planar) nor %d (interleaved)", who, S.c_step, sb, 2 * sb);
  ADVHIP_REQUIRE(S.c_step == sb || S.cb_off - S.cr_off == sb || S.cr_off - S.cb_off == sb,
                 "%s: interleaved chroma needs Cb and Cr one sample (%d bytes) apart, got offsets %lld and %lld", who, sb, S.cb_off, S.cr_off);
  ADVHIP_REQUIRE(S.y_pitch >= (long long)W * sb, "%s: luma pitch %lld below a row of %d samples (%lld bytes)", who, S.y_pitch, W, (long long)W * sb);
  ADVHIP_REQUIRE(S.c_pitch >= (long long)(W / 2) * S.c_step, "%s: chroma pitch %lld below a chroma row (%lld bytes)", who, S.c_pitch,
                 (long long)(W / 2) * S.c_step);
  if (Y.bits == 10)
    ADVHIP_REQUIRE(((uintptr_t)src | Y.frame_pitch | S.y_off | S.y_pitch | S.cb_off | S.cr_off | S.c_pitch) % 2 == 0,
                   "%s: 16-bit samples need an even address, frame pitch, offsets and pitches", who);
  const __int128 y_end = (__int128)S.y_off + (__int128)(H - 1) * S.y_pitch + (long long)W * sb;
  const __int128 c_last = (__int128)(H / 2 - 1) * S.c_pitch + (long long)(W / 2 - 1) * S.c_step + sb;
  ADVHIP_REQUIRE(y_end <= Y.frame_pitch && S.cb_off + c_last <= Y.frame_pitch && S.cr_off + c_last <= Y.frame_pitch,
                 "%s: a plane ends past the frame's %lld bytes (luma at %lld, Cb at %lld, Cr at %lld)", who, Y.frame_pitch, (long long)y_end,
                 (long long)(S.cb_off + c_last), (long long)(S.cr_off + c_last));
  return check_yuv_coef(who, k, Y.bits);
}

// one source's conversion kernel, with or without the four-pixel path
template <class Src>
static void launch_to_rgb_from(bool quad, const typename Src::Arg& arg, const uint8_t* src, uint8_t* dst, long long F, long long src_pitch, int H, int W,
                               const YuvCoef& k, hipStream_t s) {
  const long long nrows = F * H;
  if (quad) hipLaunchKernelGGL((yuv420_to_rgb_u8_kernel<Src, true>), dim3(row_grid(nrows)), dim3(256), 0, s, src, dst, src_pitch, H, W, arg, k, 1, nrows);
  else
    hipLaunchKernelGGL((yuv420_to_rgb_u8_kernel<Src, false>), dim3(row_grid(nrows)), dim3(256), 0, s, src, dst, src_pitch, H, W, arg, k,
                       (int)((uintptr_t)dst % 2 == 0), nrows);
}

// (every argument checked by the caller) frames 0, frame_step, ... of src -> compact RGB frames in dst; `compact` frames run their
// own instantiation, a surface the surface ones.  The four-pixel path needs every load and the 12-byte store aligned.  Compact
// frames: W a multiple of 4 and both pointers 4-byte aligned (a frame is 3 H / 2 * W bytes: a multiple of 4 then).  A surface: Y and
// interleaved chroma are read 4 sb bytes at a time, planar chroma 2 sb bytes, so everything that enters those addresses must be a
// multiple of that -- the pointer, the frame pitch (where a second frame is read), the offsets and the pitches.
static int launch_to_rgb(bool compact, int layout, const Yuv420Source& Y, const uint8_t* src, uint8_t* dst, long long F, long long src_pitch, int H,
                         int W, const YuvCoef& k, hipStream_t s) {
  const YuvSurface& S = Y.S;
  const int sb = Y.bits == 8 ? 1 : 2;
  const long long ya = 4 * sb, ca = S.c_step == 2 * sb ? 4 * sb : 2 * sb;
  const bool quad = W % 4 == 0 && (uintptr_t)dst % 4 == 0 &&
                    (compact ? (uintptr_t)src % 4 == 0
                             : ((uintptr_t)src | src_pitch | S.y_off | S.y_pitch) % ya == 0 &&
                                   ((uintptr_t)src | src_pitch | std::min(S.cb_off, S.cr_off) | S.c_pitch) % ca == 0 &&
                                   (S.c_step == 2 * sb || (S.cb_off | S.cr_off) % ca == 0));
  if (compact) launch_to_rgb_from<CompactSource>(quad, layout, src, dst, F, src_pitch, H, W, k, s);
  else if (Y.bits == 8) launch_to_rgb_from<SurfaceSource<8>>(quad, S, src, dst, F, src_pitch, H, W, k, s);
  else launch_to_rgb_from<SurfaceSource<10>>(quad, S, src, dst, F, src_pitch, H, W, k, s);
  return check_launch(compact ? "yuv420_to_rgb_u8" : "yuv420_surface_to_rgb_u8");
}

// both conversion entry points
static int yuv420_to_rgb(const char* who, bool compact, int layout, const Yuv420Source& Y, const uint8_t* src, uint8_t* dst, int64_t F_src,
                         int32_t frame_step, int32_t H, int32_t W, const YuvCoef& k, void* stream) {
  ADVHIP_REQUIRE(src && dst, "%s: null frames or output", who);
  ADVHIP_REQUIRE(frame_step >= 1, "%s: frame step %d", who, frame_step);
  const int64_t F = sampled_frames(F_src, frame_step);
  ADVHIP_REQUIRE(F >= 1, "%s: %lld frames", who, (long long)F_src);
  if (const int rc = compact ? check_yuv420(who, H, W, layout, k) : check_surface(who, src, H, W, Y, k); rc != ADVHIP_OK) return rc;
  long long in_bytes, out_bytes, pitch;
  ADVHIP_REQUIRE(mul_ok(F_src, Y.frame_pitch, 1, 1, &in_bytes) && mul_ok(F, H, W, 3, &out_bytes) && source_pitch(Y.frame_pitch, frame_step, F, &pitch),
                 "%s: frame sizes overflow int64", who);
  ADVHIP_REQUIRE((long long)W * 3 <= INT32_MAX, "%s: rows of %d pixels are too long", who, W);
  return launch_to_rgb(compact, layout, Y, src, dst, F, pitch, H, W, k, (hipStream_t)stream);
}

extern "C" int advhip_yuv420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t F_src, int32_t frame_step, int32_t H, int32_t W, int32_t layout,
                                       int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  return yuv420_to_rgb("yuv420_to_rgb_u8", true, layout, compact_source(H, W, layout), src, dst, F_src, frame_step, H, W,
                       YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}

extern "C" int advhip_yuv420_surface_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t F_src, int32_t frame_step, int64_t frame_pitch, int32_t H,
                                               int32_t W, int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset,
                                               int64_t cr_offset, int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv,
                                               int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  const Yuv420Source Y{bits, frame_pitch, {y_offset, y_pitch, cb_offset, cr_offset, chroma_pitch, chroma_step, shift}};
  return yuv420_to_rgb("yuv420_surface_to_rgb_u8", false, -1, Y, src, dst, F_src, frame_step, H, W, YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}

// both fused-resize entry points
static int resize_yuv420(const char* who, bool compact, int layout, const Yuv420Source& Y, const uint8_t* src, uint8_t* dst, uint8_t* ws,
                         int64_t F_src, int32_t frame_step, int32_t H, int32_t W, const ResizeArgs& R, const YuvCoef& k, void* stream) {
  ADVHIP_REQUIRE(src && dst, "%s: null frames or output", who);
  ADVHIP_REQUIRE(frame_step >= 1, "%s: frame step %d", who, frame_step);
  const int64_t F = sampled_frames(F_src, frame_step);
  ADVHIP_REQUIRE(F >= 1 && R.OH >= 1 && R.OW >= 1, "%s: sizes must be >= 1 (F=%lld, -> %d x %d)", who, (long long)F, R.OH, R.OW);
  ADVHIP_REQUIRE(R.C == 3, "%s: the output has 3 channels (RGB), got C=%d", who, R.C);
  if (const int rc = compact ? check_yuv420(who, H, W, layout, k) : check_surface(who, src, H, W, Y, k); rc != ADVHIP_OK) return rc;
  long long in_bytes, out_bytes, rgb_bytes, src_pitch;
  ADVHIP_REQUIRE(mul_ok(F_src, Y.frame_pitch, 1, 1, &in_bytes) && mul_ok(F, R.OH, R.OW, R.C, &out_bytes) && mul_ok(F, H, W, R.C, &rgb_bytes) &&
                     source_pitch(Y.frame_pitch, frame_step, F, &src_pitch),
                 "%s: frame sizes overflow int64", who);
  PassPlan P;
  if (const int rc = plan_passes(who, F, H, W, R, ws, true, &P); rc != ADVHIP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  uint8_t* to = P.vert ? ws : dst;
  if (P.horiz) {
    const long long nrows = F * R.rows;
    auto launch = [&](auto kernel, const auto& size, const auto& arg) {
      hipLaunchKernelGGL(kernel, dim3(row_grid(nrows)), dim3(256), 0, s, src, to, src_pitch, size, R.OW, R.row0, R.rows, R.xbounds, R.xcoef, R.xksize, arg, k,
                         nrows);
    };
    if (compact) launch(resize_h_yuv420_u8_kernel<CompactSource>, CompactSource::Size{H, W}, layout);
    else if (Y.bits == 8) launch(resize_h_yuv420_u8_kernel<SurfaceSource<8>>, SurfaceSource<8>::Size{W}, Y.S);
    else launch(resize_h_yuv420_u8_kernel<SurfaceSource<10>>, SurfaceSource<10>::Size{W}, Y.S);
    const int rc = check_launch("resize_yuv420_u8 horizontal pass");
    if (rc != ADVHIP_OK) return rc;
  } else {  // rare: the conversion launch, into dst (the identity) or into the workspace the vertical pass then reads
    const int rc = launch_to_rgb(compact, layout, Y, src, to, F, src_pitch, H, W, k, s);
    if (rc != ADVHIP_OK) return rc;
  }
  // the RGB resize's own vertical pass
  return P.vert ? launch_vertical("resize_yuv420_u8 vertical pass", P, R, ws, (long long)H * W * R.C, ws, dst, F, H, s) : ADVHIP_OK;
}

extern "C" int advhip_resize_yuv420_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int32_t H, int32_t W,
                                       int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                                       const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, int32_t layout,
                                       int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  return resize_yuv420("resize_yuv420_u8", true, layout, compact_source(H, W, layout), src, dst, ws, F_src, frame_step, H, W,
                       {C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, row0, rows}, YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}

extern "C" int advhip_resize_yuv420_surface_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int64_t frame_pitch,
                                               int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef,
                                               int32_t xksize, const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0,
                                               int32_t rows, int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset,
                                               int64_t cr_offset, int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv,
                                               int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  const Yuv420Source Y{bits, frame_pitch, {y_offset, y_pitch, cb_offset, cr_offset, chroma_pitch, chroma_step, shift}};
  return resize_yuv420("resize_yuv420_surface_u8", false, -1, Y, src, dst, ws, F_src, frame_step, H, W,
                       {C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, row0, rows}, YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}

// --- regions of interest: the three entry points (include/advhip.h) ---

// the arguments the three roi entry points share beyond their models'
struct RoiCall {
  int64_t F_src, N;
  const int32_t* src_of;
  int32_t frame_step;
  const int32_t* table_of;
  int32_t n_tables;
  const int32_t* rowspan;
  int32_t ws_rows;
};

// every check of a roi call that does not depend on the source form -> the kernels' argument block
static int check_roi(const char* who, const uint8_t* src, const uint8_t* dst, const uint8_t* ws, const RoiCall& Q, int32_t H, int32_t W,
                     const ResizeArgs& R, RoiArgs* A) {
  ADVHIP_REQUIRE(src && dst, "%s: null frames or output", who);
  ADVHIP_REQUIRE(ws, "%s: null workspace (both passes always run)", who);
  ADVHIP_REQUIRE(Q.frame_step >= 1, "%s: frame step %d", who, Q.frame_step);
  ADVHIP_REQUIRE(Q.F_src >= 1 && Q.N >= 1 && H >= 1 && W >= 1 && R.OH >= 1 && R.OW >= 1,
                 "%s: sizes must be >= 1 (F_src=%lld, N=%lld, %d x %d -> %d x %d)", who, (long long)Q.F_src, (long long)Q.N, H, W, R.OH, R.OW);
  ADVHIP_REQUIRE(R.C == 3, "%s: the output has 3 channels (RGB), got C=%d", who, R.C);
  ADVHIP_REQUIRE(Q.n_tables >= 1, "%s: %d tables", who, Q.n_tables);
  ADVHIP_REQUIRE(R.xbounds && R.xcoef, "%s: null horizontal tables", who);
  ADVHIP_REQUIRE(R.ybounds && R.ycoef, "%s: null vertical tables", who);
  ADVHIP_REQUIRE(R.xksize >= 1, "%s: horizontal ksize %d < 1", who, R.xksize);
  ADVHIP_REQUIRE(R.yksize >= 1, "%s: vertical ksize %d < 1", who, R.yksize);
  ADVHIP_REQUIRE(Q.rowspan, "%s: null rowspan", who);
  ADVHIP_REQUIRE(Q.ws_rows >= 1 && Q.ws_rows <= H, "%s: ws_rows %d outside [1, %d]", who, Q.ws_rows, H);
  ADVHIP_REQUIRE((long long)W * 3 <= INT32_MAX && (long long)R.OW * 3 <= INT32_MAX, "%s: rows of %d / %d pixels are too long", who, W, R.OW);
  long long last, out_bytes, ws_bytes, xk_ints, yk_ints;
  ADVHIP_REQUIRE(mul_ok(Q.N, R.OH, R.OW, R.C, &out_bytes) && mul_ok(Q.N, Q.ws_rows, R.OW, R.C, &ws_bytes) &&
                     mul_ok(Q.n_tables, R.OW, R.xksize, 1, &xk_ints) && mul_ok(Q.n_tables, R.OH, R.yksize, 1, &yk_ints),
                 "%s: frame or table sizes overflow int64", who);
  ADVHIP_REQUIRE(Q.src_of || (mul_ok(Q.N - 1, Q.frame_step, 1, 1, &last) && last < Q.F_src),
                 "%s: output frame %lld at frame step %d is past the %lld source frames", who, (long long)Q.N - 1, Q.frame_step, (long long)Q.F_src);
  *A = {Q.src_of, Q.table_of, Q.rowspan, Q.F_src, Q.N, Q.frame_step, Q.n_tables, H, Q.ws_rows};
  return ADVHIP_OK;
}

// the vertical pass of a roi call, from the workspace
static int launch_roi_vertical(const char* what, const RoiArgs& A, const ResizeArgs& R, const uint8_t* ws, uint8_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(resize_v_roi_u8_kernel, dim3(row_grid(A.N * R.OH)), dim3(256), 0, s, ws, dst, A, R.OH, R.OW * R.C, R.ybounds, R.ycoef, R.yksize);
  return check_launch(what);
}

extern "C" int advhip_resize_roi_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of, int32_t frame_step,
                                    const int32_t* table_of, int32_t n_tables, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW,
                                    const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds, const int32_t* ycoef,
                                    int32_t yksize, const int32_t* rowspan, int32_t ws_rows, void* stream) {
  const char* who = "resize_roi_u8";
  const ResizeArgs R{C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, 0, ws_rows};
  RoiArgs A;
  if (const int rc = check_roi(who, src, dst, ws, {F_src, N, src_of, frame_step, table_of, n_tables, rowspan, ws_rows}, H, W, R, &A); rc != ADVHIP_OK)
    return rc;
  long long in_bytes;
  ADVHIP_REQUIRE(mul_ok(F_src, H, W, C, &in_bytes), "%s: frame sizes overflow int64", who);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(resize_h_roi_u8_kernel, dim3(row_grid(N * ws_rows)), dim3(256), 0, s, src, ws, A, W, OW, xbounds, xcoef, xksize);
  if (const int rc = check_launch("resize_roi_u8 horizontal pass"); rc != ADVHIP_OK) return rc;
  return launch_roi_vertical("resize_roi_u8 vertical pass", A, R, ws, dst, s);
}

// both 4:2:0 roi entry points
static int resize_roi_yuv420(const char* who, bool compact, int layout, const Yuv420Source& Y, const uint8_t* src, uint8_t* dst, uint8_t* ws,
                             const RoiCall& Q, int32_t H, int32_t W, const ResizeArgs& R, const YuvCoef& k, void* stream) {
  RoiArgs A;
  if (const int rc = check_roi(who, src, dst, ws, Q, H, W, R, &A); rc != ADVHIP_OK) return rc;
  if (const int rc = compact ? check_yuv420(who, H, W, layout, k) : check_surface(who, src, H, W, Y, k); rc != ADVHIP_OK) return rc;
  long long in_bytes;
  ADVHIP_REQUIRE(mul_ok(Q.F_src, Y.frame_pitch, 1, 1, &in_bytes), "%s: frame sizes overflow int64", who);
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto kernel, const auto& size, const auto& arg) {
    hipLaunchKernelGGL(kernel, dim3(row_grid(Q.N * Q.ws_rows)), dim3(256), 0, s, src, ws, A, Y.frame_pitch, size, R.OW, R.xbounds, R.xcoef, R.xksize, arg, k);
  };
  if (compact) launch(resize_h_roi_yuv420_u8_kernel<CompactSource>, CompactSource::Size{H, W}, layout);
  else if (Y.bits == 8) launch(resize_h_roi_yuv420_u8_kernel<SurfaceSource<8>>, SurfaceSource<8>::Size{W}, Y.S);
  else launch(resize_h_roi_yuv420_u8_kernel<SurfaceSource<10>>, SurfaceSource<10>::Size{W}, Y.S);
  if (const int rc = check_launch("resize_roi_yuv420_u8 horizontal pass"); rc != ADVHIP_OK) return rc;
  return launch_roi_vertical("resize_roi_yuv420_u8 vertical pass", A, R, ws, dst, s);
}

extern "C" int advhip_resize_roi_yuv420_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of,
                                           int32_t frame_step, const int32_t* table_of, int32_t n_tables, int32_t H, int32_t W, int32_t C,
                                           int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                                           const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, const int32_t* rowspan, int32_t ws_rows,
                                           int32_t layout, int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu,
                                           void* stream) {
  return resize_roi_yuv420("resize_roi_yuv420_u8", true, layout, compact_source(H, W, layout), src, dst, ws,
                           {F_src, N, src_of, frame_step, table_of, n_tables, rowspan, ws_rows}, H, W,
                           {C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, 0, ws_rows}, YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}

extern "C" int advhip_resize_roi_surface_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of,
                                            int32_t frame_step, const int32_t* table_of, int32_t n_tables, int64_t frame_pitch, int32_t H,
                                            int32_t W, int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef,
                                            int32_t xksize, const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, const int32_t* rowspan,
                                            int32_t ws_rows, int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset,
                                            int64_t cr_offset, int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv,
                                            int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  const Yuv420Source Y{bits, frame_pitch, {y_offset, y_pitch, cb_offset, cr_offset, chroma_pitch, chroma_step, shift}};
  return resize_roi_yuv420("resize_roi_surface_u8", false, -1, Y, src, dst, ws, {F_src, N, src_of, frame_step, table_of, n_tables, rowspan, ws_rows}, H,
                           W, {C, OH, OW, xbounds, xcoef, xksize, ybounds, ycoef, yksize, 0, ws_rows}, YuvCoef{yoff, cy, crv, cgu, cgv, cbu}, stream);
}
