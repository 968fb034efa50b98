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

// Horizontal pass: dst row r = (f, y) of `rows` rows per frame <- src row (f, row0 + y); one wave per output row, a lane per
// output pixel (three channels).  Bounds and coefficients of a pixel are read once for its three channels.  Output frame f reads
// the source frame at byte f * fpitch: H * W * 3 for every frame, frame_step times that for every frame_step-th one.
__global__ __launch_bounds__(256) void resize_h_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int W,
                                                         int OW, int row0, int rows, const int* __restrict__ xb,
                                                         const int* __restrict__ xk, int ksize, long long nrows) {
  const int lane = threadIdx.x & 63;
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / rows;
    const int y = (int)(r - f * rows);
    const uint8_t* in = src + f * fpitch + (row0 + y) * (long long)W * 3;
    uint8_t* out = dst + r * OW * 3;
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
}

// Vertical pass: dst row (f, oy) <- rows [yb[oy].first - ybase, + count) of the IH-row source frame f; one wave per output row,
// a lane per output byte (the row's coefficients are the same for every lane).  Source frame f starts at byte f * fpitch.
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
    for (int q = lane; q < rowbytes; q += 64) {
      int s = 1 << (RESIZE_BITS - 1);
      for (int j = 0; j < n; ++j) s += (int)in[(long long)j * rowbytes + q] * k[j];
      out[q] = clip8(s);
    }
  }
}

// --- Y'CbCr 4:2:0 frames (NV12 / I420), uint8 (F, 3H/2, W): rows [0, H) are Y; NV12 then holds H/2 rows of interleaved (Cb, Cr)
// pairs, I420 the (H/2, W/2) Cb plane followed by the Cr plane.  Pixel (y, x) uses chroma sample (y >> 1, x >> 1) (nearest).  The
// conversion is the integer formula of include/advhip.h with the caller's 2^16 fixed-point coefficients, all in int32.
struct YuvCoef {
  int yoff, cy, crv, cgu, cgv, cbu;
};

// how a frame's chroma is addressed: Cb of sample (c, xc) at chroma[c * cw + xc * cs], Cr cr_off bytes behind it
struct YuvLayout {
  int cw, cs;
  long long cr_off;
  __device__ YuvLayout(int layout, int H, int W)
      : cw(layout == 0 ? W : W / 2), cs(layout == 0 ? 2 : 1), cr_off(layout == 0 ? 1 : (long long)(H / 2) * (W / 2)) {}
};

// the three chroma terms of a sample, formed once for the pixels that share it
struct ChromaTerms {
  int rv, guv, bu;
  __device__ __forceinline__ ChromaTerms(int cb, int cr, const YuvCoef& k)
      : rv(k.crv * (cr - 128)), guv(-k.cgu * (cb - 128) - k.cgv * (cr - 128)), bu(k.cbu * (cb - 128)) {}
};

// clip8(v >> 16) with the arithmetic shift of the definition: below 0 -> 0, from 2^24 on -> 255.  The clamp comes BEFORE the shift
// on purpose.  Written as clamp(v >> 16, 0, 255), two of these OR-ed into one word became gfx950's v_ashr_pk_u8_i32 with ROCm 7.2.0
// (AMD clang 22.0.0git, roc-7.2.0), into a register that still held a 32-bit sum; on the MI355X the bytes OR-ed in above its 16-bit
// result then came out as that sum's high half, so the instruction kept it where the compiler counted on zero.  Observed with that
// compiler only, and another one may fuse this form as well: tests/test_hip_yuv420.py's
// test_conversion_is_the_restatement_for_every_triple (every triple, clamped ones included, through the packing kernel) is the guard.
__device__ __forceinline__ int sat8_shr16(int v) { return min(max(v, 0), 0xFFFFFF) >> 16; }

__device__ __forceinline__ void yuv_rgb(int y, const ChromaTerms& c, const YuvCoef& k, int& r, int& g, int& b) {
  const int yi = k.cy * (y - k.yoff) + (1 << 15);
  r = sat8_shr16(yi + c.rv);
  g = sat8_shr16(yi + c.guv);
  b = sat8_shr16(yi + c.bu);
}

// R | G << 8 | B << 16
__device__ __forceinline__ uint32_t yuv_rgb_packed(int y, const ChromaTerms& c, const YuvCoef& k) {
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

// The conversion alone: dst row r = (f, y) <- source frame f (at byte f * fpitch); one wave per output row.  QUAD (W a multiple
// of 4, both pointers 4-byte aligned): a lane converts four adjacent pixels = two chroma samples from one 4-byte Y load and one
// 4-byte (NV12) or two 2-byte (I420) chroma loads, and stores their 12 bytes at once.  Otherwise a lane converts the pair that
// shares one chroma sample and stores three 2-byte pieces (`even`: dst is 2-byte aligned; rows and pairs are, as W is even) or bytes.
template <bool QUAD>
__global__ __launch_bounds__(256) void yuv420_to_rgb_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int H,
                                                              int W, int layout, YuvCoef k, int even, long long nrows) {
  const int lane = threadIdx.x & 63;
  const YuvLayout L(layout, H, W);
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / H;
    const int y = (int)(r - f * H);
    const uint8_t* yrow = src + f * fpitch + (long long)y * W;
    const uint8_t* cb = src + f * fpitch + (long long)H * W + (long long)(y >> 1) * L.cw;
    const uint8_t* cr = cb + L.cr_off;
    uint8_t* out = dst + r * W * 3;
    if constexpr (QUAD) {
      for (int q = lane; q < W / 4; q += 64) {
        const uint32_t yy = load_as<uint32_t>(yrow + 4 * q);
        uint32_t cc;  // Cb0 | Cr0 << 8 | Cb1 << 16 | Cr1 << 24
        if (layout == 0) {
          cc = load_as<uint32_t>(cb + 4 * q);
        } else {
          const uint32_t u = load_as<uint16_t>(cb + 2 * q), v = load_as<uint16_t>(cr + 2 * q);
          cc = (u & 255) | (v & 255) << 8 | (u >> 8) << 16 | (v >> 8) << 24;
        }
        const ChromaTerms c0(cc & 255, (cc >> 8) & 255, k), c1((cc >> 16) & 255, cc >> 24, k);
        const uint32_t p0 = yuv_rgb_packed(yy & 255, c0, k), p1 = yuv_rgb_packed((yy >> 8) & 255, c0, k);
        const uint32_t p2 = yuv_rgb_packed((yy >> 16) & 255, c1, k), p3 = yuv_rgb_packed(yy >> 24, c1, k);
        store_as(out + 12 * q, Rgb4{p0 | p1 << 24, p1 >> 8 | p2 << 16, p2 >> 16 | p3 << 8});
      }
    } else {
      for (int p = lane; p < W / 2; p += 64) {
        const ChromaTerms c(cb[p * L.cs], cr[p * L.cs], k);
        const uint32_t p0 = yuv_rgb_packed(yrow[2 * p], c, k), p1 = yuv_rgb_packed(yrow[2 * p + 1], c, k);
        uint8_t* o = out + 6 * p;
        if (even) {
          store_as(o, (uint16_t)p0);
          store_as(o + 2, (uint16_t)(p0 >> 16 | p1 << 8));
          store_as(o + 4, (uint16_t)(p1 >> 8));
        } else {
          o[0] = (uint8_t)p0, o[1] = (uint8_t)(p0 >> 8), o[2] = (uint8_t)(p0 >> 16);
          o[3] = (uint8_t)p1, o[4] = (uint8_t)(p1 >> 8), o[5] = (uint8_t)(p1 >> 16);
        }
      }
    }
  }
}

// resize_h_u8_kernel on 4:2:0 frames: every tap's pixel is converted to its three bytes first and accumulated as there, so the
// output is byte for byte that kernel's on the converted frame.  The taps [x0, x0 + n) are walked chroma sample by chroma sample:
// one chroma read and one set of products for the (up to) two taps that share it.
__global__ __launch_bounds__(256) void resize_h_yuv420_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long long fpitch, int H,
                                                                int W, int OW, int row0, int rows, const int* __restrict__ xb,
                                                                const int* __restrict__ xk, int ksize, int layout, YuvCoef k, long long nrows) {
  const int lane = threadIdx.x & 63;
  const YuvLayout L(layout, H, W);
  for (long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (long long)gridDim.x * 4) {
    const long long f = r / rows;
    const int y = row0 + (int)(r - f * rows);
    const uint8_t* yrow = src + f * fpitch + (long long)y * W;
    const uint8_t* cb = src + f * fpitch + (long long)H * W + (long long)(y >> 1) * L.cw;
    const uint8_t* cr = cb + L.cr_off;
    uint8_t* out = dst + r * OW * 3;
    for (int x = lane; x < OW; x += 64) {
      int x0 = xb[2 * x];
      int n = min(xb[2 * x + 1], ksize);
      if (x0 < 0 || x0 + n > W) x0 = 0, n = 0;  // (never for tables from resize.py: a guard against a foreign table)
      const int xe = x0 + n;
      const int* w = xk + (long long)x * ksize - x0;  // indexed by the source column
      int s0 = 1 << (RESIZE_BITS - 1), s1 = s0, s2 = s0;
      for (int xc = x0 >> 1; 2 * xc < xe; ++xc) {
        const ChromaTerms c(cb[xc * L.cs], cr[xc * L.cs], k);
#pragma unroll
        for (int xs = 2 * xc; xs < 2 * xc + 2; ++xs) {
          if (xs >= x0 && xs < xe) {
            int pr, pg, pb;
            yuv_rgb(yrow[xs], c, k, pr, pg, pb);
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
}

}  // namespace advhip

using namespace advhip;

static bool mul_ok(long long a, long long b, long long c, long long d, long long* out) {
  long long t;
  return !__builtin_mul_overflow(a, b, &t) && !__builtin_mul_overflow(t, c, &t) && !__builtin_mul_overflow(t, d, out);
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
  ADVHIP_REQUIRE(src && dst, "resize_u8: null frames or output");
  ADVHIP_REQUIRE(frame_step >= 1, "resize_u8: frame step %d", frame_step);
  // source frames 0, frame_step, 2 frame_step, ... -> a compact output (F_src < 1 is refused below)
  const int64_t F = F_src < 1 ? F_src : (F_src - 1) / frame_step + 1;
  ADVHIP_REQUIRE(F >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1, "resize_u8: sizes must be >= 1 (F=%lld, %d x %d -> %d x %d)",
                 (long long)F, H, W, OH, OW);
  ADVHIP_REQUIRE(C == 3, "resize_u8: frames must have 3 channels (RGB), got C=%d", C);
  const bool horiz = OW != W, vert = OH != H;
  long long in_bytes, out_bytes, ws_bytes = 0;
  ADVHIP_REQUIRE(mul_ok(F_src, H, W, C, &in_bytes) && mul_ok(F, OH, OW, C, &out_bytes), "resize_u8: frame sizes overflow int64");
  const long long frame_bytes = (long long)H * W * C, src_pitch = F > 1 ? frame_bytes * frame_step : frame_bytes;  // (F > 1: inside in_bytes)
  ADVHIP_REQUIRE((long long)W * C <= INT32_MAX && (long long)OW * C <= INT32_MAX, "resize_u8: rows of %d / %d pixels are too long", W, OW);
  if (horiz) {
    ADVHIP_REQUIRE(xbounds && xcoef, "resize_u8: null horizontal tables");
    ADVHIP_REQUIRE(xksize >= 1, "resize_u8: horizontal ksize %d < 1", xksize);
    ADVHIP_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= H, "resize_u8: rows [%d, %lld) of the horizontal pass outside the %d-row frames",
                   row0, (long long)row0 + rows, H);
    ADVHIP_REQUIRE(vert || (row0 == 0 && rows == H), "resize_u8: without a vertical pass the horizontal pass must compute all %d rows", H);
    ADVHIP_REQUIRE(mul_ok(F, rows, OW, C, &ws_bytes), "resize_u8: workspace size overflows int64");
    ADVHIP_REQUIRE(ws || !vert, "resize_u8: null workspace for the horizontal pass (%lld bytes)", ws_bytes);
  }
  if (vert) {
    ADVHIP_REQUIRE(ybounds && ycoef, "resize_u8: null vertical tables");
    ADVHIP_REQUIRE(yksize >= 1, "resize_u8: vertical ksize %d < 1", yksize);
  }
  hipStream_t s = (hipStream_t)stream;
  if (!horiz && !vert) {  // Pillow returns a copy
    hipError_t e = hipSuccess;
    if (frame_step > 1) e = hipMemcpy2DAsync(dst, (size_t)frame_bytes, src, (size_t)src_pitch, (size_t)frame_bytes, (size_t)F, hipMemcpyDeviceToDevice, s);
    else if (src != dst) e = hipMemcpyAsync(dst, src, (size_t)in_bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      set_error("resize_u8 copy: %s", hipGetErrorString(e));
      return ADVHIP_ELAUNCH;
    }
    return ADVHIP_OK;
  }
  if (horiz) {
    const long long nrows = F * rows;
    const int grid = (int)std::min<long long>((nrows + 3) / 4, 256 * 256);
    hipLaunchKernelGGL(resize_h_u8_kernel, dim3(grid), dim3(256), 0, s, src, vert ? ws : dst, src_pitch, W, OW, row0, rows, xbounds, xcoef, xksize,
                       nrows);
    const int rc = check_launch("resize_u8 horizontal pass");
    if (rc != ADVHIP_OK) return rc;
  }
  if (vert) {
    const long long nrows = F * OH;
    const int grid = (int)std::min<long long>((nrows + 3) / 4, 256 * 256);
    hipLaunchKernelGGL(resize_v_u8_kernel, dim3(grid), dim3(256), 0, s, horiz ? (const uint8_t*)ws : src, dst,
                       horiz ? (long long)rows * OW * C : src_pitch, horiz ? rows : H, OH, OW * C,
                       horiz ? row0 : 0, ybounds, ycoef, yksize, nrows);
    return check_launch("resize_u8 vertical pass");
  }
  return ADVHIP_OK;
}

// the checks both 4:2:0 entry points share: even geometry, a known layout, coefficients that keep every int32 sum exact
static int check_yuv420(const char* who, int32_t H, int32_t W, int32_t layout, const YuvCoef& k) {
  ADVHIP_REQUIRE(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "%s: 4:2:0 frames need even H and W >= 2, got %d x %d", who, H, W);
  ADVHIP_REQUIRE(layout == ADVHIP_YUV420_NV12 || layout == ADVHIP_YUV420_I420, "%s: layout %d is neither NV12 (0) nor I420 (1)", who, layout);
  ADVHIP_REQUIRE(k.yoff == 0 || k.yoff == 16, "%s: luma offset %d is neither 0 (full range) nor 16 (limited range)", who, k.yoff);
  const int lim = 1 << 18;
  ADVHIP_REQUIRE(k.cy > 0 && k.cy < lim, "%s: luma coefficient %d outside (0, 2^18)", who, k.cy);
  ADVHIP_REQUIRE(k.crv >= 0 && k.crv < lim && k.cgu >= 0 && k.cgu < lim && k.cgv >= 0 && k.cgv < lim && k.cbu >= 0 && k.cbu < lim,
                 "%s: chroma coefficients (%d, %d, %d, %d) outside [0, 2^18)", who, k.crv, k.cgu, k.cgv, k.cbu);
  return ADVHIP_OK;
}

// (every argument checked by the caller) frames 0, frame_step, ... of src -> compact RGB frames in dst
static int launch_yuv420_to_rgb(const uint8_t* src, uint8_t* dst, long long F, long long src_pitch, int H, int W, int layout, const YuvCoef& k,
                                hipStream_t s) {
  const long long nrows = F * H;
  const int grid = (int)std::min<long long>((nrows + 3) / 4, 256 * 256);
  const bool quad = W % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0;  // (a frame is 3 H / 2 * W bytes: a multiple of 4 then)
  if (quad) hipLaunchKernelGGL(yuv420_to_rgb_u8_kernel<true>, dim3(grid), dim3(256), 0, s, src, dst, src_pitch, H, W, layout, k, 1, nrows);
  else
    hipLaunchKernelGGL(yuv420_to_rgb_u8_kernel<false>, dim3(grid), dim3(256), 0, s, src, dst, src_pitch, H, W, layout, k,
                       (int)((uintptr_t)dst % 2 == 0), nrows);
  return check_launch("yuv420_to_rgb_u8");
}

extern "C" int advhip_yuv420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t F_src, int32_t frame_step, int32_t H, int32_t W, int32_t layout,
                                       int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  const YuvCoef k{yoff, cy, crv, cgu, cgv, cbu};
  ADVHIP_REQUIRE(src && dst, "yuv420_to_rgb_u8: null frames or output");
  ADVHIP_REQUIRE(frame_step >= 1, "yuv420_to_rgb_u8: frame step %d", frame_step);
  const int64_t F = F_src < 1 ? F_src : (F_src - 1) / frame_step + 1;
  ADVHIP_REQUIRE(F >= 1, "yuv420_to_rgb_u8: %lld frames", (long long)F_src);
  if (const int rc = check_yuv420("yuv420_to_rgb_u8", H, W, layout, k); rc != ADVHIP_OK) return rc;
  long long in_bytes, out_bytes, pitch;
  ADVHIP_REQUIRE(mul_ok(F_src, H / 2, W, 3, &in_bytes) && mul_ok(F, H, W, 3, &out_bytes) && mul_ok(H / 2, W, 3, frame_step, &pitch),
                 "yuv420_to_rgb_u8: frame sizes overflow int64");
  ADVHIP_REQUIRE((long long)W * 3 <= INT32_MAX, "yuv420_to_rgb_u8: rows of %d pixels are too long", W);
  return launch_yuv420_to_rgb(src, dst, F, F > 1 ? pitch : 0, H, W, layout, k, (hipStream_t)stream);
}

extern "C" int advhip_resize_yuv420_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int32_t H, int32_t W,
                                       int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                                       const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, int32_t layout,
                                       int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream) {
  const YuvCoef k{yoff, cy, crv, cgu, cgv, cbu};
  ADVHIP_REQUIRE(src && dst, "resize_yuv420_u8: null frames or output");
  ADVHIP_REQUIRE(frame_step >= 1, "resize_yuv420_u8: frame step %d", frame_step);
  const int64_t F = F_src < 1 ? F_src : (F_src - 1) / frame_step + 1;
  ADVHIP_REQUIRE(F >= 1 && OH >= 1 && OW >= 1, "resize_yuv420_u8: sizes must be >= 1 (F=%lld, -> %d x %d)", (long long)F, OH, OW);
  ADVHIP_REQUIRE(C == 3, "resize_yuv420_u8: the output has 3 channels (RGB), got C=%d", C);
  if (const int rc = check_yuv420("resize_yuv420_u8", H, W, layout, k); rc != ADVHIP_OK) return rc;
  const bool horiz = OW != W, vert = OH != H;
  long long in_bytes, out_bytes, rgb_bytes, src_pitch, ws_bytes = 0;
  ADVHIP_REQUIRE(mul_ok(F_src, H / 2, W, 3, &in_bytes) && mul_ok(F, OH, OW, C, &out_bytes) && mul_ok(F, H, W, C, &rgb_bytes) &&
                     mul_ok(H / 2, W, 3, frame_step, &src_pitch),
                 "resize_yuv420_u8: frame sizes overflow int64");
  if (F == 1) src_pitch = 0;  // (F > 1: inside in_bytes)
  ADVHIP_REQUIRE((long long)W * C <= INT32_MAX && (long long)OW * C <= INT32_MAX, "resize_yuv420_u8: rows of %d / %d pixels are too long", W, OW);
  if (horiz) {
    ADVHIP_REQUIRE(xbounds && xcoef, "resize_yuv420_u8: null horizontal tables");
    ADVHIP_REQUIRE(xksize >= 1, "resize_yuv420_u8: horizontal ksize %d < 1", xksize);
    ADVHIP_REQUIRE(row0 >= 0 && rows >= 1 && (long long)row0 + rows <= H,
                   "resize_yuv420_u8: rows [%d, %lld) of the horizontal pass outside the %d-row frames", row0, (long long)row0 + rows, H);
    ADVHIP_REQUIRE(vert || (row0 == 0 && rows == H), "resize_yuv420_u8: without a vertical pass the horizontal pass must compute all %d rows", H);
    ADVHIP_REQUIRE(mul_ok(F, rows, OW, C, &ws_bytes), "resize_yuv420_u8: workspace size overflows int64");
    ADVHIP_REQUIRE(ws || !vert, "resize_yuv420_u8: null workspace for the horizontal pass (%lld bytes)", ws_bytes);
  } else if (vert) {
    ADVHIP_REQUIRE(ws, "resize_yuv420_u8: null workspace for the converted frames of a vertical-only resize (%lld bytes)", rgb_bytes);
  }
  if (vert) {
    ADVHIP_REQUIRE(ybounds && ycoef, "resize_yuv420_u8: null vertical tables");
    ADVHIP_REQUIRE(yksize >= 1, "resize_yuv420_u8: vertical ksize %d < 1", yksize);
  }
  hipStream_t s = (hipStream_t)stream;
  if (horiz) {
    const long long nrows = F * rows;
    const int grid = (int)std::min<long long>((nrows + 3) / 4, 256 * 256);
    hipLaunchKernelGGL(resize_h_yuv420_u8_kernel, dim3(grid), dim3(256), 0, s, src, vert ? ws : dst, src_pitch, H, W, OW, row0, rows, xbounds, xcoef,
                       xksize, layout, k, nrows);
    const int rc = check_launch("resize_yuv420_u8 horizontal pass");
    if (rc != ADVHIP_OK) return rc;
  } else {  // rare: the conversion launch, into dst (the identity) or into the workspace the vertical pass then reads
    const int rc = launch_yuv420_to_rgb(src, vert ? ws : dst, F, src_pitch, H, W, layout, k, s);
    if (rc != ADVHIP_OK) return rc;
  }
  if (vert) {  // the RGB resize's own vertical pass
    const long long nrows = F * OH;
    const int grid = (int)std::min<long long>((nrows + 3) / 4, 256 * 256);
    hipLaunchKernelGGL(resize_v_u8_kernel, dim3(grid), dim3(256), 0, s, (const uint8_t*)ws, dst, horiz ? (long long)rows * OW * C : (long long)H * W * C,
                       horiz ? rows : H, OH, OW * C, horiz ? row0 : 0, ybounds, ycoef, yksize, nrows);
    return check_launch("resize_yuv420_u8 vertical pass");
  }
  return ADVHIP_OK;
}
