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
