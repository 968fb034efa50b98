// The normalisation modes of the uint8-frame path (src/gtransforms.py:57-112): per-channel standardisation and the two min-max
// normalisers, whose statistics are taken per (frame, crop[, channel]) over the crop's pixels before any pixel can be written.
//   crop_minmax_u8                      : (min, max) per channel of the six TenCrop windows of every pitch-th frame
//   tencrop_normalize[_planes]_u8_modes : the two TenCrop passes of misc.hip with a mode, per-channel constants and that table
// The default normalisation ((x - 114.75) / 57.375, one scalar pair) stays on misc.hip's kernels and entry points.
#include <algorithm>

#include "common.h"

namespace advhip {

// ---- statistics ----------------------------------------------------------------------------------------------------------------

// (min, max) of up to three running values over the workgroup's four waves: cross-lane butterflies within a wave, then one LDS
// round across the waves.  Integer min / max: exact, and the same bits whatever the order.  Thread k < 2 * nv of the workgroup
// ends up with value k / 2's minimum (k even) or maximum (k odd) in *out; returns whether this thread holds one.
__device__ __forceinline__ bool block_minmax(int (&mn)[3], int (&mx)[3], int nv, int* lds /* [4][6] */, int* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      mn[k] = min(mn[k], __shfl_xor(mn[k], off, 64));
      mx[k] = max(mx[k], __shfl_xor(mx[k], off, 64));
    }
  }
  __syncthreads();  // (the previous round's readers are done with lds)
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lds[wave * 6 + 2 * k] = mn[k];
      lds[wave * 6 + 2 * k + 1] = mx[k];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= 2 * nv) return false;
  int v = lds[t];
#pragma unroll
  for (int w = 1; w < 4; ++w) v = (t & 1) ? max(v, lds[w * 6 + t]) : min(v, lds[w * 6 + t]);
  *out = v;
  return true;
}

// The pixel SETS of TenCrop's ten crops are six windows of the frame: the four corners, the centre, and the centre of the mirrored
// frame, whose left edge W - cs - cleft is the centre's only where W - cs is even (the Python-rounded half of an odd difference is
// not its own mirror image).  A mirrored corner crop holds the pixels of the opposite corner's window.
__device__ __forceinline__ int crop_window(int crop) { return crop < 5 ? crop : (crop == 9 ? 5 : (crop - 5) ^ 1); }

// One workgroup per (statistics frame i, window j): frame i * pitch, window j of those six (top-left, top-right, bottom-left,
// bottom-right, centre, mirrored centre).  stats[((i * 6 + j) * C + c) * 2 + {0, 1}] = (min, max) of channel c.  Wave w takes the
// window's rows w, w + 4, ...: a row is cs * C consecutive bytes that start anywhere.
// WIDE3 (C == 3): the bytes in front of the first 4-byte boundary and behind the last whole 12-byte group go one per lane; between
// them lane q reads the 12 bytes of group q as three aligned dwords.  12 = lcm(3, 4): byte e of every group of a row belongs to
// channel (head + e) % 3, so a lane folds its twelve bytes into three phase accumulators and the phase -> channel rotation
// happens once per row, on wave-uniform `head`.  Every load lies inside the row.
// Otherwise: one pass per channel, one byte per lane.
template <bool WIDE3>
__global__ __launch_bounds__(256) void crop_minmax_u8_kernel(const uint8_t* __restrict__ x, uint8_t* __restrict__ stats, int H, int W, int C,
                                                             int cs, int ctop, int cleft, int pitch) {
  __shared__ int lds[24];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x / 6, j = blockIdx.x % 6;
  const int top = j >= 4 ? ctop : ((j >> 1) ? H - cs : 0), left = j == 4 ? cleft : (j == 5 ? W - cs - cleft : ((j & 1) ? W - cs : 0));
  const uint8_t* win = x + (((long long)i * pitch * H + top) * W + left) * C;
  const long long rpitch = (long long)W * C;
  uint8_t* out = stats + ((long long)i * 6 + j) * C * 2;
  int res;
  if constexpr (WIDE3) {
    int mn[3] = {255, 255, 255}, mx[3] = {0, 0, 0};  // by channel
    const int n = cs * 3;
    for (int y = wave; y < cs; y += 4) {
      const uint8_t* row = win + y * rpitch;
      const int head = min(n, (int)((4 - ((uintptr_t)row & 3)) & 3));
      const int groups = (n - head) / 12, edge = n - groups * 12;  // edge bytes: `head` in front, the rest behind the groups
      int pmn[3] = {255, 255, 255}, pmx[3] = {0, 0, 0};  // by phase: byte e of a group -> e % 3
      const uint32_t* body = reinterpret_cast<const uint32_t*>(row + head);
      for (int q = lane; q < groups; q += 64) {
        const uint32_t a = body[3 * q], b = body[3 * q + 1], c = body[3 * q + 2];
        // bytes 0..11 of the group: phases 0 1 2 0 | 1 2 0 1 | 2 0 1 2
        const int b0 = a & 0xff, b1 = (a >> 8) & 0xff, b2 = (a >> 16) & 0xff, b3 = a >> 24;
        const int b4 = b & 0xff, b5 = (b >> 8) & 0xff, b6 = (b >> 16) & 0xff, b7 = b >> 24;
        const int b8 = c & 0xff, b9 = (c >> 8) & 0xff, b10 = (c >> 16) & 0xff, b11 = c >> 24;
        pmn[0] = min(min(pmn[0], min(b0, b3)), min(b6, b9));
        pmx[0] = max(max(pmx[0], max(b0, b3)), max(b6, b9));
        pmn[1] = min(min(pmn[1], min(b1, b4)), min(b7, b10));
        pmx[1] = max(max(pmx[1], max(b1, b4)), max(b7, b10));
        pmn[2] = min(min(pmn[2], min(b2, b5)), min(b8, b11));
        pmx[2] = max(max(pmx[2], max(b2, b5)), max(b8, b11));
      }
      // phase k of this row is channel (head + k) % 3
      const int h3 = head % 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int pk = (k + 3 - h3) % 3;  // the phase that holds channel k
        const int vmn = pk == 0 ? pmn[0] : (pk == 1 ? pmn[1] : pmn[2]), vmx = pk == 0 ? pmx[0] : (pk == 1 ? pmx[1] : pmx[2]);
        mn[k] = min(mn[k], vmn);
        mx[k] = max(mx[k], vmx);
      }
      if (lane < edge) {  // (edge <= 3 + 11)
        const int idx = lane < head ? lane : groups * 12 + lane;
        const int b = row[idx], ch = idx % 3;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (ch == k) {
            mn[k] = min(mn[k], b);
            mx[k] = max(mx[k], b);
          }
      }
    }
    if (block_minmax(mn, mx, 3, lds, &res)) out[threadIdx.x] = (uint8_t)res;
  } else {
    for (int c = 0; c < C; ++c) {
      int mn[3] = {255, 255, 255}, mx[3] = {0, 0, 0};  // (only [0] is used)
      for (int y = wave; y < cs; y += 4) {
        const uint8_t* row = win + y * rpitch + c;
        for (int q = lane; q < cs; q += 64) {
          const int b = row[(long long)q * C];
          mn[0] = min(mn[0], b);
          mx[0] = max(mx[0], b);
        }
      }
      if (block_minmax(mn, mx, 1, lds, &res)) out[2 * c + threadIdx.x] = (uint8_t)res;
    }
  }
}

// ---- the two TenCrop passes with a mode ---------------------------------------------------------------------------------------

// Per-channel constants as the kernels take them (by value).  Standardisation: y = (x - sub) / div with (sub, div) = (mean[c],
// std[c]).  Min-max: y = (x - mn) / (mx - mn) * r[c] + lo[c] with (mn, mx) from the statistics table, of channel c
// (ADVHIP_NORM_CHANNEL_MINMAX) or over all channels (ADVHIP_NORM_PIXEL_MINMAX).
struct NormConsts {
  float a[3], b[3];  // (mean, std) or (lo, r)
};

// What one output row (one frame, one crop, one channel) needs: looked up once per wave-row.
struct RowNorm {
  float sub, div, r, lo;
};

template <bool MM>
__device__ __forceinline__ RowNorm row_norm(const NormConsts& k, int mode, const uint8_t* __restrict__ stats, int spitch, int f, int crop,
                                            int c, int C) {
  RowNorm n;
  if constexpr (!MM) {
    n.sub = k.a[c];
    n.div = k.b[c];
    n.r = 0.f;
    n.lo = 0.f;
  } else {
    const uint8_t* s = stats + ((long long)(f / spitch) * 6 + crop_window(crop)) * C * 2;
    int mn = s[2 * c], mx = s[2 * c + 1];
    if (mode == ADVHIP_NORM_PIXEL_MINMAX)
      for (int cc = 0; cc < C; ++cc) {
        mn = min(mn, (int)s[2 * cc]);
        mx = max(mx, (int)s[2 * cc + 1]);
      }
    n.sub = (float)mn;
    n.div = (float)mx - (float)mn;  // (exact; 0 for a constant crop / channel: 0 / 0 = NaN, as the reference gives)
    n.r = k.b[c];
    n.lo = k.a[c];
  }
  return n;
}

// Separately rounded operations throughout: a true division (no reciprocal multiply), and q * r + lo as a multiply and an add.
// hipcc contracts that pair into one FMA by default (and its __fmul_rn / __fadd_rn are the plain operators, contracted alike),
// which changes about a fifth of the outputs at (lo, hi) = (0.1, 0.7): contraction is switched off for this function, and the
// instructions keep that when it is inlined.
template <bool MM>
__device__ __forceinline__ float apply_norm(const RowNorm& n, uint8_t px) {
#pragma clang fp contract(off)
  const float q = ((float)px - n.sub) / n.div;
  if constexpr (!MM) {
    return q;
  } else {
    const float m = q * n.r;
    return m + n.lo;
  }
}

// tencrop_normalize_u8_kernel (misc.hip) with the mode: the same row decode, LoopPad rule, crop nibbles and frame_step addressing.
template <int VW, bool MM>
__global__ __launch_bounds__(256) void tencrop_normalize_u8_modes_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, int F, int H, int W,
                                                                         int C, int fpc, int cstride, int cs, int ctop, int cleft,
                                                                         long long rows, int nc, unsigned long long crops, int fstep,
                                                                         int mode, NormConsts k, const uint8_t* __restrict__ stats,
                                                                         int spitch) {
  const int lane = threadIdx.x & 63;
  const int csv = cs / VW;
  for (long long r0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r0 < rows; r0 += (long long)gridDim.x * 4) {
    long long r = r0;  // output order: (clip, crop, c, t, y, x)
    const int yo = (int)(r % cs);
    r /= cs;
    const int t = (int)(r % fpc);
    r /= fpc;
    const int c = (int)(r % C);
    r /= C;
    const int clip = (int)(r / nc);
    const int crop = (int)(crops >> (4 * (int)(r - (long long)clip * nc))) & 15;
    const int len = min(fpc, (F - clip * cstride + fstep - 1) / fstep);
    const int f = clip * cstride + (t % len) * fstep;
    const int j = crop % 5;
    const int top = j == 4 ? ctop : ((j >> 1) ? H - cs : 0), left = j == 4 ? cleft : ((j & 1) ? W - cs : 0);
    const RowNorm n = row_norm<MM>(k, mode, stats, spitch, f, crop, c, C);
    const uint8_t* row = x + (((long long)f * H + top + yo) * W) * C + c;
    float* out = y + r0 * cs;
    for (int q = lane; q < csv; q += 64) {
      float v[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) {
        const int xo = q * VW + e;
        const int sx = crop < 5 ? left + xo : W - 1 - (left + xo);
        v[e] = apply_norm<MM>(n, row[(long long)sx * C]);
      }
      if constexpr (VW == 4) reinterpret_cast<float4*>(out)[q] = make_float4(v[0], v[1], v[2], v[3]);
      else out[q] = v[0];
    }
  }
}

// tencrop_normalize_planes_u8_kernel (misc.hip) with the mode; the padding columns stay zero.
template <bool MM>
__global__ __launch_bounds__(256) void tencrop_normalize_planes_u8_modes_kernel(const uint8_t* __restrict__ x, float* __restrict__ xs, int F,
                                                                                int H, int W, int C, int fpc, int cstride, int cs, int ctop,
                                                                                int cleft, long long first, long long rows, int WP, int nc,
                                                                                unsigned long long crops, int fstep, int mode, NormConsts k,
                                                                                const uint8_t* __restrict__ stats, int spitch) {
  const int lane = threadIdx.x & 63;
  for (long long r0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r0 < rows; r0 += (long long)gridDim.x * 4) {
    long long r = r0;  // (clip-crop - first, c, t, y)
    const int yo = (int)(r % cs);
    r /= cs;
    const int t = (int)(r % fpc);
    r /= fpc;
    const int c = (int)(r % C);
    r = r / C + first;
    const int clip = (int)(r / nc);
    const int crop = (int)(crops >> (4 * (int)(r - (long long)clip * nc))) & 15;
    const int len = min(fpc, (F - clip * cstride + fstep - 1) / fstep);
    const int f = clip * cstride + (t % len) * fstep;
    const int j5 = crop % 5;
    const int top = j5 == 4 ? ctop : ((j5 >> 1) ? H - cs : 0), left = j5 == 4 ? cleft : ((j5 & 1) ? W - cs : 0);
    const RowNorm n = row_norm<MM>(k, mode, stats, spitch, f, crop, c, C);
    const uint8_t* row = x + (((long long)f * H + top + yo) * W) * C + c;
    float* out = xs + r0 * 2 * WP;
    for (int q = lane; q < 2 * WP; q += 64) {
      const int par = q >= WP, idx = q - par * WP, xo = 2 * (idx - 2) + par;
      float v = 0.f;
      if (idx >= 2 && xo < cs) {
        const int sx = crop < 5 ? left + xo : W - 1 - (left + xo);
        v = apply_norm<MM>(n, row[(long long)sx * C]);
      }
      out[q] = v;
    }
  }
}

// The checks the two `_modes` passes share beyond the scalar passes' own, and the constants the kernels take.  `a`, `b`: host
// triples of doubles -- (mean, std) or (lo, hi) per channel, as the caller states them, so that the range is rounded as the
// reference rounds it: pixel mode r = float(hi - lo) with the subtraction in double, channel mode r = float(hi) - float(lo).
static int norm_consts(const char* who, int mode, const double* a, const double* b, const uint8_t* stats, int stats_pitch, int C,
                       const ClipSampling& s, NormConsts* k) {
  ADVHIP_REQUIRE(mode == ADVHIP_NORM_STANDARDIZE || mode == ADVHIP_NORM_PIXEL_MINMAX || mode == ADVHIP_NORM_CHANNEL_MINMAX,
                 "%s: unknown normalisation mode %d", who, mode);
  ADVHIP_REQUIRE(a && b, "%s: null constants", who);
  ADVHIP_REQUIRE(C <= 3, "%s: the per-channel constants are triples, C = %d", who, C);
  if (mode == ADVHIP_NORM_STANDARDIZE) {
    for (int c = 0; c < 3; ++c) {
      k->a[c] = (float)a[c];
      k->b[c] = (float)b[c];
      ADVHIP_REQUIRE(k->b[c] != 0.f, "%s: std must be non-zero (channel %d)", who, c);
    }
    return ADVHIP_OK;
  }
  bool any = false;
  for (int c = 0; c < 3; ++c) {
    // (negated comparisons: a NaN bound is refused too)
    ADVHIP_REQUIRE(mode != ADVHIP_NORM_PIXEL_MINMAX || a[c] < b[c], "%s: range [%g, %g]: min must be below max", who, a[c], b[c]);
    any = any || a[c] < b[c];
    k->a[c] = (float)a[c];
    k->b[c] = mode == ADVHIP_NORM_PIXEL_MINMAX ? (float)(b[c] - a[c]) : (float)b[c] - (float)a[c];
  }
  ADVHIP_REQUIRE(any, "%s: range: min must be below max in at least one channel", who);
  ADVHIP_REQUIRE(stats, "%s: the min-max modes need the statistics table", who);
  ADVHIP_REQUIRE(stats_pitch >= 1, "%s: stats pitch %d", who, stats_pitch);
  ADVHIP_REQUIRE(s.clip_stride % stats_pitch == 0 && s.frame_step % stats_pitch == 0,
                 "%s: stats pitch %d does not divide clip stride %d and frame step %d", who, stats_pitch, s.clip_stride, s.frame_step);
  return ADVHIP_OK;
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_crop_minmax_u8(const uint8_t* frames, uint8_t* stats, int32_t F, int32_t H, int32_t W, int32_t C, int32_t crop,
                                     int32_t frame_pitch, void* stream) {
  const char* who = "crop_minmax_u8";
  ADVHIP_REQUIRE(frames && stats, "%s: null pointer", who);
  ADVHIP_REQUIRE(F > 0 && H > 0 && W > 0 && C > 0 && crop > 0, "%s: bad arguments", who);
  ADVHIP_REQUIRE(frame_pitch >= 1, "%s: frame pitch %d", who, frame_pitch);
  ADVHIP_REQUIRE(H >= crop && W >= crop, "%s: frames (%d x %d) smaller than the %d crop", who, H, W, crop);
  ADVHIP_REQUIRE((long long)crop * C < (1ll << 30), "%s: crop rows of %lld bytes", who, (long long)crop * C);
  const long long nf = ((long long)F + frame_pitch - 1) / frame_pitch;
  ADVHIP_REQUIRE(nf * 6 < (1ll << 31), "%s: too many frames", who);
  const int ctop = half_even(H - crop), cleft = half_even(W - crop);
  if (C == 3) hipLaunchKernelGGL(crop_minmax_u8_kernel<true>, dim3((unsigned)(nf * 6)), dim3(256), 0, (hipStream_t)stream, frames, stats, H, W, C,
                                 crop, ctop, cleft, frame_pitch);
  else hipLaunchKernelGGL(crop_minmax_u8_kernel<false>, dim3((unsigned)(nf * 6)), dim3(256), 0, (hipStream_t)stream, frames, stats, H, W, C, crop,
                          ctop, cleft, frame_pitch);
  return check_launch(who);
}

extern "C" int advhip_tencrop_normalize_u8_modes(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                                 int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                 int32_t ncrops, uint64_t crops_packed, int32_t mode, const double* a, const double* b,
                                                 const uint8_t* stats, int32_t stats_pitch, void* stream) {
  const char* who = "tencrop_normalize_u8_modes";
  const ClipSampling s{frames_per_clip, clip_stride, frame_step, ncrops, crops_packed};
  if (int rc = s.check_crops(who)) return rc;
  ADVHIP_REQUIRE(frames && y, "%s: null pointer", who);
  ADVHIP_REQUIRE(F > 0 && C > 0 && s.fpc > 0 && crop > 0, "%s: bad arguments", who);
  if (int rc = s.check_windows(who, 1ll << 31)) return rc;
  ADVHIP_REQUIRE(H >= crop && W >= crop, "%s: frames (%d x %d) smaller than the %d crop", who, H, W, crop);
  NormConsts k;
  if (int rc = norm_consts(who, mode, a, b, stats, stats_pitch, C, s, &k)) return rc;
  const int ctop = half_even(H - crop), cleft = half_even(W - crop);
  const bool vec = crop % 4 == 0 && ((uintptr_t)y & 15) == 0, mm = mode != ADVHIP_NORM_STANDARDIZE;
  const long long rows = s.video_windows(F) * s.ncrops * C * s.fpc * (long long)crop;
  const int grid = (int)std::min<long long>((rows + 3) / 4, 256 * 256);
#define ADVHIP_LAUNCH_MODES(VW, MM)                                                                                                          \
  hipLaunchKernelGGL((tencrop_normalize_u8_modes_kernel<VW, MM>), dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, y, F, H, W, C, s.fpc, \
                     s.clip_stride, crop, ctop, cleft, rows, s.ncrops, s.crops, s.frame_step, mode, k, stats, stats_pitch)
  if (vec && mm) ADVHIP_LAUNCH_MODES(4, true);
  else if (vec) ADVHIP_LAUNCH_MODES(4, false);
  else if (mm) ADVHIP_LAUNCH_MODES(1, true);
  else ADVHIP_LAUNCH_MODES(1, false);
#undef ADVHIP_LAUNCH_MODES
  return check_launch(who);
}

extern "C" int advhip_tencrop_normalize_planes_u8_modes(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                        int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                        int32_t ncrops, uint64_t crops_packed, int64_t first_crop_clip, int64_t count,
                                                        int32_t mode, const double* a, const double* b, const uint8_t* stats,
                                                        int32_t stats_pitch, void* stream) {
  const char* who = "tencrop_normalize_planes_u8_modes";
  const ClipSampling s{frames_per_clip, clip_stride, frame_step, ncrops, crops_packed};
  if (int rc = s.check_crops(who)) return rc;
  ADVHIP_REQUIRE(frames && xs, "%s: null pointer", who);
  ADVHIP_REQUIRE(F > 0 && C > 0 && s.fpc > 0 && crop > 0 && crop % 2 == 0, "%s: bad arguments", who);
  if (int rc = s.check_windows(who, 1ll << 31)) return rc;
  ADVHIP_REQUIRE(H >= crop && W >= crop, "%s: frames (%d x %d) smaller than the %d crop", who, H, W, crop);
  NormConsts k;
  if (int rc = norm_consts(who, mode, a, b, stats, stats_pitch, C, s, &k)) return rc;
  const long long n_clips = s.video_windows(F);
  ADVHIP_REQUIRE(first_crop_clip >= 0 && count > 0 && first_crop_clip + count <= n_clips * s.ncrops,
                 "%s: crop-clips [%lld, %lld) outside the video's %lld", who, (long long)first_crop_clip,
                 (long long)(first_crop_clip + count), n_clips * s.ncrops);
  const long long rows = (long long)count * C * s.fpc * crop;
  const int grid = (int)std::min<long long>((rows + 3) / 4, 256 * 256);
  const int ctop = half_even(H - crop), cleft = half_even(W - crop);
  if (mode != ADVHIP_NORM_STANDARDIZE)
    hipLaunchKernelGGL(tencrop_normalize_planes_u8_modes_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, xs, F, H, W, C,
                       s.fpc, s.clip_stride, crop, ctop, cleft, (long long)first_crop_clip, rows, crop / 2 + 4, s.ncrops, s.crops,
                       s.frame_step, mode, k, stats, stats_pitch);
  else
    hipLaunchKernelGGL(tencrop_normalize_planes_u8_modes_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, frames, xs, F, H, W, C,
                       s.fpc, s.clip_stride, crop, ctop, cleft, (long long)first_crop_clip, rows, crop / 2 + 4, s.ncrops, s.crops,
                       s.frame_step, mode, k, stats, stats_pitch);
  return check_launch(who);
}
