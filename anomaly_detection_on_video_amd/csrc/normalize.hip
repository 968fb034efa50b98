// The uint8-frame front end: TenCrop + float + normalise + LoopPad + permute from resized frames, in every sampling (clip_stride,
// crops, frame_step) and with each of the reference's normalisers (src/gtransforms.py:57-112): the scalar pair (x - 114.75) / 57.375,
// per-channel standardisation, and the two min-max normalisers, whose statistics are taken per (frame, crop[, channel]) over the
// crop's pixels before any pixel can be written.
//   crop_minmax_u8               : (min, max) per channel of the six TenCrop windows of every pitch-th frame
//   tencrop_normalize[_planes]_u8: ONE row decode (crop_row), two writers (dense rows, column-parity planes), three normaliser
//                                  policies, one host launcher behind the ten entry points (plain / _strided / _crops / _sampled /
//                                  _modes of each writer)
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

// ---- the TenCrop passes -------------------------------------------------------------------------------------------------------

// TenCrop + float + normalise + LoopPad + permute in one pass (src/gtransforms.py:20-73, 115-132; src/dataset.py:175-195;
// extract_features.py:83): resized uint8 frames (F, H, W, C) -- the HWC bytes a decoder / PIL hands over -- to the backbone's
// input (n_clips * nc, C, fpc, cs, cs) fp32, or to column-parity planes of it.  One wave per output row (clip, crop, c, t, y): the
// row decode (five divisions) and the normaliser's lookup happen once per row, the lanes run along x (the first form decoded
// every float4 separately and indexed a by-value crop table: 165 us for 40 crop-clips, VALU-bound at 2.3 TB/s).

// The launch scalars of a pass.  (ctop, cleft): the centre crop's offsets, Python-rounded halves (half_even).
struct TenCrop {
  int F, H, W, C, fpc, cstride, fstep, cs, ctop, cleft, nc;
  unsigned long long crops;
};

// One output row: channel c of crop `crop` of source frame f; pixel x of it is at(g, x).
struct CropRow {
  const uint8_t* src;  // channel c of the first pixel of the frame row the crop row lies in
  int f, crop, c, left;

  // crops 5..9 are the five windows of the horizontally flipped frame: pixel (y, x) = frame[top + y][W - 1 - (left + x)]
  __device__ __forceinline__ uint8_t at(const TenCrop& g, int xo) const {
    const int sx = crop < 5 ? left + xo : g.W - 1 - (left + xo);
    return src[(long long)sx * g.C];
  }
};

// THE row decode: output row r = (clip-crop - first, c, t, y) of a pass that starts at crop-clip `first`.
//   clip-crop k = clip * nc + j holds crop (crops >> 4 j) & 15 of that clip (a crop SUBSET: nc of the ten, ascending, as nibbles
//     of one argument -- the same arithmetic per pixel, so the row is the ten-crop pass's row clip * 10 + that crop);
//   frame t of clip w = frames[w * cstride + (t % len_w) * fstep], len_w = min(fpc, ceil((F - w * cstride) / fstep)) (LoopPad: a
//     short last clip repeats itself); cstride = the distance between clip starts, fstep = the temporal sampling step;
//   crop j % 5 = the (top, left) window: top-left, top-right, bottom-left, bottom-right, centre (torchvision five_crop order).
__device__ __forceinline__ CropRow crop_row(const uint8_t* __restrict__ x, const TenCrop& g, long long r, long long first) {
  const int yo = (int)(r % g.cs);
  r /= g.cs;
  const int t = (int)(r % g.fpc);
  r /= g.fpc;
  const int c = (int)(r % g.C);
  r = r / g.C + first;
  const int clip = (int)(r / g.nc);
  const int crop = (int)(g.crops >> (4 * (int)(r - (long long)clip * g.nc))) & 15;
  const int len = min(g.fpc, (g.F - clip * g.cstride + g.fstep - 1) / g.fstep);
  const int f = clip * g.cstride + (t % len) * g.fstep;
  const int j = crop % 5;
  const int top = j == 4 ? g.ctop : ((j >> 1) ? g.H - g.cs : 0), left = j == 4 ? g.cleft : ((j & 1) ? g.W - g.cs : 0);
  return {x + (((long long)f * g.H + top + yo) * g.W) * g.C + c, f, crop, c, left};
}

// ---- normaliser policies: by-value kernel arguments.  row(): what one output row needs, looked up once per wave-row (every
// quantity in it is wave-uniform); apply(): one pixel.  Separately rounded operations throughout: a true division (no reciprocal
// multiply), and q * r + lo as a multiply and an add.  hipcc contracts that pair into one FMA by default (and its __fmul_rn /
// __fadd_rn are the plain operators, contracted alike), which changes about a fifth of the outputs at (lo, hi) = (0.1, 0.7):
// contraction is switched off in apply, and the instructions keep that when it is inlined.

struct RowNorm {
  float sub, div, r, lo;
};

__device__ __forceinline__ float standardize(const RowNorm& n, uint8_t px) {
#pragma clang fp contract(off)
  return ((float)px - n.sub) / n.div;
}

// (x - mean) / std with one scalar pair: the reference's own normalisation; any C
struct ScalarPair {
  float mean, stdv;
  __device__ __forceinline__ RowNorm row(const CropRow&, int) const { return {mean, stdv, 0.f, 0.f}; }
  static __device__ __forceinline__ float apply(const RowNorm& n, uint8_t px) { return standardize(n, px); }
};

// Per-channel constants as the kernels take them: (mean, std) or (lo, r) of up to three channels
struct NormConsts {
  float a[3], b[3];
};

// (x - mean[c]) / std[c]
struct PerChannel {
  NormConsts k;
  __device__ __forceinline__ RowNorm row(const CropRow& w, int) const { return {k.a[w.c], k.b[w.c], 0.f, 0.f}; }
  static __device__ __forceinline__ float apply(const RowNorm& n, uint8_t px) { return standardize(n, px); }
};

// (x - mn) / (mx - mn) * r[c] + lo[c] with (mn, mx) from the statistics table, of channel c (ADVHIP_NORM_CHANNEL_MINMAX) or over
// all channels (ADVHIP_NORM_PIXEL_MINMAX)
struct MinMax {
  NormConsts k;
  int mode, spitch;
  const uint8_t* __restrict__ stats;
  __device__ __forceinline__ RowNorm row(const CropRow& w, int C) const {
    const uint8_t* s = stats + ((long long)(w.f / spitch) * 6 + crop_window(w.crop)) * C * 2;
    int mn = s[2 * w.c], mx = s[2 * w.c + 1];
    if (mode == ADVHIP_NORM_PIXEL_MINMAX)
      for (int cc = 0; cc < C; ++cc) {
        mn = min(mn, (int)s[2 * cc]);
        mx = max(mx, (int)s[2 * cc + 1]);
      }
    // (the range is exact; 0 for a constant crop / channel: 0 / 0 = NaN, as the reference gives)
    return {(float)mn, (float)mx - (float)mn, k.b[w.c], k.a[w.c]};
  }
  static __device__ __forceinline__ float apply(const RowNorm& n, uint8_t px) {
#pragma clang fp contract(off)
    const float m = standardize(n, px) * n.r;
    return m + n.lo;
  }
};

// ---- the two writers ----

// Dense rows y[(clip-crop, c, t, y)][x]: 16-byte stores (VW = 4: cs % 4 == 0 and y 16-byte aligned) or scalar ones.
template <int VW, class Norm>
__global__ __launch_bounds__(256) void tencrop_dense_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, TenCrop g, long long rows,
                                                            Norm norm) {
  const int lane = threadIdx.x & 63;
  const int csv = g.cs / VW;
  for (long long r0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r0 < rows; r0 += (long long)gridDim.x * 4) {
    const CropRow row = crop_row(x, g, r0, 0);
    const RowNorm n = norm.row(row, g.C);
    float* out = y + r0 * g.cs;
    for (int q = lane; q < csv; q += 64) {
      float v[VW];
#pragma unroll
      for (int e = 0; e < VW; ++e) v[e] = Norm::apply(n, row.at(g, q * VW + e));
      if constexpr (VW == 4) reinterpret_cast<float4*>(out)[q] = make_float4(v[0], v[1], v[2], v[3]);
      else out[q] = v[0];
    }
  }
}

// COLUMN-PARITY PLANES (the operand of the stem's 16-byte gather, advhip_conv3d_s2w_*): crop-clips [first, first + count),
// xs[(clip-crop, c, t, y)][par][2 + j] = normalised pixel of crop column 2 j + par, zero in the padding columns.  One wave per
// (row, both planes); the arithmetic per pixel is the dense writer's, so the values are its values.
template <class Norm>
__global__ __launch_bounds__(256) void tencrop_planes_kernel(const uint8_t* __restrict__ x, float* __restrict__ xs, TenCrop g, long long first,
                                                             long long rows, int WP, Norm norm) {
  const int lane = threadIdx.x & 63;
  for (long long r0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); r0 < rows; r0 += (long long)gridDim.x * 4) {
    const CropRow row = crop_row(x, g, r0, first);
    const RowNorm n = norm.row(row, g.C);
    float* out = xs + r0 * 2 * WP;
    for (int q = lane; q < 2 * WP; q += 64) {
      const int par = q >= WP, idx = q - par * WP, xo = 2 * (idx - 2) + par;
      float v = 0.f;
      if (idx >= 2 && xo < g.cs) v = Norm::apply(n, row.at(g, xo));
      out[q] = v;
    }
  }
}

// ---- host ----

// The normalisation as an entry point states it: the scalar pair (a == nullptr) or a mode with host triples of doubles `a`, `b`
// -- (mean, std) or (lo, hi) per channel -- and, for the min-max modes, the statistics table.
struct NormSpec {
  float mean, stdv;
  int mode;
  const double *a, *b;
  const uint8_t* stats;
  int stats_pitch;
  bool modes;
};

// The checks of a mode beyond the sampling's own, and the constants the kernels take, rounded as the reference rounds them: pixel
// mode r = float(hi - lo) with the subtraction in double, channel mode r = float(hi) - float(lo).
static int norm_consts(const char* who, const NormSpec& n, int C, const ClipSampling& s, NormConsts* k) {
  const int mode = n.mode;
  const double *a = n.a, *b = n.b;
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
  ADVHIP_REQUIRE(n.stats, "%s: the min-max modes need the statistics table", who);
  ADVHIP_REQUIRE(n.stats_pitch >= 1, "%s: stats pitch %d", who, n.stats_pitch);
  ADVHIP_REQUIRE(s.clip_stride % n.stats_pitch == 0 && s.frame_step % n.stats_pitch == 0,
                 "%s: stats pitch %d does not divide clip stride %d and frame step %d", who, n.stats_pitch, s.clip_stride, s.frame_step);
  return ADVHIP_OK;
}

// Every TenCrop entry point: the checks, the launch shape (block 256 = four rows, grid capped at 256 x 256) and the launch.
// `range` = {first crop-clip, count}: the planes writer over those crop-clips; null: the dense writer over the whole video.
static int tencrop_launch(const char* who, const uint8_t* frames, float* out, int F, int H, int W, int C, const ClipSampling& s, int crop,
                          const int64_t* range, const NormSpec& n, void* stream) {
  if (int rc = s.check_crops(who)) return rc;
  ADVHIP_REQUIRE(frames && out, "%s: null pointer", who);
  ADVHIP_REQUIRE(F > 0 && C > 0 && s.fpc > 0 && crop > 0 && (!range || crop % 2 == 0), "%s: bad arguments", who);
  if (int rc = s.check_windows(who, 1ll << 31)) return rc;
  ADVHIP_REQUIRE(H >= crop && W >= crop, "%s: frames (%d x %d) smaller than the %d crop", who, H, W, crop);
  NormConsts k;
  if (n.modes) {
    if (int rc = norm_consts(who, n, C, s, &k)) return rc;
  } else {
    ADVHIP_REQUIRE(n.stdv != 0.f, "%s: std must be non-zero", who);
  }
  const long long crop_clips = s.video_windows(F) * s.ncrops;
  const long long first = range ? range[0] : 0, count = range ? range[1] : crop_clips;
  ADVHIP_REQUIRE(first >= 0 && count > 0 && first + count <= crop_clips, "%s: crop-clips [%lld, %lld) outside the video's %lld", who, first,
                 first + count, crop_clips);
  const TenCrop g{F, H, W, C, s.fpc, s.clip_stride, s.frame_step, crop, half_even(H - crop), half_even(W - crop), s.ncrops, s.crops};
  const long long rows = count * C * s.fpc * crop;
  const dim3 grid((unsigned)std::min<long long>((rows + 3) / 4, 256 * 256)), block(256);
  const bool vec = crop % 4 == 0 && ((uintptr_t)out & 15) == 0;
  auto launch = [&](auto norm) {
    using Norm = decltype(norm);
    if (range) hipLaunchKernelGGL(tencrop_planes_kernel<Norm>, grid, block, 0, (hipStream_t)stream, frames, out, g, first, rows, crop / 2 + 4, norm);
    else if (vec) hipLaunchKernelGGL((tencrop_dense_kernel<4, Norm>), grid, block, 0, (hipStream_t)stream, frames, out, g, rows, norm);
    else hipLaunchKernelGGL((tencrop_dense_kernel<1, Norm>), grid, block, 0, (hipStream_t)stream, frames, out, g, rows, norm);
  };
  if (!n.modes) launch(ScalarPair{n.mean, n.stdv});
  else if (n.mode == ADVHIP_NORM_STANDARDIZE) launch(PerChannel{k});
  else launch(MinMax{k, n.mode, n.stats_pitch, n.stats});
  return check_launch(who);
}

static NormSpec scalar_pair(float mean, float stdv) { return {mean, stdv, 0, nullptr, nullptr, nullptr, 0, false}; }

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

// ---- the ten TenCrop names: dense and planes, each plain / _strided / _crops / _sampled (the scalar pair; the shorter names fill
// in the sampling arguments they lack: back-to-back clips, all ten crops, every frame) and _modes ----

extern "C" int advhip_tencrop_normalize_u8(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                           int32_t frames_per_clip, int32_t crop, float mean, float stdv, void* stream) {
  return tencrop_launch("tencrop_normalize_u8", frames, y, F, H, W, C, {frames_per_clip, frames_per_clip, 1, 10, TENCROP_ALL}, crop, nullptr,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_u8_strided(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                                   int32_t frames_per_clip, int32_t clip_stride, int32_t crop, float mean, float stdv,
                                                   void* stream) {
  return tencrop_launch("tencrop_normalize_u8", frames, y, F, H, W, C, {frames_per_clip, clip_stride, 1, 10, TENCROP_ALL}, crop, nullptr,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_u8_crops(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                                 int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int32_t ncrops,
                                                 uint64_t crops_packed, float mean, float stdv, void* stream) {
  return tencrop_launch("tencrop_normalize_u8", frames, y, F, H, W, C, {frames_per_clip, clip_stride, 1, ncrops, crops_packed}, crop, nullptr,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_u8_sampled(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                                   int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                   int32_t ncrops, uint64_t crops_packed, float mean, float stdv, void* stream) {
  return tencrop_launch("tencrop_normalize_u8", frames, y, F, H, W, C, {frames_per_clip, clip_stride, frame_step, ncrops, crops_packed}, crop, nullptr,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_u8_modes(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                                 int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                 int32_t ncrops, uint64_t crops_packed, int32_t mode, const double* a, const double* b,
                                                 const uint8_t* stats, int32_t stats_pitch, void* stream) {
  return tencrop_launch("tencrop_normalize_u8_modes", frames, y, F, H, W, C, {frames_per_clip, clip_stride, frame_step, ncrops, crops_packed}, crop,
                        nullptr, {0.f, 0.f, mode, a, b, stats, stats_pitch, true}, stream);
}

extern "C" int advhip_tencrop_normalize_planes_u8(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                  int32_t frames_per_clip, int32_t crop, int64_t first_crop_clip, int64_t count, float mean,
                                                  float stdv, void* stream) {
  const int64_t range[2] = {first_crop_clip, count};
  return tencrop_launch("tencrop_normalize_planes_u8", frames, xs, F, H, W, C, {frames_per_clip, frames_per_clip, 1, 10, TENCROP_ALL}, crop, range,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_planes_u8_strided(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                          int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int64_t first_crop_clip,
                                                          int64_t count, float mean, float stdv, void* stream) {
  const int64_t range[2] = {first_crop_clip, count};
  return tencrop_launch("tencrop_normalize_planes_u8", frames, xs, F, H, W, C, {frames_per_clip, clip_stride, 1, 10, TENCROP_ALL}, crop, range,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_planes_u8_crops(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                        int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int32_t ncrops,
                                                        uint64_t crops_packed, int64_t first_crop_clip, int64_t count, float mean,
                                                        float stdv, void* stream) {
  const int64_t range[2] = {first_crop_clip, count};
  return tencrop_launch("tencrop_normalize_planes_u8", frames, xs, F, H, W, C, {frames_per_clip, clip_stride, 1, ncrops, crops_packed}, crop, range,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_planes_u8_sampled(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                          int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                          int32_t ncrops, uint64_t crops_packed, int64_t first_crop_clip, int64_t count,
                                                          float mean, float stdv, void* stream) {
  const int64_t range[2] = {first_crop_clip, count};
  return tencrop_launch("tencrop_normalize_planes_u8", frames, xs, F, H, W, C, {frames_per_clip, clip_stride, frame_step, ncrops, crops_packed}, crop, range,
                        scalar_pair(mean, stdv), stream);
}

extern "C" int advhip_tencrop_normalize_planes_u8_modes(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                                        int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                                        int32_t ncrops, uint64_t crops_packed, int64_t first_crop_clip, int64_t count,
                                                        int32_t mode, const double* a, const double* b, const uint8_t* stats,
                                                        int32_t stats_pitch, void* stream) {
  const int64_t range[2] = {first_crop_clip, count};
  return tencrop_launch("tencrop_normalize_planes_u8_modes", frames, xs, F, H, W, C, {frames_per_clip, clip_stride, frame_step, ncrops, crops_packed}, crop,
                        range, {0.f, 0.f, mode, a, b, stats, stats_pitch, true}, stream);
}
