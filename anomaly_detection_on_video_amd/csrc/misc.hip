// On-device analogues of the numpy post-processing either side of the hot path.
//   segment_features     : extract_features.py:171-183
//   add_magnitude        : src/dataset.py:121-124
//   normalize_permute_u8 : src/dataset.py:175-183 on already cropped uint8 clips
//   frame_scores         : src/runner.py:66-76
// (The TenCrop passes from uint8 frames are normalize.hip's.)
#include <algorithm>

#include "common.h"

namespace advhip {

// np.linspace(0, n, seg+1, dtype=int): float64 i*step truncated; last element is exactly n.
__device__ __forceinline__ int linspace_int(int i, int n, int seg) {
  if (i >= seg) return n;
  const double step = (double)n / (double)seg;
  return (int)((double)i * step);
}

// one thread per output element (crop, s, c); rows of a bucket are added in order in fp32 and
// divided by the count, as np.mean over axis 0 of a float32 array does
__global__ void segment_kernel(const float* __restrict__ f, float* __restrict__ out, int n, int ncrops, int C, int seg) {
  const long long total = (long long)ncrops * seg * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int s = (int)((i / C) % seg);
    const int crop = (int)(i / ((long long)C * seg));
    const int r0 = linspace_int(s, n, seg), r1 = linspace_int(s + 1, n, seg);
    float v;
    if (r0 != r1) {
      float acc = 0.f;
      for (int r = r0; r < r1; ++r) acc += f[((size_t)r * ncrops + crop) * C + c];
      v = acc / (float)(r1 - r0);
    } else {
      v = f[((size_t)r0 * ncrops + crop) * C + c];
    }
    out[i] = v;
  }
}

// one wavefront per row: copy C floats and append the L2 norm
__global__ void add_magnitude_kernel(const float* __restrict__ f, float* __restrict__ out, long long rows, int C) {
  const int lane = threadIdx.x & 63;
  const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = f + row * C;
  float* q = out + row * (C + 1);
  float s = 0.f;
  for (int i = lane; i < C; i += 64) {
    const float v = p[i];
    q[i] = v;
    s += v * v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) q[C] = sqrtf(s);
}

// uint8 frames (N, T, C, H, W) -> fp32 (N, C, T, H, W), y = (x - mean) / std: the reference's
// PILToTensor().float() + GroupNormalize + the (B,10,16,3,H,W)->(B,10,3,16,H,W) permute
// (src/dataset.py:175-183, extract_features.py:83) in one pass, so only uint8 crosses
// PCIe.  Each thread converts 4 consecutive pixels of a row (one 32-bit load, one 16-byte store).
__global__ void normalize_permute_u8_kernel(const uint8_t* __restrict__ x, float* __restrict__ y, int T, int C,
                                            long long HW, float mean, float stdv, long long total4) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total4;
       i += (long long)gridDim.x * blockDim.x) {
    const long long hw4 = HW / 4;
    const long long p4 = i % hw4;            // output order: (n, c, t, hw)
    long long r = i / hw4;
    const int t = (int)(r % T);
    r /= T;
    const int c = (int)(r % C);
    const long long n = r / C;
    const uint32_t v = *reinterpret_cast<const uint32_t*>(x + (((n * T + t) * C + c) * HW + p4 * 4));
    float4 o;
    o.x = ((float)(v & 0xff) - mean) / stdv;
    o.y = ((float)((v >> 8) & 0xff) - mean) / stdv;
    o.z = ((float)((v >> 16) & 0xff) - mean) / stdv;
    o.w = ((float)(v >> 24) - mean) / stdv;
    reinterpret_cast<float4*>(y)[i] = o;
  }
}

// Per-window scores (n,) -> per-frame scores: window w covers frames [w * cstride, w * cstride + fpc); the score of a frame is
// the mean of the scores of the windows covering it, added in ascending window order, one division by their count (cstride =
// fpc: one window per frame, np.repeat(scores, fpc) of runner.py:66-76).  One thread per frame, at most ceil(fpc / cstride) adds.
__global__ __launch_bounds__(256) void frame_scores_kernel(const float* __restrict__ scores, float* __restrict__ out, int n, int fpc, int cstride,
                                                           int n_frames) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_frames) return;
  const int lo = f < fpc ? 0 : (f - fpc) / cstride + 1;  // first w with w * cstride + fpc > f
  const int hi = min(n - 1, f / cstride);                // last w with w * cstride <= f
  float acc = scores[lo];
  for (int w = lo + 1; w <= hi; ++w) acc += scores[w];
  out[f] = acc / (float)(hi - lo + 1);
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_frame_scores_f32(const float* scores, float* out, int64_t n_windows, int32_t frames_per_clip, int32_t clip_stride,
                                       int64_t n_frames, void* stream) {
  ADVHIP_REQUIRE(scores && out && n_windows > 0 && frames_per_clip > 0, "frame_scores: bad arguments");
  ADVHIP_REQUIRE(clip_stride >= 1 && clip_stride <= frames_per_clip, "frame_scores: clip stride %d outside [1, %d]", clip_stride, frames_per_clip);
  const long long covered = (long long)(n_windows - 1) * clip_stride + frames_per_clip;
  ADVHIP_REQUIRE(n_frames > 0 && n_frames <= covered, "frame_scores: %lld frames, but %lld windows of %d at stride %d cover %lld",
                 (long long)n_frames, (long long)n_windows, frames_per_clip, clip_stride, covered);
  ADVHIP_REQUIRE(covered < (1ll << 31), "frame_scores: more than 2^31 frames");
  const unsigned grid = (unsigned)((n_frames + 255) / 256);
  hipLaunchKernelGGL(frame_scores_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, scores, out, (int)n_windows, frames_per_clip, clip_stride,
                     (int)n_frames);
  return check_launch("frame_scores");
}

extern "C" int advhip_normalize_permute_u8(const uint8_t* x, float* y, int64_t N, int32_t T, int32_t C, int32_t H,
                                           int32_t W, float mean, float stdv, void* stream) {
  ADVHIP_REQUIRE(x && y && N > 0 && T > 0 && C > 0 && H > 0 && W > 0, "normalize_permute_u8: bad arguments");
  ADVHIP_REQUIRE(((long long)H * W) % 4 == 0, "normalize_permute_u8: H*W=%lld must be a multiple of 4", (long long)H * W);
  ADVHIP_REQUIRE(stdv != 0.f, "normalize_permute_u8: std must be non-zero");
  const long long total4 = (long long)N * T * C * H * W / 4;
  const int grid = (int)std::min<long long>((total4 + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(normalize_permute_u8_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, y, T, C,
                     (long long)H * W, mean, stdv, total4);
  return check_launch("normalize_permute_u8");
}

extern "C" int advhip_segment_features_f32(const float* feats, float* out, int32_t n_clips, int32_t ncrops, int32_t C,
                                           int32_t seg, void* stream) {
  ADVHIP_REQUIRE(feats && out && n_clips > 0 && ncrops > 0 && C > 0 && seg > 0, "segment_features: bad arguments");
  const long long total = (long long)ncrops * seg * C;
  const int grid = (int)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(segment_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, feats, out, n_clips, ncrops, C, seg);
  return check_launch("segment_features");
}

extern "C" int advhip_add_magnitude_f32(const float* feats, float* out, int64_t rows, int32_t C, void* stream) {
  ADVHIP_REQUIRE(feats && out && rows > 0 && C > 0, "add_magnitude: bad arguments");
  const long long grid = (rows + 3) / 4;
  ADVHIP_REQUIRE(grid < (1ll << 31), "add_magnitude: too many rows");
  hipLaunchKernelGGL(add_magnitude_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, feats, out,
                     (long long)rows, C);
  return check_launch("add_magnitude");
}
