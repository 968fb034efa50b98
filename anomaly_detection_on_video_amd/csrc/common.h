// Shared helpers for the gfx950 kernels behind include/advhip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/advhip.h"

#define ADVHIP_REQUIRE(cond, ...)        \
  do {                                   \
    if (!(cond)) {                       \
      advhip::set_error(__VA_ARGS__);    \
      return ADVHIP_EINVAL;              \
    }                                    \
  } while (0)

namespace advhip {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return ADVHIP_ELAUNCH;
  }
  return ADVHIP_OK;
}

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// MI355X: 8 XCDs, blocks are dealt round-robin over them.  Map the hardware block id to a
// logical tile id so that each XCD works on a contiguous range of logical tiles (neighbouring
// tiles share operand panels -> same L2).  Bijective for any grid size.  Speed only.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  constexpr int NX = 8;
  const int q = nwg >> 3, r = nwg & 7;  // unsigned-style shifts: no signed-division fix-ups
  const int xcd = bid & 7, k = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + k;
}

using f32x4 = __attribute__((ext_vector_type(4))) float;

// The backbone's ReLU and window maxima: NaN in, NaN out, as torch.relu / clamp_min / max_pool3d (fmaxf returns the operand that
// is NOT a NaN, which would turn a NaN clip into finite features).  IEEE 754-2019 maximum = one v_maximum3_f32 on gfx950, the
// instruction count of fmaxf; without a NaN operand the result is fmaxf's bit for bit (max(-0, +0) = +0 in both).
__device__ __forceinline__ float max_nan(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float relu_nan(float v) { return max_nan(v, 0.f); }

// A crop subset of TenCrop as the kernels take it: `ncrops` 4-bit indices, entry j in bits [4 j, 4 j + 4) (row clip * ncrops + j
// holds crop entry j).  All ten in order = the identity set.
constexpr unsigned long long TENCROP_ALL = 0x9876543210ull;

// null = well formed: 1 <= ncrops <= 10, every index < 10, strictly ascending (TenCrop's own order), unused nibbles zero
inline const char* crops_packed_error(int ncrops, unsigned long long packed) {
  if (ncrops < 1 || ncrops > 10) return "ncrops outside [1, 10]";
  int prev = -1;
  for (int j = 0; j < ncrops; ++j) {
    const int c = (int)((packed >> (4 * j)) & 15);
    if (c > 9) return "crop index above 9";
    if (c <= prev) return "crop indices not strictly ascending";
    prev = c;
  }
  if (packed >> (4 * ncrops)) return "bits set above the last crop index";
  return nullptr;
}

// The clip-sampling rule of the uint8-frame ops, host side.  Window w of a video samples frames w * clip_stride + t * frame_step,
// t in [0, fpc); row w * ncrops + j of an op's output holds crop (crops >> 4 j) & 15 of window w.  The device restates the frame
// index once for the TenCrop passes (normalize.hip: crop_row) and in the stems' gather tables; every count and every check of the
// five numbers is here.
struct ClipSampling {
  int fpc, clip_stride, frame_step, ncrops;
  unsigned long long crops;

  int check_crops(const char* who) const {
    const char* why = crops_packed_error(ncrops, crops);
    ADVHIP_REQUIRE(!why, "%s: crop set (%d, 0x%llx): %s", who, ncrops, crops, why);
    return ADVHIP_OK;
  }
  // `span_limit`: the op's own bound on fpc * frame_step (what its kernel's index arithmetic holds)
  int check_windows(const char* who, long long span_limit) const {
    ADVHIP_REQUIRE(frame_step >= 1 && (long long)fpc * frame_step < span_limit, "%s: frame step %d", who, frame_step);
    ADVHIP_REQUIRE(clip_stride >= 1 && clip_stride <= fpc * frame_step, "%s: clip stride %d outside [1, %d]", who, clip_stride,
                   fpc * frame_step);
    return ADVHIP_OK;
  }
  // windows of a video of F frames; the last one may be short (LoopPad repeats it)
  long long video_windows(long long F) const {
    const long long span = (long long)fpc * frame_step;
    return 1 + (F > span ? (F - span + clip_stride - 1) / clip_stride : 0);
  }
  // windows of a buffer that holds whole windows only: F = (n - 1) * clip_stride + (fpc - 1) * frame_step + 1 for n >= 1
  // (frame_step = 1, clip_stride = fpc: whole back-to-back clips); any other F is refused
  int buffer_windows(const char* who, long long F, long long* n) const {
    const long long reach = (long long)(fpc - 1) * frame_step + 1;  // frames from a window's first sampled frame to its last
    const bool whole = F >= reach && (F - reach) % clip_stride == 0;
    ADVHIP_REQUIRE(frame_step > 1 || whole, "%s: %lld frames are not whole clips of %d at stride %d", who, F, fpc, clip_stride);
    ADVHIP_REQUIRE(whole, "%s: %lld frames are not whole clips of %d, one frame in %d, at stride %d", who, F, fpc, frame_step, clip_stride);
    *n = (F - reach) / clip_stride + 1;
    return ADVHIP_OK;
  }
};

// torchvision center_crop's offset: int(round(d / 2.0)) with Python's round-half-to-even
inline int half_even(int d) { return (d % 2 == 0) ? d / 2 : ((d / 2) % 2 == 0 ? d / 2 : d / 2 + 1); }

}  // namespace advhip
