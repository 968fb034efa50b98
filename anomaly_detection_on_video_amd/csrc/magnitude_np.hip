// FeatureDataset.add_magnitude (the reference's src/dataset.py:121-124) with numpy's own bits in the appended channel:
// np.linalg.norm(x, axis=2) of a float32 array is sqrt(add.reduce(x * x)), and add.reduce over a contiguous axis is numpy's
// pairwise sum -- blocks of at most 128 elements, eight accumulators per block, the blocks combined by a fixed tree of adds
// (include/advhip.h states the rule).  add_magnitude_kernel (misc.hip) sums lane-strided and agrees to 1e-6 only; a dataset
// held on the device must hand the trainer exactly what the host loader hands it, so this pass restates numpy's order.
#include <algorithm>

#include "pw_sum.h"

namespace advhip {

// One wavefront (= one workgroup) per row: pw_row_magnitude (pw_sum.h) copies the row and appends its magnitude.
__global__ __launch_bounds__(64) void add_magnitude_np_kernel(const float* __restrict__ f, float* __restrict__ out, long long a, int b, int C,
                                                              int transpose, PwLeaves tab) {
  extern __shared__ float pw_lds[];
  const long long rows = a * b;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const long long orow = transpose ? (row % b) * a + row / b : row;
    pw_row_magnitude(f + row * C, out + orow * (C + 1), C, tab, pw_lds);
  }
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_add_magnitude_np_leaves(int32_t C, int32_t* leaves, int32_t* n_leaves) {
  ADVHIP_REQUIRE(leaves && n_leaves, "add_magnitude_np_leaves: null pointer");
  ADVHIP_REQUIRE(C >= 1 && C <= PW_MAX_C, "add_magnitude_np_leaves: C=%d outside [1, %d]", C, PW_MAX_C);
  const PwLeaves& t = pw_leaves(C);
  for (int i = 0; i < t.n; ++i) {
    leaves[3 * i] = (int32_t)(t.e[i] & 0x3fff);
    leaves[3 * i + 1] = (int32_t)((t.e[i] >> 14) & 0xff);
    leaves[3 * i + 2] = (int32_t)(t.e[i] >> 22);
  }
  *n_leaves = t.n;
  return ADVHIP_OK;
}

extern "C" int advhip_add_magnitude_np_f32(const float* feats, float* out, int64_t a, int32_t b, int32_t C, int32_t transpose,
                                           void* stream) {
  ADVHIP_REQUIRE(feats && out, "add_magnitude_np: null pointer");
  ADVHIP_REQUIRE(a > 0 && b > 0 && C > 0 && (transpose == 0 || transpose == 1), "add_magnitude_np: bad arguments");
  ADVHIP_REQUIRE(C <= PW_MAX_C,
                 "add_magnitude_np: C=%d above %d: numpy sums in chunks of %d elements, the order of its adds changes there", C, PW_MAX_C,
                 PW_MAX_C);
  ADVHIP_REQUIRE(a <= (1ll << 40) / b, "add_magnitude_np: more than 2^40 rows");
  const PwLeaves& tab = pw_leaves(C);
  const long long rows = (long long)a * b;
  const unsigned grid = (unsigned)std::min<long long>(rows, 1ll << 20);
  const size_t lds = pw_lds_bytes(C, tab);
  hipLaunchKernelGGL(add_magnitude_np_kernel, dim3(grid), dim3(64), lds, (hipStream_t)stream, feats, out, (long long)a, (int)b, (int)C,
                     (int)transpose, tab);
  return check_launch("add_magnitude_np");
}
