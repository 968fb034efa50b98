// numpy's pairwise sum of a row's squares, as one wavefront computes it: the rule of advhip_add_magnitude_np_f32
// (include/advhip.h states it), shared by the kernels that append the magnitude channel (magnitude_np.hip, live.hip).
// np.linalg.norm(x, axis=2) of a float32 array is sqrt(add.reduce(x * x)), and add.reduce over a contiguous axis is numpy's
// pairwise sum -- blocks of at most 128 elements, eight accumulators per block, the blocks combined by a fixed tree of adds.
#pragma once
#include <mutex>
#include <vector>

#include "common.h"

namespace advhip {

constexpr int PW_MAX_C = 8192;    // numpy reduces in chunks of 8192 elements: above that the order of its sum changes
constexpr int PW_BLOCK = 128;     // numpy's PW_BLOCKSIZE
constexpr int PW_MAX_LEAVES = 128;  // a split block's halves hold >= 64 elements each: at most C / 64 leaves

// The leaves of the split recursion in order: start | len << 14 | adds << 22.  `adds`: how many pending partial sums are added
// once this leaf's sum is known -- the post-order walk of the tree of `+`, run with a stack.
struct PwLeaves {
  uint32_t e[PW_MAX_LEAVES];
  int32_t n;
};

inline void pw_split(int start, int n, PwLeaves& t) {
  if (n <= PW_BLOCK) {
    t.e[t.n++] = (uint32_t)start | (uint32_t)n << 14;
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  pw_split(start, n2, t);
  pw_split(start + n2, n - n2, t);
  t.e[t.n - 1] += 1u << 22;
}

// built once per C (pure integer arithmetic), kept for the life of the library
inline const PwLeaves& pw_leaves(int C) {
  static std::mutex mu;
  static std::vector<PwLeaves*> cache(PW_MAX_C + 1, nullptr);
  std::lock_guard<std::mutex> lock(mu);
  if (!cache[C]) {
    PwLeaves* t = new PwLeaves();
    t->n = 0;
    pw_split(0, C, *t);
    cache[C] = t;
  }
  return *cache[C];
}

// LDS index of square i: 8 floats of padding per 128, so that chain j of eight consecutive full leaves lands on eight
// different groups of 8 banks (64 four-byte banks; at pitch 128 all eight would share one group)
__device__ __forceinline__ int pw_pad(int i) { return i + ((i >> 7) << 3); }

__host__ __device__ inline int pw_sq_floats(int C) { return C + ((C >> 7) << 3) + 8; }

// dynamic LDS of a workgroup that calls pw_row_magnitude on rows of C
inline size_t pw_lds_bytes(int C, const PwLeaves& tab) { return sizeof(float) * (size_t)(pw_sq_floats(C) + 9 * tab.n + 16); }

// One row by one wavefront that is its whole workgroup (64 threads; every lane calls): q[0..C) = p[0..C) bit for bit, q[C] = the
// magnitude.  Pass 1: coalesced dword loads of the row, coalesced dword stores of the copy (an output row pitch of C + 1 is only
// 4-byte aligned), squares parked in LDS.  Pass 2: the leaves' eight accumulator chains, one chain per lane (C = 2048: 16 leaves
// x 8 = 128 chains, two per lane).  Pass 3: one lane per leaf closes its block -- the fixed tree over the eight accumulators,
// then the n % 8 tail in order.  Pass 4: lane 0 walks the tree of `+` over the leaf sums.  Every multiply and add is its own fp32
// operation: no contraction.  `lds`: pw_lds_bytes(C, tab) of the workgroup's; free again on return.
__device__ __forceinline__ void pw_row_magnitude(const float* __restrict__ p, float* __restrict__ q, int C, const PwLeaves& tab, float* lds) {
#pragma clang fp contract(off)
  const int n = tab.n;
  float* sq = lds;
  float* chain = sq + pw_sq_floats(C);  // (n, 8)
  float* leafsum = chain + 8 * n;       // (n)
  float* stack = leafsum + n;           // (16): the tree is at most 8 deep
  const int lane = threadIdx.x;
  for (int i = lane; i < C; i += 64) {
    const float v = p[i];
    q[i] = v;
    sq[pw_pad(i)] = v * v;
  }
  __syncthreads();
  if (C < 8) {
    if (lane == 0) {
      float s = 0.f;
      for (int i = 0; i < C; ++i) s += sq[i];
      q[C] = sqrtf(0.f + s);
    }
  } else {
    for (int c = lane; c < 8 * n; c += 64) {
      const uint32_t e = tab.e[c >> 3];
      const int start = (int)(e & 0x3fff) + (c & 7), len = (int)(e >> 14) & 0xff;
      float r = sq[pw_pad(start)];
      for (int i = 8; i < len - (len & 7); i += 8) r += sq[pw_pad(start + i)];
      chain[c] = r;
    }
    __syncthreads();
    for (int l = lane; l < n; l += 64) {
      const uint32_t e = tab.e[l];
      const int start = (int)(e & 0x3fff), len = (int)(e >> 14) & 0xff;
      const float* r = chain + 8 * l;
      float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (int i = len - (len & 7); i < len; ++i) res += sq[pw_pad(start + i)];
      leafsum[l] = res;
    }
    __syncthreads();
    if (lane == 0) {
      int sp = 0;
      for (int l = 0; l < n; ++l) {
        float v = leafsum[l];
        for (int k = (int)(tab.e[l] >> 22); k > 0; --k) v = stack[--sp] + v;
        stack[sp++] = v;
      }
      q[C] = sqrtf(0.f + stack[0]);
    }
  }
  __syncthreads();  // the next row overwrites the squares
}

}  // namespace advhip
