// float4 values as the scorer's kernels use them (a lane's four consecutive positions), and the wave / block sums they share.
// Every helper takes and returns float4 by value and spells the four components ONCE, as scalar fp32 expressions: the compiler
// then sees what the hand-written .x / .y / .z / .w lines gave it and pairs the lanes into packed instructions by itself.  HIP's
// own float4 operators and ext_vector_type(4) cost 8-10 % more instructions in the register-resident LayerNorm forward
// (profiles/scorer_cores_codegen.md).
#pragma once
#include "common.h"

namespace advhip {

// f applied to the x, y, z and w components of its arguments: q4_map(f, a, b) = (f(a.x, b.x), ..., f(a.w, b.w)).  A kernel's
// per-component formula is a scalar lambda; values that are the same for all four components are captured.
template <class F, class... A>
__device__ __forceinline__ float4 q4_map(F f, A... a) {
  return make_float4(f(a.x...), f(a.y...), f(a.z...), f(a.w...));
}

__device__ __forceinline__ float4 q4_splat(float s) { return make_float4(s, s, s, s); }
__device__ __forceinline__ float4 q4_add(float4 a, float4 b) { return q4_map([](float x, float y) { return x + y; }, a, b); }
__device__ __forceinline__ float4 q4_sub(float4 a, float4 b) { return q4_map([](float x, float y) { return x - y; }, a, b); }
__device__ __forceinline__ float4 q4_mul(float4 a, float4 b) { return q4_map([](float x, float y) { return x * y; }, a, b); }
__device__ __forceinline__ float4 q4_scale(float4 a, float s) { return q4_map([s](float x) { return x * s; }, a); }
// acc + a * b
__device__ __forceinline__ float4 q4_madd(float4 acc, float4 a, float4 b) {
  return q4_map([](float c, float x, float y) { return c + x * y; }, acc, a, b);
}

// acc[0 .. 4) += a * v, for accumulators kept as scalars
__device__ __forceinline__ void q4_axpy(float* acc, float a, float4 v) {
  acc[0] += a * v.x;
  acc[1] += a * v.y;
  acc[2] += a * v.z;
  acc[3] += a * v.w;
}

// 16-byte accesses: p is 16-byte aligned
__device__ __forceinline__ float4 q4_load(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void q4_store(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// v + (v of the lane `off` away), all four components
__device__ __forceinline__ float4 q4_shfl_xor_add(float4 v, int off) {
  return q4_map([off](float x) { return x + __shfl_xor(x, off, 64); }, v);
}

// The two orders in which the kernels add a float4's components.  Both are in use and neither may turn into the other: the
// order is part of every result's bits.
__device__ __forceinline__ float q4_sum_seq(float4 v) { return ((v.x + v.y) + v.z) + v.w; }     // LayerNorm / head per-channel sums
__device__ __forceinline__ float q4_sum_pairs(float4 v) { return (v.x + v.y) + (v.z + v.w); }   // bn_rows_*_reg_kernel

// NV running sums, each added up over WIDTH consecutive lanes (a power of two <= 64) by an xor butterfly in fixed order: every
// lane of the group ends with the group's sums
template <int WIDTH, int NV>
__device__ __forceinline__ void lane_group_sums(float (&v)[NV]) {
#pragma unroll
  for (int off = WIDTH / 2; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += __shfl_xor(v[i], off, 64);
}

// v added up over the NT threads of the block (waves by butterfly, then in wave order through red[NT / 64]); every thread gets
// the sum.  The wave sums are added from red[0] on, not from 0.f: 0.f + (-0.f) would turn a mean of -0 into +0.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();  // red may still be read from a previous call
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; ++i) t += red[i];
  return t;
}

}  // namespace advhip
