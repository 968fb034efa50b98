// Multi-block scans shared by roc.hip and events.hip.  One workgroup scans SCAN_TILE elements, four contiguous ones per thread,
// the 256 thread sums through LDS.  No workgroup waits on another one: a scan over more than one tile is reduce / scan the
// partials (recursively) / apply, as separate launches on the caller's stream.
//
// The element type T brings its own `operator+` (any associative operation: a sum, a maximum) and `zero_of((const T*)nullptr)`,
// its identity; both are looked up where the scan is instantiated.  An IO type reads element i (`load`) and receives the
// exclusive and the inclusive result for it (`store`), so a pass can compute its input on the fly and write something other
// than the scan itself.
#pragma once
#include <stdint.h>

#include "common.h"

namespace advhip {
namespace {

constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;  // 1024 elements per workgroup

__host__ __device__ inline uint32_t zero_of(const uint32_t*) { return 0u; }

template <class T>
__device__ __forceinline__ T block_scan_inclusive(T v, T* sh /* [2][256] */) {
  const int tid = threadIdx.x;
  int cur = 0;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    T x = sh[cur * 256 + tid];
    if (tid >= off) x = sh[cur * 256 + tid - off] + x;
    sh[(cur ^ 1) * 256 + tid] = x;
    __syncthreads();
    cur ^= 1;
  }
  return sh[cur * 256 + tid];
}

template <class T>
struct ArrayIO {  // exclusive scan of an array in place
  T* a;
  __device__ T load(long long i) const { return a[i]; }
  __device__ void store(long long i, const T& excl, const T&) const { a[i] = excl; }
};

template <class T, class IO>
__global__ __launch_bounds__(256) void scan_reduce_kernel(IO io, long long n, T* __restrict__ partials) {
  __shared__ T sh[2 * 256];
  const long long first = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  T sum = zero_of((const T*)nullptr);
  for (int j = 0; j < SCAN_ITEMS; ++j)
    if (first + j < n) sum = sum + io.load(first + j);
  const T incl = block_scan_inclusive(sum, sh);
  if (threadIdx.x == 255) partials[blockIdx.x] = incl;
}

// `partials`: the exclusive scan of the tile sums (null: a single tile)
template <class T, class IO>
__global__ __launch_bounds__(256) void scan_apply_kernel(IO io, long long n, const T* __restrict__ partials) {
  __shared__ T sh[2 * 256];
  const long long first = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  T v[SCAN_ITEMS];
  T sum = zero_of((const T*)nullptr);
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    v[j] = first + j < n ? io.load(first + j) : zero_of((const T*)nullptr);
    sum = sum + v[j];
  }
  block_scan_inclusive(sum, sh);
  // (after the helper's last barrier the result sits in buffer 0: eight steps, an even number of swaps)
  T run = threadIdx.x ? sh[threadIdx.x - 1] : zero_of((const T*)nullptr);
  if (partials) run = partials[blockIdx.x] + run;
  for (int j = 0; j < SCAN_ITEMS; ++j) {
    if (first + j >= n) break;
    const T incl = run + v[j];
    io.store(first + j, run, incl);
    run = incl;
  }
}

inline long long align256(long long b) { return (b + 255) & ~255ll; }

// bytes of partials an n-element scan needs below `ws`
inline long long scan_ws_bytes(long long n, long long elem) {
  long long total = 0;
  while (n > SCAN_TILE) {
    n = (n + SCAN_TILE - 1) / SCAN_TILE;
    total += align256(n * elem);
  }
  return total;
}

template <class T, class IO>
void scan_launch(IO io, long long n, char* ws, hipStream_t s) {
  const long long tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (tiles == 1) {
    hipLaunchKernelGGL((scan_apply_kernel<T, IO>), dim3(1), dim3(256), 0, s, io, n, (const T*)nullptr);
    return;
  }
  T* partials = (T*)ws;
  hipLaunchKernelGGL((scan_reduce_kernel<T, IO>), dim3((unsigned)tiles), dim3(256), 0, s, io, n, partials);
  scan_launch<T, ArrayIO<T>>(ArrayIO<T>{partials}, tiles, ws + align256(tiles * (long long)sizeof(T)), s);
  hipLaunchKernelGGL((scan_apply_kernel<T, IO>), dim3((unsigned)tiles), dim3(256), 0, s, io, n, (const T*)partials);
}

}  // namespace
}  // namespace advhip
