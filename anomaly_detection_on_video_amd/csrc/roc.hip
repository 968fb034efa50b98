// Weighted ROC counts on the device (include/advhip.h: advhip_roc_counts): M items (score, pos, neg) -> one entry per distinct
// score in descending order with the running sums of pos / neg -- the tps / fps arrays of metrics._ranked, integer for integer.
//
//   key      fp32 -> uint32 whose ASCENDING order is the DESCENDING order of the floats: -0.0 becomes +0.0 first, then the usual
//            order-preserving map (negative: all bits flipped, else the sign bit set), then all bits flipped.  Two scores share a
//            key iff they are equal as floats; denormals keep their own keys (nothing is flushed: only bits are compared).
//   sort     stable LSD radix sort of (key, item index), four passes of 8 bits.  A pass is three steps, each its own launch(es):
//            per-tile digit histograms -> exclusive scan of the (digit, tile) table -> stable scatter.
//   counts   inclusive int64 scan of (pos, neg, group-end flag) over the sorted order; an item that ends a group (its key differs
//            from the next one's, or it is the last) writes entry [flags before it]: its score, and the two running sums.
//
// No workgroup waits on another one: every multi-block scan is reduce / scan the partials (recursively) / apply, as separate
// launches on the caller's stream.  Every result is an integer or a copied input float and nothing depends on scheduling (the
// only atomics are integer adds: LDS histogram bins and the count of non-finite scores).
#include <stdint.h>

#include "common.h"
#include "scan.h"

namespace advhip {
namespace {

constexpr int RADIX_CHUNKS = 8;                 // a radix tile is RADIX_CHUNKS rounds of one item per thread
constexpr int RADIX_TILE = 256 * RADIX_CHUNKS;  // 2048 items per workgroup

struct Tri {  // (sum of pos, sum of neg, group ends) up to and including an item
  long long p, n, g;
};
__host__ __device__ inline Tri operator+(const Tri& a, const Tri& b) { return {a.p + b.p, a.n + b.n, a.g + b.g}; }
__host__ __device__ inline Tri zero_of(const Tri*) { return {0, 0, 0}; }

__device__ __forceinline__ uint32_t score_key(float s, bool* finite) {
  uint32_t u = __float_as_uint(s);
  *finite = (u & 0x7f800000u) != 0x7f800000u;
  if (u == 0x80000000u) u = 0u;                                    // -0.0 == +0.0: one group
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending with the floats
  return ~asc;
}

// keys, the identity permutation, and the number of non-finite scores (one integer atomic per workgroup that saw any)
__global__ __launch_bounds__(256) void roc_keys_kernel(const float* __restrict__ scores, uint32_t* __restrict__ keys,
                                                       uint32_t* __restrict__ idx, long long M, long long* __restrict__ meta) {
  __shared__ unsigned int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < M) {
    bool finite;
    keys[i] = score_key(scores[i], &finite);
    idx[i] = (uint32_t)i;
    if (!finite) atomicAdd(&bad, 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0 && bad) atomicAdd((unsigned long long*)(meta + 1), (unsigned long long)bad);
}

// hist[digit * tiles + tile]: the flat exclusive scan of this table is where (digit, tile)'s first item goes
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ hist, long long M,
                                                         unsigned tiles, int shift) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * RADIX_TILE;
  for (int c = 0; c < RADIX_CHUNKS; ++c) {
    const long long i = base + c * 256 + threadIdx.x;
    if (i < M) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one tile.  Round c ranks 256 items: inside a wave an item's rank among the lanes with its digit comes from
// eight ballots (the lanes that agree on every digit bit) and a popcount of the lanes below; the first lane of each digit
// leaves the wave's count in LDS, and an item's slot is the digit's running offset + the counts of the waves before + its rank.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                            uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                            const uint32_t* __restrict__ offs, long long M, unsigned tiles, int shift) {
  __shared__ unsigned int cnt[4][256];
  __shared__ unsigned int run[256];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long base = (long long)blockIdx.x * RADIX_TILE;
  run[tid] = offs[(size_t)tid * tiles + blockIdx.x];
  for (int c = 0; c < RADIX_CHUNKS; ++c) {
    if (base + c * 256 >= M) break;  // (uniform over the workgroup)
    cnt[0][tid] = 0;
    cnt[1][tid] = 0;
    cnt[2][tid] = 0;
    cnt[3][tid] = 0;
    __syncthreads();
    const long long i = base + c * 256 + tid;
    const bool valid = i < M;
    const uint32_t k = valid ? kin[i] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) cnt[w][d] = (unsigned)__popcll(peers);
    __syncthreads();
    if (valid) {
      unsigned slot = run[d] + rank;
      for (int v = 0; v < w; ++v) slot += cnt[v][d];
      kout[slot] = k;
      vout[slot] = vin[i];
    }
    __syncthreads();
    run[tid] += cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
    __syncthreads();
  }
}

// ---- scans (scan.h): reduce / scan the partials / apply ---------------------------------------------------------------------------
struct RocIO {  // the counts pass: reads the sorted order, writes the compacted curve
  const uint32_t* keys;
  const uint32_t* idx;
  const int32_t* pos;
  const int32_t* neg;
  const float* scores;
  float* thresholds;
  long long* tps;
  long long* fps;
  long long* meta;
  long long M;
  __device__ Tri load(long long i) const {
    const uint32_t id = idx[i];
    const bool end = i == M - 1 || keys[i] != keys[i + 1];
    return {(long long)pos[id], (long long)neg[id], end ? 1ll : 0ll};
  }
  __device__ void store(long long i, const Tri& excl, const Tri& incl) const {
    if (incl.g == excl.g) return;  // not the end of a group
    const long long g = excl.g;    // < number of groups <= M
    thresholds[g] = scores[idx[i]];
    tps[g] = incl.p;
    fps[g] = incl.n;
    if (i == M - 1) {
      meta[0] = incl.g;
      meta[2] = incl.p;
      meta[3] = incl.n;
    }
  }
};

struct RocLayout {
  long long tiles, keys, hist, hist_scan, tri_scan, total;  // byte offsets / sizes
  explicit RocLayout(long long M) {
    tiles = (M + RADIX_TILE - 1) / RADIX_TILE;
    keys = align256(M * 4);  // four of them: keys and indices, in and out
    hist = align256(256 * tiles * 4);
    hist_scan = scan_ws_bytes(256 * tiles, 4);
    tri_scan = scan_ws_bytes(M, sizeof(Tri));
    total = 4 * keys + hist + (hist_scan > tri_scan ? hist_scan : tri_scan);
  }
};

}  // namespace
}  // namespace advhip

using namespace advhip;

extern "C" int64_t advhip_roc_counts_ws_bytes(int64_t M) {
  if (M < 1 || M >= (1ll << 31)) {
    set_error("roc_counts: M = %lld outside [1, 2^31)", (long long)M);
    return ADVHIP_EINVAL;
  }
  return RocLayout(M).total;
}

extern "C" int advhip_roc_counts(const float* scores, const int32_t* pos, const int32_t* neg, int64_t M, float* thresholds, int64_t* tps,
                                 int64_t* fps, int64_t* meta, void* workspace, int64_t workspace_bytes, void* stream) {
  ADVHIP_REQUIRE(M >= 1 && M < (1ll << 31), "roc_counts: M = %lld outside [1, 2^31)", (long long)M);
  ADVHIP_REQUIRE(scores && pos && neg && thresholds && tps && fps && meta && workspace, "roc_counts: null pointer");
  const RocLayout L(M);
  ADVHIP_REQUIRE(workspace_bytes >= L.total, "roc_counts: workspace of %lld bytes, %lld needed (advhip_roc_counts_ws_bytes)",
                 (long long)workspace_bytes, L.total);
  ADVHIP_REQUIRE(((uintptr_t)workspace & 7) == 0, "roc_counts: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint32_t* k[2] = {(uint32_t*)ws, (uint32_t*)(ws + L.keys)};
  uint32_t* v[2] = {(uint32_t*)(ws + 2 * L.keys), (uint32_t*)(ws + 3 * L.keys)};
  uint32_t* hist = (uint32_t*)(ws + 4 * L.keys);
  char* scan_ws = ws + 4 * L.keys + L.hist;
  const unsigned tiles = (unsigned)L.tiles;

  if (hipMemsetAsync(meta, 0, 4 * sizeof(int64_t), s) != hipSuccess) return check_launch("roc_counts (meta)");
  hipLaunchKernelGGL(roc_keys_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, scores, k[0], v[0], (long long)M, (long long*)meta);
  for (int pass = 0; pass < 4; ++pass) {
    const int in = pass & 1, shift = 8 * pass;
    hipLaunchKernelGGL(radix_hist_kernel, dim3(tiles), dim3(256), 0, s, (const uint32_t*)k[in], hist, (long long)M, tiles, shift);
    scan_launch<uint32_t, ArrayIO<uint32_t>>(ArrayIO<uint32_t>{hist}, 256ll * tiles, scan_ws, s);
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(tiles), dim3(256), 0, s, (const uint32_t*)k[in], (const uint32_t*)v[in], k[in ^ 1], v[in ^ 1],
                       (const uint32_t*)hist, (long long)M, tiles, shift);
  }
  // (four passes: the sorted order is back in buffer 0)
  const RocIO io{k[0], v[0], pos, neg, scores, thresholds, (long long*)tps, (long long*)fps, (long long*)meta, (long long)M};
  scan_launch<Tri, RocIO>(io, M, scan_ws, s);
  return check_launch("roc_counts");
}
