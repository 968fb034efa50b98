// Anomaly events from per-frame scores on the device (include/advhip.h: advhip_smooth_scores_f32, advhip_score_events): a ragged
// batch of V videos flattened into N positions, video v = [offsets[v], offsets[v + 1]).  No step looks across a video boundary.
//
//   smooth   one thread per position with its own ascending fp32 loop over the clipped window, one division by the count: the
//            rule's bits.  A workgroup stages its 256 positions and a halo of (window - 1) / 2 on either side in LDS; the largest
//            window (1023) needs 1278 floats, so every window is served from LDS and there is no second path.
//   events   a frame is active iff y >= low.  The last active position before a frame comes from an exclusive max-scan of
//            (active ? position : -1), the next one after it from the same scan over the reversed order; videos are contiguous
//            ranges, so "inside my video" is a comparison with the video's bounds and the scans need no segment flags.  The apply
//            step of either scan writes the start / end marks.  A scan of the two marks numbers the candidates (the k-th start
//            pairs with the k-th end), one wave per candidate reduces strong / peak / first peak frame / the float64 sum in a
//            strided loop and a fixed shuffle tree, and a scan of the keep flags compacts the events in (video, start) order.
//
// No workgroup waits on another one (scan.h).  Every reduction has a fixed order, there is no float atomic: two runs give the
// same bits.  The only atomic is the integer count of a video's events.  Offsets are read on the device and never trusted for an
// address: a position's video comes from a binary search that ends inside [0, V), its bounds are clamped to [0, N], and every
// index into the candidate and event arrays is checked against the array's size.
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "scan.h"

namespace advhip {
namespace {

constexpr int SMOOTH_MAX_WINDOW = 1023;
constexpr int SMOOTH_STAGE = 256 + SMOOTH_MAX_WINDOW - 1;  // a workgroup's positions and the widest halo on both sides

struct VideoRange {
  int v;
  long long s, e;  // 0 <= s <= i < e <= N for the position i it was made for
};

// The video of position i: the last v with offsets[v] <= i (videos of length 0 share their offset with the next one and are
// stepped over).  v is in [0, V) whatever the array holds.
__device__ __forceinline__ VideoRange video_range(const long long* __restrict__ offsets, int V, long long N, long long i) {
  int lo = 0, hi = V;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  const long long s = offsets[lo], e = offsets[lo + 1];
  return {lo, s < 0 ? 0 : (s > i ? i : s), e > N ? N : (e <= i ? i + 1 : e)};
}

__global__ __launch_bounds__(256) void smooth_kernel(const float* __restrict__ x, const long long* __restrict__ offsets, int V, long long N,
                                                     int h, float* __restrict__ out) {
  __shared__ float tile[SMOOTH_STAGE];
  const long long base = (long long)blockIdx.x * 256 - h;  // the position tile[0] holds
  for (int j = threadIdx.x; j < 256 + 2 * h; j += 256) {
    const long long g = base + j;
    tile[j] = g >= 0 && g < N ? x[g] : 0.f;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const VideoRange r = video_range(offsets, V, N, i);
  const long long a = i - h > r.s ? i - h : r.s, b = i + h < r.e - 1 ? i + h : r.e - 1;  // |u - i| <= h: inside the staged range
  float acc = 0.f;
  for (long long u = a; u <= b; ++u) acc += tile[u - base];
  out[i] = acc / (float)(b - a + 1);
}

struct MaxI {  // the largest position so far, -1: none
  int v;
};
__host__ __device__ inline MaxI operator+(const MaxI& a, const MaxI& b) { return {a.v > b.v ? a.v : b.v}; }
__host__ __device__ inline MaxI zero_of(const MaxI*) { return {-1}; }

struct Marks {  // (starts, ends) up to and including a position
  uint32_t s, e;
};
__host__ __device__ inline Marks operator+(const Marks& a, const Marks& b) { return {a.s + b.s, a.e + b.e}; }
__host__ __device__ inline Marks zero_of(const Marks*) { return {0u, 0u}; }

// Scan element j stands for position j (forward) or N - 1 - j (reverse); `excl` is then the nearest active element before j.
// A frame starts (ends) a candidate iff it is active and no frame of the merge_gap + 1 before (after) it inside its video is.
template <bool REVERSE>
struct MarkIO {
  const float* y;
  const long long* offsets;
  int V;
  long long N;
  float low;
  long long gap;
  uint8_t* mark;
  __device__ MaxI load(long long j) const {
    const long long i = REVERSE ? N - 1 - j : j;
    return {y[i] >= low ? (int)j : -1};
  }
  __device__ void store(long long j, const MaxI& excl, const MaxI& incl) const {
    const long long i = REVERSE ? N - 1 - j : j;
    uint8_t m = 0;
    if (incl.v == (int)j) {  // active
      const VideoRange r = video_range(offsets, V, N, i);
      // the elements of the video's frames that must hold no active one: [from, j)
      long long from = j - gap - 1;
      const long long edge = REVERSE ? N - r.e : r.s;  // the video's first element in scan order
      if (from < edge) from = edge;
      m = excl.v < from;
    }
    mark[i] = m;
  }
};

struct CandidateIO {  // numbers the marks: candidate k = [k-th start, k-th end]
  const uint8_t* start_mark;
  const uint8_t* end_mark;
  int* cand_start;
  int* cand_end;  // exclusive
  long long* ncand;
  long long N, cand_cap;
  __device__ Marks load(long long i) const { return {start_mark[i], end_mark[i]}; }
  __device__ void store(long long i, const Marks& excl, const Marks& incl) const {
    if (incl.s != excl.s && excl.s < cand_cap) cand_start[excl.s] = (int)i;
    if (incl.e != excl.e && excl.e < cand_cap) cand_end[excl.e] = (int)i + 1;
    if (i == N - 1) {
      long long c = incl.s < incl.e ? incl.s : incl.e;  // (equal for offsets that partition [0, N))
      *ncand = c < cand_cap ? c : cand_cap;
    }
  }
};

// One wave per candidate: lane l takes frames start + l, start + l + 64, ... in ascending order, then a shuffle tree in which
// lane l takes in lane l + 32, 16, ... 1.  The order is fixed, so the float64 sum has the same bits in every run.  Leaves the
// candidate's video, its bounds local to the video, the peak, its first frame, the mean and whether it is kept.
__global__ __launch_bounds__(256) void candidate_kernel(const float* __restrict__ y, const long long* __restrict__ offsets, int V, long long N,
                                                        float high, long long min_len, int* __restrict__ cand_start, int* __restrict__ cand_end,
                                                        const long long* __restrict__ ncand, int* __restrict__ cand_video,
                                                        int* __restrict__ cand_peak_frame, float* __restrict__ cand_peak,
                                                        float* __restrict__ cand_mean, uint32_t* __restrict__ cand_keep) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * 4, C = *ncand;
  for (long long k = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); k < C; k += waves) {  // (uniform over the wave)
    long long a = cand_start[k], b = cand_end[k];
    if (a < 0) a = 0;
    if (b > N) b = N;
    double sum = 0.0;
    float best = -INFINITY;
    int best_at = 0x7fffffff;
    bool strong = false;
    for (long long t = a + lane; t < b; t += 64) {
      const float v = y[t];
      sum += (double)v;
      strong = strong || v >= high;
      if (v > best) {  // (a NaN is never greater: ignored)
        best = v;
        best_at = (int)t;
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double o_sum = __shfl_down(sum, off);
      const float o_best = __shfl_down(best, off);
      const int o_at = __shfl_down(best_at, off);
      sum += o_sum;
      if (o_best > best || (o_best == best && o_at < best_at)) {
        best = o_best;
        best_at = o_at;
      }
    }
    const bool any_strong = __any(strong);
    if (lane == 0) {
      const bool some = b > a;
      const VideoRange r = video_range(offsets, V, N, some ? a : 0);
      cand_video[k] = r.v;
      cand_start[k] = (int)(a - r.s);
      cand_end[k] = (int)(b - r.s);
      cand_peak_frame[k] = (int)(best_at - r.s);
      cand_peak[k] = best;
      cand_mean[k] = some ? (float)(sum / (double)(b - a)) : 0.f;
      cand_keep[k] = some && any_strong && b - a >= min_len;
    }
  }
}

struct KeepIO {  // compacts the kept candidates in order
  const uint32_t* cand_keep;
  const long long* ncand;
  const int* cand_video;
  const int* cand_start;
  const int* cand_end;
  const int* cand_peak_frame;
  const float* cand_peak;
  const float* cand_mean;
  int* ev_int;
  float* ev_f;
  int* counts;
  long long* meta;
  long long cap, n;
  __device__ uint32_t load(long long k) const { return k < *ncand ? cand_keep[k] : 0u; }
  __device__ void store(long long k, const uint32_t& excl, const uint32_t& incl) const {
    if (incl != excl && (long long)excl < cap) {
      const int v = cand_video[k];  // in [0, V): video_range's
      int* row = ev_int + 4 * (long long)excl;
      row[0] = v;
      row[1] = cand_start[k];
      row[2] = cand_end[k];
      row[3] = cand_peak_frame[k];
      ev_f[2 * (long long)excl] = cand_peak[k];
      ev_f[2 * (long long)excl + 1] = cand_mean[k];
      atomicAdd(counts + v, 1);
    }
    if (k == n - 1) {
      meta[0] = incl;
      meta[1] = (long long)incl < cap ? (long long)incl : cap;
    }
  }
};

struct EventsLayout {
  long long cand_cap, marks, cand, ncand, scan, total;  // sizes in bytes (cand_cap: entries)
  EventsLayout(long long N, long long V) {
    // candidates of one video are separated by a frame that is not active: at most sum of ceil(L_v / 2) <= (N + V) / 2 of them
    cand_cap = (N + V + 1) / 2 < N ? (N + V + 1) / 2 : N;
    marks = align256(N);            // two of them: start and end marks, one byte each
    cand = align256(cand_cap * 4);  // seven of them: start, end, video, peak frame, peak, mean, keep
    ncand = 256;
    const long long s1 = scan_ws_bytes(N, sizeof(Marks)), s2 = scan_ws_bytes(cand_cap, 4);
    scan = s1 > s2 ? s1 : s2;
    total = 2 * marks + 7 * cand + ncand + scan;
  }
};

const char* events_shape_error(int64_t N, int64_t V) {
  if (N < 1 || N >= (1ll << 31)) return "N outside [1, 2^31)";
  if (V < 1 || V >= (1ll << 31)) return "V outside [1, 2^31)";
  return nullptr;
}

}  // namespace
}  // namespace advhip

using namespace advhip;

extern "C" int advhip_smooth_scores_f32(const float* scores, const int64_t* offsets, int64_t V, int64_t N, int32_t window, float* out,
                                        void* stream) {
  ADVHIP_REQUIRE(scores && offsets && out, "smooth_scores: null pointer");
  const char* why = events_shape_error(N, V);
  ADVHIP_REQUIRE(!why, "smooth_scores: N = %lld, V = %lld: %s", (long long)N, (long long)V, why);
  ADVHIP_REQUIRE(window >= 1 && window <= SMOOTH_MAX_WINDOW && (window & 1), "smooth_scores: window %d is not an odd number in [1, %d]", window,
                 SMOOTH_MAX_WINDOW);
  ADVHIP_REQUIRE(scores != out, "smooth_scores: out must not be the scores (a workgroup reads its neighbours' positions)");
  hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores, (const long long*)offsets,
                     (int)V, (long long)N, (window - 1) / 2, out);
  return check_launch("smooth_scores");
}

extern "C" int64_t advhip_score_events_ws_bytes(int64_t N, int64_t V) {
  const char* why = events_shape_error(N, V);
  if (why) {
    set_error("score_events: N = %lld, V = %lld: %s", (long long)N, (long long)V, why);
    return ADVHIP_EINVAL;
  }
  return EventsLayout(N, V).total;
}

extern "C" int advhip_score_events(const float* smoothed, const int64_t* offsets, int64_t V, int64_t N, float low, float high, int32_t merge_gap,
                                   int32_t min_len, int32_t* ev_int, float* ev_f, int64_t cap, int32_t* counts, int64_t* meta, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  ADVHIP_REQUIRE(smoothed && offsets && ev_int && ev_f && counts && meta && workspace, "score_events: null pointer");
  const char* why = events_shape_error(N, V);
  ADVHIP_REQUIRE(!why, "score_events: N = %lld, V = %lld: %s", (long long)N, (long long)V, why);
  ADVHIP_REQUIRE(isfinite(low) && isfinite(high), "score_events: thresholds low = %g, high = %g must be finite", (double)low, (double)high);
  ADVHIP_REQUIRE(low <= high, "score_events: low = %g above high = %g", (double)low, (double)high);
  ADVHIP_REQUIRE(merge_gap >= 0, "score_events: merge_gap = %d is negative", merge_gap);
  ADVHIP_REQUIRE(min_len >= 1, "score_events: min_len = %d below 1", min_len);
  ADVHIP_REQUIRE(cap >= 1, "score_events: cap = %lld below 1", (long long)cap);
  const EventsLayout L(N, V);
  ADVHIP_REQUIRE(workspace_bytes >= L.total, "score_events: workspace of %lld bytes, %lld needed (advhip_score_events_ws_bytes)",
                 (long long)workspace_bytes, L.total);
  ADVHIP_REQUIRE(((uintptr_t)workspace & 7) == 0, "score_events: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  uint8_t* start_mark = (uint8_t*)ws;
  uint8_t* end_mark = (uint8_t*)(ws + L.marks);
  char* c = ws + 2 * L.marks;
  int* cand_start = (int*)c;
  int* cand_end = (int*)(c + L.cand);
  int* cand_video = (int*)(c + 2 * L.cand);
  int* cand_peak_frame = (int*)(c + 3 * L.cand);
  float* cand_peak = (float*)(c + 4 * L.cand);
  float* cand_mean = (float*)(c + 5 * L.cand);
  uint32_t* cand_keep = (uint32_t*)(c + 6 * L.cand);
  long long* ncand = (long long*)(c + 7 * L.cand);
  char* scan_ws = c + 7 * L.cand + L.ncand;
  const long long* offs = (const long long*)offsets;

  if (hipMemsetAsync(counts, 0, (size_t)V * sizeof(int32_t), s) != hipSuccess) return check_launch("score_events (counts)");
  scan_launch<MaxI, MarkIO<false>>(MarkIO<false>{smoothed, offs, (int)V, (long long)N, low, (long long)merge_gap, start_mark}, N, scan_ws, s);
  scan_launch<MaxI, MarkIO<true>>(MarkIO<true>{smoothed, offs, (int)V, (long long)N, low, (long long)merge_gap, end_mark}, N, scan_ws, s);
  scan_launch<Marks, CandidateIO>(CandidateIO{start_mark, end_mark, cand_start, cand_end, ncand, (long long)N, L.cand_cap}, N, scan_ws, s);
  const long long blocks = (L.cand_cap + 3) / 4;
  hipLaunchKernelGGL(candidate_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, smoothed, offs, (int)V, (long long)N, high,
                     (long long)min_len, cand_start, cand_end, (const long long*)ncand, cand_video, cand_peak_frame, cand_peak, cand_mean,
                     cand_keep);
  const KeepIO keep{cand_keep, ncand,  cand_video, cand_start, cand_end,         cand_peak_frame, cand_peak,
                    cand_mean, ev_int, ev_f,       counts,     (long long*)meta, (long long)cap,  L.cand_cap};
  scan_launch<uint32_t, KeepIO>(keep, L.cand_cap, scan_ws, s);
  return check_launch("score_events");
}
