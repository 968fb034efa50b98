// Live anomaly events: the event rule of events.hip as a per-camera streaming state machine (include/advhip.h: "live events").
// Every camera keeps its last `smooth` samples in a ring (sample k in slot k % smooth), an open candidate and a log of its last K
// events, all in tensors the caller owns.  One launch feeds one new sample to each listed camera, or finishes / resets the listed
// cameras.  One wavefront (= one workgroup) per camera: the ring row is staged into LDS by all lanes, then lane 0 alone runs the
// ordered fp32 sum and the state machine, so every order is fixed: no atomics, no workgroup waits on another, the same bits in
// every run.  Only the listed cameras' state is written.
#include <math.h>

#include "common.h"

namespace advhip {

constexpr int LE_MAX_SMOOTH = 1023;
constexpr long long LE_MAX_SAMPLES = 2147483647ll;  // positions are int32: end <= 2^31 - 1

struct LiveEventsArgs {
  const float* scores;
  const int* cam_ids;
  float* ring;          // (n_cam, smooth)
  long long* samples;   // (n_cam,)
  int* cand_int;        // (n_cam, ADVHIP_LIVE_EVENTS_CAND_INTS) = {start, last_active, peak_frame, strong, generation}
  float* cand_peak;     // (n_cam,)
  double* cand_sum;     // (n_cam, 2) = {running sum since start, its value at last_active}
  int* alert;           // (n_cam,)
  int* open_start;      // (n_cam,)
  int* log_int;         // (n_cam, K, 4) = {generation, start, end, peak_frame}
  float* log_f;         // (n_cam, K, 2) = {peak, mean}
  long long* emitted;   // (n_cam,)
  int n_cam, K, smooth, merge_gap, min_len, by_camera, mode;
  float low, high;
};

// One camera's candidate in registers, and where its events go.
struct LiveCandidate {
  int start, last_active, peak_frame, strong, generation;
  float peak;
  double run, snap;
  long long emitted;

  // the open candidate ends at last_active + 1: an event iff it is strong and long enough (event j in log slot j % K)
  __device__ void close(const LiveEventsArgs& a, int c) {
    const int end = last_active + 1;
    if (strong && end - start >= a.min_len) {
      const long long slot = (long long)c * a.K + emitted % a.K;
      int* li = a.log_int + slot * 4;
      float* lf = a.log_f + slot * 2;
      li[0] = generation;
      li[1] = start;
      li[2] = end;
      li[3] = peak_frame;
      lf[0] = peak;
      lf[1] = (float)(snap / (double)(end - start));
      emitted += 1;
    }
    start = -1;
  }

  // the final smoothed sample y at position t, in order
  __device__ void step(const LiveEventsArgs& a, int c, int t, float y) {
    const bool active = y >= a.low;  // (a NaN is neither active nor strong)
    if (start >= 0) {
      run += (double)y;
      if (active) {
        last_active = t;
        snap = run;
        if (y >= a.high) strong = 1;
        if (y > peak) {  // (strict: the first position of the largest value, of -0.0 and +0.0 the earlier one)
          peak = y;
          peak_frame = t;
        }
      } else if (t - last_active > a.merge_gap) {
        close(a, c);
      }
    } else if (active) {
      start = last_active = peak_frame = t;
      strong = y >= a.high ? 1 : 0;
      peak = y;
      run = 0.0 + (double)y;
      snap = run;
    }
  }
};

// x[lo .. hi] of the camera's series out of the staged ring, summed in fp32 in ascending order from +0.0, one division
__device__ __forceinline__ float live_window_mean(const float* row, int smooth, long long lo, long long hi) {
  float acc = 0.f;
  int slot = (int)(lo % smooth);
  for (long long k = lo; k <= hi; ++k) {
    acc += row[slot];
    slot = slot + 1 == smooth ? 0 : slot + 1;
  }
  return acc / (float)(hi - lo + 1);
}

__global__ __launch_bounds__(64) void live_events_kernel(LiveEventsArgs a, int nb) {
  __shared__ float row[LE_MAX_SMOOTH + 1];
  const int v = blockIdx.x;
  if (v >= nb) return;
  const int c = a.cam_ids[v];
  if (c < 0 || c >= a.n_cam) return;  // (the whole workgroup: nothing waits at the barrier)
  const long long n = a.samples[c];
  // a count no tracker leaves behind (positions are int32; a negative event number has no log slot): nothing is written
  if (n < 0 || n > LE_MAX_SAMPLES || (a.mode == ADVHIP_LIVE_EVENTS_UPDATE && n == LE_MAX_SAMPLES) || a.emitted[c] < 0) return;
  const int smooth = a.smooth, h = (smooth - 1) / 2;
  float* ring = a.ring + (long long)c * smooth;
  if (a.mode != ADVHIP_LIVE_EVENTS_RESET)
    for (int i = threadIdx.x; i < smooth; i += 64) row[i] = ring[i];
  __syncthreads();
  if (threadIdx.x != 0) return;

  int* ci = a.cand_int + (long long)c * ADVHIP_LIVE_EVENTS_CAND_INTS;
  LiveCandidate s;
  s.start = ci[0];
  s.last_active = ci[1];
  s.peak_frame = ci[2];
  s.strong = ci[3];
  s.generation = ci[4];
  s.peak = a.cand_peak[c];
  s.run = a.cand_sum[2 * c];
  s.snap = a.cand_sum[2 * c + 1];
  s.emitted = a.emitted[c];
  long long count = n;

  if (a.mode == ADVHIP_LIVE_EVENTS_UPDATE) {
    const float x = a.scores[a.by_camera ? c : v];
    const int slot = (int)(n % smooth);
    ring[slot] = x;
    row[slot] = x;
    count = n + 1;
    if (n >= h) {  // y[n - h] is final: its window [max(0, n - 2 h), n] is whole
      const long long t = n - h;
      s.step(a, c, (int)t, live_window_mean(row, smooth, t > h ? t - h : 0, n));
    }
  } else {
    if (a.mode == ADVHIP_LIVE_EVENTS_FINISH) {  // the pending min(h, n) samples, their windows clipped at n - 1, then the open candidate
      for (long long t = n > h ? n - h : 0; t < n; ++t) s.step(a, c, (int)t, live_window_mean(row, smooth, t > h ? t - h : 0, n - 1));
      if (s.start >= 0) s.close(a, c);
    }
    s.start = -1;
    s.generation += 1;
    count = 0;
  }

  const bool open = s.start >= 0;
  if (!open) {  // (no stale candidate fields: the state of two runs compares equal whatever they closed)
    s.last_active = s.peak_frame = -1;
    s.strong = 0;
    s.peak = 0.f;
    s.run = s.snap = 0.0;
  }
  ci[0] = s.start;
  ci[1] = s.last_active;
  ci[2] = s.peak_frame;
  ci[3] = s.strong;
  ci[4] = s.generation;
  a.cand_peak[c] = s.peak;
  a.cand_sum[2 * c] = s.run;
  a.cand_sum[2 * c + 1] = s.snap;
  a.emitted[c] = s.emitted;
  a.samples[c] = count;
  a.alert[c] = open && s.strong && s.last_active + 1 - s.start >= a.min_len ? 1 : 0;
  a.open_start[c] = s.start;
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_live_events_update_f32(const float* scores, const int32_t* cam_ids, float* ring, int64_t* samples, int32_t* cand_int,
                                             float* cand_peak, double* cand_sum, int32_t* alert, int32_t* open_start, int32_t* log_int,
                                             float* log_f, int64_t* emitted, int32_t nb, int32_t n_cam, int32_t K, int32_t smooth, float low,
                                             float high, int32_t merge_gap, int32_t min_len, int32_t by_camera, int32_t mode, void* stream) {
  ADVHIP_REQUIRE(cam_ids && ring && samples && cand_int && cand_peak && cand_sum && alert && open_start && log_int && log_f && emitted,
                 "live_events: null pointer");
  ADVHIP_REQUIRE(mode == ADVHIP_LIVE_EVENTS_UPDATE || mode == ADVHIP_LIVE_EVENTS_FINISH || mode == ADVHIP_LIVE_EVENTS_RESET,
                 "live_events: mode = %d is not update (0), finish (1) or reset (2)", mode);
  ADVHIP_REQUIRE(scores || mode != ADVHIP_LIVE_EVENTS_UPDATE, "live_events: null pointer (an update reads scores)");
  ADVHIP_REQUIRE(nb >= 1 && n_cam >= 1 && K >= 1, "live_events: bad shape (nb = %d, n_cam = %d, K = %d)", nb, n_cam, K);
  ADVHIP_REQUIRE(smooth >= 1 && smooth <= LE_MAX_SMOOTH && smooth % 2 == 1, "live_events: smooth = %d is not an odd window in [1, %d]", smooth,
                 LE_MAX_SMOOTH);
  ADVHIP_REQUIRE(merge_gap >= 0, "live_events: merge_gap = %d is negative", merge_gap);
  ADVHIP_REQUIRE(min_len >= 1, "live_events: min_len = %d below 1", min_len);
  ADVHIP_REQUIRE(isfinite(low) && isfinite(high), "live_events: thresholds low = %g, high = %g must be finite", (double)low, (double)high);
  ADVHIP_REQUIRE(low <= high, "live_events: low = %g above high = %g", (double)low, (double)high);
  ADVHIP_REQUIRE(by_camera == 0 || by_camera == 1, "live_events: by_camera = %d is not 0 or 1", by_camera);
  LiveEventsArgs a;
  a.scores = scores;
  a.cam_ids = (const int*)cam_ids;
  a.ring = ring;
  a.samples = (long long*)samples;
  a.cand_int = (int*)cand_int;
  a.cand_peak = cand_peak;
  a.cand_sum = cand_sum;
  a.alert = (int*)alert;
  a.open_start = (int*)open_start;
  a.log_int = (int*)log_int;
  a.log_f = log_f;
  a.emitted = (long long*)emitted;
  a.n_cam = n_cam;
  a.K = K;
  a.smooth = smooth;
  a.merge_gap = merge_gap;
  a.min_len = min_len;
  a.by_camera = by_camera;
  a.mode = mode;
  a.low = low;
  a.high = high;
  hipLaunchKernelGGL(live_events_kernel, dim3((unsigned)nb), dim3(64), 0, (hipStream_t)stream, a, (int)nb);
  return check_launch("live_events");
}
