// Live scoring: the state in front of the padded scorer pass and the read-out behind it (include/advhip.h: "live scoring").
// Every camera keeps its last W clips of features, magnitude channel included, in a ring on the device; the clip pushed at count k
// lies in slot k % W.  Three entry points, each a copy or a sum in an order the library has already stated: no atomics, no
// workgroup waits on another, the same bits in every run.
#include "pw_sum.h"

namespace advhip {

// One wavefront (= one workgroup) per pushed row (i, k): the slot from the camera's count, the row and its magnitude by
// pw_row_magnitude.  The count is only read here: ring_advance_kernel, launched behind this one, moves it.
__global__ __launch_bounds__(64) void ring_push_kernel(const float* __restrict__ feats, const int* __restrict__ cam_ids, float* __restrict__ ring,
                                                       const long long* __restrict__ counts, int n_cam, int ncrops, int W, int C, PwLeaves tab) {
  extern __shared__ float pw_lds[];
  const int i = blockIdx.x / ncrops, k = blockIdx.x % ncrops;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;  // (the whole workgroup: nothing waits at a barrier)
  const long long count = counts[c];
  if (count < 0) return;
  const long long slot = count % W;
  pw_row_magnitude(feats + (long long)blockIdx.x * C, ring + (((long long)c * ncrops + k) * W + slot) * (C + 1), C, tab, pw_lds);
}

__global__ __launch_bounds__(256) void ring_advance_kernel(const int* __restrict__ cam_ids, long long* __restrict__ counts, int n, int n_cam) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = cam_ids[i];
  if (c >= 0 && c < n_cam) counts[c] += 1;  // ids are distinct: one thread per count
}

// One workgroup per dst row (v, k, t), as pack_padded_kernel: dword copies of C1 floats, every lane's loads issued before its
// stores.  Rows of the ring and of dst start at 4-byte boundaries only (C1 is odd at the trained width), and the slot a row comes
// from moves by one with every push, so source and destination share a 16-byte phase in one step of four: there is no wider form.
constexpr int RW_UNROLL = 4;
__global__ __launch_bounds__(256) void ring_windows_kernel(const float* __restrict__ ring, const long long* __restrict__ counts,
                                                           const int* __restrict__ cam_ids, float* __restrict__ dst, int n_cam, int ncrops, int W,
                                                           int Tmax, int C1) {
  const long long row = blockIdx.x;  // (v * ncrops + k) * Tmax + t
  const int t = (int)(row % Tmax);
  const long long vk = row / Tmax;
  const int v = (int)(vk / ncrops), k = (int)(vk % ncrops);
  const int c = cam_ids[v];
  if (c < 0 || c >= n_cam) return;
  const long long count = counts[c];
  const long long len = min(min(count, (long long)W), (long long)Tmax);
  if (t >= len) return;  // (count <= 0: len <= 0, nothing is written)
  const long long slot = (count - len + t) % W;
  const unsigned* __restrict__ s = (const unsigned*)ring + (((long long)c * ncrops + k) * W + slot) * C1;
  unsigned* __restrict__ d = (unsigned*)dst + row * C1;
  int i = threadIdx.x;
  for (; i + 256 * (RW_UNROLL - 1) < C1; i += 256 * RW_UNROLL) {
    unsigned r[RW_UNROLL];
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) r[u] = s[i + 256 * u];
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) d[i + 256 * u] = r[u];
  }
  for (; i < C1; i += 256) d[i] = s[i];
}

// crop_mean_scatter_kernel's sum (mil.hip: crop order from 0.f, one division) at the newest clip of every listed camera
__global__ __launch_bounds__(256) void crop_mean_last_kernel(const float* __restrict__ scores, const int* __restrict__ lens,
                                                             const int* __restrict__ cam_ids, float* __restrict__ latest, int nb, int ncrops, int Tmax) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nb) return;
  const int L = lens[v];
  if (L < 1 || L > Tmax) return;
  float s = 0.f;
  for (int k = 0; k < ncrops; ++k) s += scores[((size_t)v * ncrops + k) * Tmax + (L - 1)];
  latest[cam_ids[v]] = s / (float)ncrops;
}

// ---- live frames (include/advhip.h: "live frames"): per-camera rings of the last R resized uint8 frames.  Two copies of bits in
// gather_batch_kernel's form (mil.hip): a frame is cut into chunks of FRAME_CHUNK elements of V, blockIdx.x = chunk, blockIdx.y =
// frame row; every lane issues its FRAME_UNROLL loads before its first store; all byte offsets are 64-bit.  V is u32x4 when both
// pointers and frame_bytes are multiples of 16 (the working frame, 256 x 340 x 3 = 261 120 bytes, is), one dword when they are
// multiples of 4, else one byte -- the host decides, so every frame and every ring slot starts at a multiple of sizeof(V): never
// an unaligned wide access.
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
constexpr int FRAME_UNROLL = 4;
constexpr int FRAME_CHUNK = 256 * FRAME_UNROLL;

template <typename V>
__device__ __forceinline__ void frame_copy_chunk(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, long long frame_bytes) {
  const long long nv = frame_bytes / (long long)sizeof(V);  // a frame in elements of V
  const V* __restrict__ s = reinterpret_cast<const V*>(src);
  V* __restrict__ d = reinterpret_cast<V*>(dst);
  const long long e0 = (long long)blockIdx.x * FRAME_CHUNK + threadIdx.x;
  V v[FRAME_UNROLL] = {};
#pragma unroll
  for (int u = 0; u < FRAME_UNROLL; ++u) {
    const long long e = e0 + u * 256;
    if (e < nv) v[u] = s[e];
  }
#pragma unroll
  for (int u = 0; u < FRAME_UNROLL; ++u) {
    const long long e = e0 + u * 256;
    if (e < nv) d[e] = v[u];
  }
}

// Frame i into slot counts[c] % R of camera c = cam_ids[i].  The count is only read here: ring_advance_kernel moves it.
template <typename V>
__global__ __launch_bounds__(256) void frame_ring_push_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ cam_ids,
                                                              unsigned char* __restrict__ ring, const long long* __restrict__ counts, int n_cam, int R,
                                                              long long frame_bytes) {
  const long long i = blockIdx.y;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;
  const long long count = counts[c];
  if (count < 0) return;
  frame_copy_chunk<V>(frames + i * frame_bytes, ring + ((long long)c * R + count % R) * frame_bytes, frame_bytes);
}

// dst row v * fpc + t = entry t of listed camera v's window: the frame in slot (count + t * frame_step) % R.
template <typename V>
__global__ __launch_bounds__(256) void frame_ring_windows_kernel(const unsigned char* __restrict__ ring, const long long* __restrict__ counts,
                                                                 const int* __restrict__ cam_ids, unsigned char* __restrict__ dst, int n_cam, int R,
                                                                 long long frame_bytes, int fpc, int frame_step) {
  const long long row = blockIdx.y;
  const int v = (int)(row / fpc), t = (int)(row % fpc);
  const int c = cam_ids[v];
  if (c < 0 || c >= n_cam) return;
  const long long count = counts[c];
  if (count < R) return;  // no window yet: its rows stay as they are
  const long long slot = (count + (long long)t * frame_step) % R;
  frame_copy_chunk<V>(ring + ((long long)c * R + slot) * frame_bytes, dst + row * frame_bytes, frame_bytes);
}

// The access width of a frame copy from everything that enters an address: 16, 4 or 1 bytes.
inline int frame_access_bytes(const void* a, const void* b, long long frame_bytes) {
  const unsigned long long bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (unsigned long long)frame_bytes;
  return (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 1;
}

// One frame copy of `rows` frames between `a` and `b`: the access width, the chunks of a frame, the grid's bounds, then
// launch(V{}, grid) with V = u32x4, unsigned or unsigned char -- the caller's lambda names its kernel<V> and passes its arguments.
template <typename Launch>
int launch_frame_copy(const void* a, const void* b, long long frame_bytes, long long rows, const char* who, Launch launch) {
  const int width = frame_access_bytes(a, b, frame_bytes);
  const long long chunks = (frame_bytes / width + FRAME_CHUNK - 1) / FRAME_CHUNK;
  ADVHIP_REQUIRE(rows <= 65535 && chunks * rows * 256 < (1ll << 32), "%s: %lld rows of %lld bytes are outside the launch grid", who, rows, frame_bytes);
  const dim3 grid((unsigned)chunks, (unsigned)rows);
  if (width == 16)
    launch(u32x4{}, grid);
  else if (width == 4)
    launch(unsigned{}, grid);
  else
    launch((unsigned char)0, grid);
  return check_launch(who);
}

// The counts of the n listed cameras plus one, behind the kernel that read them.
inline int launch_ring_advance(const int32_t* cam_ids, int64_t* counts, int32_t n, int32_t n_cam, void* stream, const char* who) {
  hipLaunchKernelGGL(ring_advance_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const int*)cam_ids, (long long*)counts,
                     (int)n, (int)n_cam);
  return check_launch(who);
}

// ---- live frames: motion gate (include/advhip.h: "live frames: motion gate").  Integers only, no atomics: every workgroup
// stores the count of its chunk, one workgroup per pushed row adds the counts up and applies the rule, a predicated frame copy
// moves the anchor.  The three launches cut a frame into the same chunks (launch_frame_copy's, from the same three operands);
// partial p of pushed row i lies in scratch[i * chunks + p], and the row's verdict replaces partial 0 once all are summed.
constexpr int GATE_STILL_MAX = 1 << 30;

// the sum of v over the 256 lanes of a workgroup, in every lane: xor-moves within the wave, the four waves' sums through LDS
__device__ __forceinline__ int gate_block_sum(int v, int* wave_sums) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  return wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
}

// bytes of one element of V with |a - b| > tau, compared as integers
__device__ __forceinline__ int gate_changed_bytes(unsigned a, unsigned b, int tau) {
  int n = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) {
    const int d = (int)((a >> k) & 255u) - (int)((b >> k) & 255u);
    n += (d < 0 ? -d : d) > tau;
  }
  return n;
}
__device__ __forceinline__ int gate_changed_bytes(u32x4 a, u32x4 b, int tau) {
  return gate_changed_bytes(a.x, b.x, tau) + gate_changed_bytes(a.y, b.y, tau) + gate_changed_bytes(a.z, b.z, tau) +
         gate_changed_bytes(a.w, b.w, tau);
}
__device__ __forceinline__ int gate_changed_bytes(unsigned char a, unsigned char b, int tau) {
  const int d = (int)a - (int)b;
  return (d < 0 ? -d : d) > tau;
}

// (a) workgroup (chunk, row i): the changed bytes of its chunk of frame i against the anchor of c = cam_ids[i]
template <typename V>
__global__ __launch_bounds__(256) void frame_gate_count_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ cam_ids,
                                                               const unsigned char* __restrict__ anchor, int* __restrict__ scratch, int n_cam,
                                                               long long frame_bytes, int tau) {
  __shared__ int wave_sums[4];
  const long long i = blockIdx.y;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;  // (the whole workgroup: nothing waits at the barrier)
  const long long nv = frame_bytes / (long long)sizeof(V);
  const V* __restrict__ f = reinterpret_cast<const V*>(frames + i * frame_bytes);
  const V* __restrict__ a = reinterpret_cast<const V*>(anchor + (long long)c * frame_bytes);
  const long long e0 = (long long)blockIdx.x * FRAME_CHUNK + threadIdx.x;
  V vf[FRAME_UNROLL] = {}, va[FRAME_UNROLL] = {};  // (behind the frame's end both stay zero: no byte differs)
#pragma unroll
  for (int u = 0; u < FRAME_UNROLL; ++u) {
    const long long e = e0 + u * 256;
    if (e < nv) {
      vf[u] = f[e];
      va[u] = a[e];
    }
  }
  int n = 0;
#pragma unroll
  for (int u = 0; u < FRAME_UNROLL; ++u) n += gate_changed_bytes(vf[u], va[u], tau);
  n = gate_block_sum(n, wave_sums);
  if (threadIdx.x == 0) scratch[i * gridDim.x + blockIdx.x] = n;
}

// (b) workgroup i: n = the sum of row i's partials, steps 2 and 3 of the rule on the camera's state row {still, epoch, changed,
// peak}, and the verdict (1: the frame moves, the anchor is to be replaced) where partial 0 was
__global__ __launch_bounds__(256) void frame_gate_decide_kernel(const int* __restrict__ cam_ids, int* __restrict__ state, int* __restrict__ scratch,
                                                                int n_cam, int chunks, int limit) {
  __shared__ int wave_sums[4];
  const long long i = blockIdx.x;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;
  int* __restrict__ part = scratch + i * chunks;
  int n = 0;
  for (int p = threadIdx.x; p < chunks; p += 256) n += part[p];
  n = gate_block_sum(n, wave_sums);  // (its barrier stands between every read of the partials and the store of the verdict)
  if (threadIdx.x != 0) return;
  int* __restrict__ st = state + (long long)c * 4;
  const int still = st[0];
  const bool moves = still < 0 || n > limit;
  if (moves) {
    st[0] = 0;
    st[1] = (int)((unsigned)st[1] + 1u);
    st[2] = still < 0 ? -1 : n;
    st[3] = 0;
  } else {
    st[0] = min(still + 1, GATE_STILL_MAX);
    st[2] = n;
    st[3] = max(st[3], n);
  }
  part[0] = moves;
}

// (c) frame_ring_push_kernel's copy, frame i -> the anchor of its camera, where the row's verdict says so
template <typename V>
__global__ __launch_bounds__(256) void frame_gate_anchor_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ cam_ids,
                                                                unsigned char* __restrict__ anchor, const int* __restrict__ scratch, int n_cam,
                                                                long long frame_bytes) {
  const long long i = blockIdx.y;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;
  if (!scratch[i * gridDim.x]) return;
  frame_copy_chunk<V>(frames + i * frame_bytes, anchor + (long long)c * frame_bytes, frame_bytes);
}

// One wavefront per row (i, k): the newest clip of camera c = cam_ids[i], crop k, again -- its C1 dwords from slot (count - 1) % W
// to slot count % W, every lane's loads of a round before its stores.  The count is only read here.
__global__ __launch_bounds__(64) void ring_repeat_kernel(const int* __restrict__ cam_ids, float* __restrict__ ring, const long long* __restrict__ counts,
                                                         int n_cam, int ncrops, int W, int C1) {
  const int i = blockIdx.x / ncrops, k = blockIdx.x % ncrops;
  const int c = cam_ids[i];
  if (c < 0 || c >= n_cam) return;
  const long long count = counts[c];
  if (count < 1) return;  // no clip to repeat
  const long long from = (count - 1) % W, to = count % W;
  if (from == to) return;  // W == 1: the clip lies where it belongs
  unsigned* __restrict__ row = (unsigned*)ring + ((long long)c * ncrops + k) * W * C1;
  const unsigned* __restrict__ s = row + from * C1;
  unsigned* __restrict__ d = row + to * C1;
  int j = threadIdx.x;
  for (; j + 64 * (RW_UNROLL - 1) < C1; j += 64 * RW_UNROLL) {
    unsigned r[RW_UNROLL];
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) r[u] = s[j + 64 * u];
#pragma unroll
    for (int u = 0; u < RW_UNROLL; ++u) d[j + 64 * u] = r[u];
  }
  for (; j < C1; j += 64) d[j] = s[j];
}

// ring_advance_kernel for cameras that hold a clip: a camera at count 0 has nothing to repeat and stays there
__global__ __launch_bounds__(256) void ring_repeat_advance_kernel(const int* __restrict__ cam_ids, long long* __restrict__ counts, int n, int n_cam) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c = cam_ids[i];
  if (c >= 0 && c < n_cam && counts[c] > 0) counts[c] += 1;  // ids are distinct: one thread per count
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_frame_gate_update_u8(const uint8_t* frames, const int32_t* cam_ids, uint8_t* anchor, int32_t* state, int32_t* scratch,
                                           int32_t n, int32_t n_cam, int64_t frame_bytes, int32_t pixel_delta, int32_t limit, void* stream) {
  ADVHIP_REQUIRE(frames && cam_ids && anchor && state && scratch, "frame_gate_update: null pointer");
  ADVHIP_REQUIRE(n > 0 && n_cam > 0 && frame_bytes > 0 && frame_bytes < (1ll << 31), "frame_gate_update: bad shape (n=%d n_cam=%d frame_bytes=%lld)", n,
                 n_cam, (long long)frame_bytes);
  ADVHIP_REQUIRE(n <= n_cam, "frame_gate_update: %d frames for %d cameras: one frame per camera and call (the scratch holds n_cam rows)", n, n_cam);
  ADVHIP_REQUIRE(pixel_delta >= 0 && pixel_delta <= 255, "frame_gate_update: pixel_delta %d outside [0, 255]", pixel_delta);
  ADVHIP_REQUIRE(limit >= 0 && limit <= frame_bytes, "frame_gate_update: limit %d outside [0, frame_bytes = %lld]", limit, (long long)frame_bytes);
  const char* who = "frame_gate_update";
  const int width = frame_access_bytes(frames, anchor, frame_bytes);
  const int chunks = (int)((frame_bytes / width + FRAME_CHUNK - 1) / FRAME_CHUNK);  // launch_frame_copy's, below
  int rc = launch_frame_copy(frames, anchor, frame_bytes, n, who, [&](auto v, dim3 grid) {
    hipLaunchKernelGGL(frame_gate_count_kernel<decltype(v)>, grid, dim3(256), 0, (hipStream_t)stream, frames, (const int*)cam_ids,
                       (const unsigned char*)anchor, (int*)scratch, (int)n_cam, (long long)frame_bytes, (int)pixel_delta);
  });
  if (rc != ADVHIP_OK) return rc;
  hipLaunchKernelGGL(frame_gate_decide_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, (const int*)cam_ids, (int*)state, (int*)scratch,
                     (int)n_cam, chunks, (int)limit);
  rc = check_launch("frame_gate_update (state)");
  if (rc != ADVHIP_OK) return rc;
  return launch_frame_copy(frames, anchor, frame_bytes, n, "frame_gate_update (anchor)", [&](auto v, dim3 grid) {
    hipLaunchKernelGGL(frame_gate_anchor_kernel<decltype(v)>, grid, dim3(256), 0, (hipStream_t)stream, frames, (const int*)cam_ids, anchor,
                       (const int*)scratch, (int)n_cam, (long long)frame_bytes);
  });
}

extern "C" int advhip_ring_repeat_f32(const int32_t* cam_ids, float* ring, int64_t* counts, int32_t n, int32_t n_cam, int32_t ncrops, int32_t W,
                                      int32_t C1, void* stream) {
  ADVHIP_REQUIRE(cam_ids && ring && counts, "ring_repeat: null pointer");
  ADVHIP_REQUIRE(n > 0 && n_cam > 0 && ncrops > 0 && W > 0 && C1 > 0, "ring_repeat: bad shape");
  const long long rows = (long long)n * ncrops;
  ADVHIP_REQUIRE(rows < (1ll << 31), "ring_repeat: %lld rows is outside the launch grid", rows);
  hipLaunchKernelGGL(ring_repeat_kernel, dim3((unsigned)rows), dim3(64), 0, (hipStream_t)stream, (const int*)cam_ids, ring, (const long long*)counts,
                     (int)n_cam, (int)ncrops, (int)W, (int)C1);
  const int rc = check_launch("ring_repeat");
  if (rc != ADVHIP_OK) return rc;
  hipLaunchKernelGGL(ring_repeat_advance_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const int*)cam_ids,
                     (long long*)counts, (int)n, (int)n_cam);
  return check_launch("ring_repeat (counts)");
}

extern "C" int advhip_frame_ring_push_u8(const uint8_t* frames, const int32_t* cam_ids, uint8_t* ring, int64_t* counts, int32_t n, int32_t n_cam,
                                         int32_t R, int64_t frame_bytes, void* stream) {
  ADVHIP_REQUIRE(frames && cam_ids && ring && counts, "frame_ring_push: null pointer");
  ADVHIP_REQUIRE(n > 0 && n_cam > 0 && R > 0 && frame_bytes > 0, "frame_ring_push: bad shape (n=%d n_cam=%d R=%d frame_bytes=%lld)", n, n_cam, R,
                 (long long)frame_bytes);
  const int rc = launch_frame_copy(frames, ring, frame_bytes, n, "frame_ring_push", [&](auto v, dim3 grid) {
    hipLaunchKernelGGL(frame_ring_push_kernel<decltype(v)>, grid, dim3(256), 0, (hipStream_t)stream, frames, (const int*)cam_ids, ring,
                       (const long long*)counts, (int)n_cam, (int)R, (long long)frame_bytes);
  });
  if (rc != ADVHIP_OK) return rc;
  return launch_ring_advance(cam_ids, counts, n, n_cam, stream, "frame_ring_push (counts)");
}

extern "C" int advhip_frame_ring_windows_u8(const uint8_t* ring, const int64_t* counts, const int32_t* cam_ids, uint8_t* dst, int32_t nb,
                                            int32_t n_cam, int32_t R, int64_t frame_bytes, int32_t frames_per_clip, int32_t frame_step,
                                            void* stream) {
  ADVHIP_REQUIRE(ring && counts && cam_ids && dst, "frame_ring_windows: null pointer");
  ADVHIP_REQUIRE(nb > 0 && n_cam > 0 && R > 0 && frame_bytes > 0 && frames_per_clip > 0 && frame_step > 0,
                 "frame_ring_windows: bad shape (nb=%d n_cam=%d R=%d frame_bytes=%lld frames_per_clip=%d frame_step=%d)", nb, n_cam, R,
                 (long long)frame_bytes, frames_per_clip, frame_step);
  ADVHIP_REQUIRE((long long)frames_per_clip * frame_step == R, "frame_ring_windows: R=%d is not frames_per_clip * frame_step = %d * %d", R,
                 frames_per_clip, frame_step);
  return launch_frame_copy(ring, dst, frame_bytes, (long long)nb * frames_per_clip, "frame_ring_windows", [&](auto v, dim3 grid) {
    hipLaunchKernelGGL(frame_ring_windows_kernel<decltype(v)>, grid, dim3(256), 0, (hipStream_t)stream, ring, (const long long*)counts,
                       (const int*)cam_ids, dst, (int)n_cam, (int)R, (long long)frame_bytes, (int)frames_per_clip, (int)frame_step);
  });
}

extern "C" int advhip_ring_push_f32(const float* feats, const int32_t* cam_ids, float* ring, int64_t* counts, int32_t n, int32_t n_cam,
                                    int32_t ncrops, int32_t W, int32_t C, void* stream) {
  ADVHIP_REQUIRE(feats && cam_ids && ring && counts, "ring_push: null pointer");
  ADVHIP_REQUIRE(n > 0 && n_cam > 0 && ncrops > 0 && W > 0 && C > 0, "ring_push: bad shape");
  ADVHIP_REQUIRE(C <= PW_MAX_C, "ring_push: C=%d above %d: numpy sums in chunks of %d elements, the order of its adds changes there", C,
                 PW_MAX_C, PW_MAX_C);
  const long long rows = (long long)n * ncrops;
  ADVHIP_REQUIRE(rows < (1ll << 31), "ring_push: %lld rows is outside the launch grid", rows);
  const PwLeaves& tab = pw_leaves(C);
  hipLaunchKernelGGL(ring_push_kernel, dim3((unsigned)rows), dim3(64), pw_lds_bytes(C, tab), (hipStream_t)stream, feats, (const int*)cam_ids, ring,
                     (const long long*)counts, (int)n_cam, (int)ncrops, (int)W, (int)C, tab);
  const int rc = check_launch("ring_push");
  if (rc != ADVHIP_OK) return rc;
  return launch_ring_advance(cam_ids, counts, n, n_cam, stream, "ring_push (counts)");
}

extern "C" int advhip_ring_windows_f32(const float* ring, const int64_t* counts, const int32_t* cam_ids, float* dst, int32_t nb, int32_t n_cam,
                                       int32_t ncrops, int32_t W, int32_t Tmax, int32_t C1, void* stream) {
  ADVHIP_REQUIRE(ring && counts && cam_ids && dst, "ring_windows: null pointer");
  ADVHIP_REQUIRE(nb > 0 && n_cam > 0 && ncrops > 0 && W > 0 && Tmax > 0 && C1 > 0, "ring_windows: bad shape");
  const long long rows = (long long)nb * ncrops * Tmax;
  ADVHIP_REQUIRE(rows < (1ll << 31), "ring_windows: %lld rows is outside the launch grid", rows);
  hipLaunchKernelGGL(ring_windows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, ring, (const long long*)counts,
                     (const int*)cam_ids, dst, (int)n_cam, (int)ncrops, (int)W, (int)Tmax, (int)C1);
  return check_launch("ring_windows");
}

extern "C" int advhip_crop_mean_last_f32(const float* scores, const int32_t* lens, const int32_t* cam_ids, float* latest, int32_t nb,
                                         int32_t ncrops, int32_t Tmax, void* stream) {
  ADVHIP_REQUIRE(scores && lens && cam_ids && latest, "crop_mean_last: null pointer");
  ADVHIP_REQUIRE(nb > 0 && ncrops > 0 && Tmax > 0, "crop_mean_last: bad shape");
  hipLaunchKernelGGL(crop_mean_last_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, (hipStream_t)stream, scores, (const int*)lens,
                     (const int*)cam_ids, latest, (int)nb, (int)ncrops, (int)Tmax);
  return check_launch("crop_mean_last");
}
