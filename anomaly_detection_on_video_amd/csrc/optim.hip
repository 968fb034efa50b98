// The optimizer step of the scorer's training loop on many parameter tensors at once: Adam (advhip_adam_multi_f32,
// advhip_adam_multi_dev_f32) and the global gradient-norm clip in front of it (advhip_grad_norm_multi_f32).
// All reductions are deterministic (fixed-order partial sums, no atomics).
#include <algorithm>
#include <cmath>

#include "common.h"

using namespace advhip;

// ---- Adam with L2-in-gradient weight decay over many parameter tensors in one launch (torch.optim.Adam's update rule,
// the reference's src/runner.py:53-59; torch/optim/adam.py) ----------------------------------------------------------------
//   g' = g + wd * p;  m = m + (1 - b1) (g' - m);  v = b2 v + (1 - b2) g'^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// t = *step (a device-side counter the caller has already incremented for this step; fp32 as torch's capturable Adam keeps it).
// The item table travels in the kernel arguments (a launch inside a captured HIP graph replays it as is); a workgroup finds its
// item by a scalar scan and updates ADAM_PER_BLOCK consecutive elements of it, 16 bytes per lane and access.
constexpr int ADAM_MAX_ITEMS = 80, ADAM_PER_BLOCK = 4096;
struct AdamItem {
  float* p;
  const float* g;
  float* m;
  float* v;
  const float* step;
  int n;
  int block_begin;
};
struct AdamArgs {
  AdamItem it[ADAM_MAX_ITEMS];
  int n;
  double lr, b1, b2;  // (doubles: 1 - beta and lr / (1 - beta^t) are formed in double and rounded once, as torch does in Python)
  float eps, wd;
};
// The update of one workgroup's ADAM_PER_BLOCK elements, shared by the by-value launch and the device-scalar one.  SCALED: every
// gradient element is first multiplied by `scale` as ONE separately rounded fp32 product (torch's in-place `g.mul_(coef)`;
// __fmul_rn is never contracted into the weight-decay FMA behind it); what follows is the same instruction sequence either way.
template <bool SCALED>
__device__ __forceinline__ void adam_update_block(const AdamArgs& aa, const double lr, const float scale) {
  int i = 0;
  while (i + 1 < aa.n && (int)blockIdx.x >= aa.it[i + 1].block_begin) ++i;
  const AdamItem& t = aa.it[i];
  const int base = ((int)blockIdx.x - t.block_begin) * ADAM_PER_BLOCK;
  const double st = (double)*t.step;
  const float step_size = (float)(lr / (1.0 - pow(aa.b1, st)));
  const float bc2_sqrt = (float)sqrt(1.0 - pow(aa.b2, st));
  const float omb1 = (float)(1.0 - aa.b1), b2 = (float)aa.b2, omb2 = (float)(1.0 - aa.b2), eps = aa.eps, wd = aa.wd;
  auto upd = [&](float& p, float g, float& m, float& v) {
    if constexpr (SCALED) g = __fmul_rn(g, scale);
    g = g + wd * p;
    m = m + omb1 * (g - m);
    v = b2 * v + omb2 * g * g;
    p = p - step_size * m / (sqrtf(v) / bc2_sqrt + eps);
  };
  const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0);
#pragma unroll
  for (int u = 0; u < ADAM_PER_BLOCK / 1024; ++u) {
    const int e = base + u * 1024 + (int)threadIdx.x * 4;
    if (e >= t.n) break;
    if (vec && e + 4 <= t.n) {
      float4 p = *reinterpret_cast<const float4*>(t.p + e), m = *reinterpret_cast<const float4*>(t.m + e), v = *reinterpret_cast<const float4*>(t.v + e);
      const float4 g = *reinterpret_cast<const float4*>(t.g + e);
      upd(p.x, g.x, m.x, v.x); upd(p.y, g.y, m.y, v.y); upd(p.z, g.z, m.z, v.z); upd(p.w, g.w, m.w, v.w);
      *reinterpret_cast<float4*>(t.p + e) = p;
      *reinterpret_cast<float4*>(t.m + e) = m;
      *reinterpret_cast<float4*>(t.v + e) = v;
    } else {
      for (int k = e; k < e + 4 && k < t.n; ++k) {
        float p = t.p[k], m = t.m[k], v = t.v[k];
        upd(p, t.g[k], m, v);
        t.p[k] = p; t.m[k] = m; t.v[k] = v;
      }
    }
  }
}
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamArgs aa) { adam_update_block<false>(aa, aa.lr, 1.0f); }
// lr (a double: lr / (1 - b1^t) is still formed in double and rounded once) and the gradient scale are read from device memory, so
// a captured launch sees the values of the replay, not of the capture.  Both loads are uniform: one scalar load per workgroup.
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(const AdamArgs aa, const double* __restrict__ lr_dev, const float* __restrict__ scale_dev) {
  const double lr = *lr_dev;
  if (scale_dev) adam_update_block<true>(aa, lr, *scale_dev);
  else adam_update_block<false>(aa, lr, 1.0f);
}

static int adam_multi_launch(const char* what, const advhip_adam_item* items, int32_t n_items, double lr, const double* lr_dev, const float* scale_dev,
                             double beta1, double beta2, double eps, double weight_decay, void* stream) {
  ADVHIP_REQUIRE(items && n_items > 0, "%s: bad arguments", what);
  ADVHIP_REQUIRE(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0. && weight_decay >= 0.,
                 "%s: bad hyper-parameters (lr %g, betas %g %g, eps %g, weight_decay %g)", what, lr, beta1, beta2, eps, weight_decay);
  for (int base = 0; base < n_items; base += ADAM_MAX_ITEMS) {
    AdamArgs aa;
    aa.n = std::min(ADAM_MAX_ITEMS, n_items - base);
    aa.lr = lr; aa.b1 = beta1; aa.b2 = beta2; aa.eps = (float)eps; aa.wd = (float)weight_decay;
    long long blocks = 0;
    for (int i = 0; i < aa.n; ++i) {
      const advhip_adam_item& s = items[base + i];
      ADVHIP_REQUIRE(s.param && s.grad && s.exp_avg && s.exp_avg_sq && s.step && s.n > 0 && s.n < (1ll << 31), "%s: item %d: bad arguments", what, base + i);
      aa.it[i] = AdamItem{s.param, s.grad, s.exp_avg, s.exp_avg_sq, s.step, (int)s.n, (int)blocks};
      blocks += (s.n + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK;
      ADVHIP_REQUIRE(blocks < (1ll << 31), "%s: too many elements", what);
    }
    for (int i = aa.n; i < ADAM_MAX_ITEMS; ++i) aa.it[i] = AdamItem{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0x7FFFFFFF};
    if (lr_dev) hipLaunchKernelGGL(adam_multi_dev_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, aa, lr_dev, scale_dev);
    else hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, aa);
    if (int rc = check_launch(what)) return rc;
  }
  return ADVHIP_OK;
}

extern "C" int advhip_adam_multi_f32(const advhip_adam_item* items, int32_t n_items, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, void* stream) {
  return adam_multi_launch("adam_multi", items, n_items, lr, nullptr, nullptr, beta1, beta2, eps, weight_decay, stream);
}

extern "C" int advhip_adam_multi_dev_f32(const advhip_adam_item* items, int32_t n_items, const double* lr_dev, const float* grad_scale_dev, double beta1,
                                         double beta2, double eps, double weight_decay, void* stream) {
  ADVHIP_REQUIRE(lr_dev, "adam_multi_dev: lr_dev is null");
  return adam_multi_launch("adam_multi_dev", items, n_items, 0., lr_dev, grad_scale_dev, beta1, beta2, eps, weight_decay, stream);
}

// ---- global L2 norm of many gradient tensors and the clip factor (torch.nn.utils.clip_grad_norm_), for advhip_adam_multi_dev_f32 ----
// Stage 1: one workgroup per NORM_PER_BLOCK consecutive elements of one tensor (found by the scalar scan Adam uses, in two strides): every lane adds
// the squares of its elements, formed in double, in index order; the 64 lanes of a wave are added by a shuffle tree, the four waves in
// wave order; the sum goes to partials[first + blockIdx.x].  Stage 2: ONE workgroup adds the partials -- lane l takes l, l + 256, ...
// in that order, then the same tree -- and writes the norm and the factor.  Every order is fixed and no atomic is used: same bits
// every run.
constexpr int NORM_MAX_ITEMS = 240, NORM_PER_BLOCK = 4096;
struct NormItem {
  const float* g;
  int n;
  int block_begin;
};
struct NormArgs {
  NormItem it[NORM_MAX_ITEMS];
  int n;
  double* partials;  // (this launch's first slot)
};
__device__ __forceinline__ double block_sum_256(double s, double* lds4) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];  // (read by every lane; lane 0's copy is the one stored)
}
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const NormArgs na) {
  __shared__ double lds4[4];
  // the scalar scan of the Adam launch in two strides (16 items, then 1): every step is a dependent scalar load, and a table of 240
  // items scanned one by one costs the late workgroups more than their 16 KiB of gradient
  int i = 0;
  while (i + 16 < na.n && (int)blockIdx.x >= na.it[i + 16].block_begin) i += 16;
  while (i + 1 < na.n && (int)blockIdx.x >= na.it[i + 1].block_begin) ++i;
  const NormItem& t = na.it[i];
  const int base = ((int)blockIdx.x - t.block_begin) * NORM_PER_BLOCK;
  const bool vec = (((uintptr_t)t.g & 15) == 0);
  double s = 0.0;
  auto add4 = [&](const float4 g) {
    s += (double)g.x * (double)g.x; s += (double)g.y * (double)g.y; s += (double)g.z * (double)g.z; s += (double)g.w * (double)g.w;
  };
  if (vec && base + NORM_PER_BLOCK <= t.n) {
    // a whole block of an aligned tensor: the four loads are issued together, the sum keeps the order of the general path below
    const float4* g4 = reinterpret_cast<const float4*>(t.g + base) + threadIdx.x;
    const float4 g0 = g4[0], g1 = g4[256], g2 = g4[512], g3 = g4[768];
    add4(g0); add4(g1); add4(g2); add4(g3);
  } else {
#pragma unroll
    for (int u = 0; u < NORM_PER_BLOCK / 1024; ++u) {
      const int e = base + u * 1024 + (int)threadIdx.x * 4;
      if (e < t.n) {
        if (vec && e + 4 <= t.n) {
          add4(*reinterpret_cast<const float4*>(t.g + e));
        } else {
          for (int k = e; k < e + 4 && k < t.n; ++k) s += (double)t.g[k] * (double)t.g[k];
        }
      }
    }
  }
  s = block_sum_256(s, lds4);
  if (threadIdx.x == 0) na.partials[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partials, long long n, float max_norm, float* __restrict__ norm_out,
                                                               float* __restrict__ scale_out) {
  __shared__ double lds4[4];
  double s = 0.0;
  for (long long k = threadIdx.x; k < n; k += 256) s += partials[k];
  s = block_sum_256(s, lds4);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    // torch: clamp(max_norm / (norm + 1e-6), max=1.0) on an fp32 tensor; `number / tensor` is tensor.reciprocal() * number there
    const float coef = __fmul_rn(__fdiv_rn(1.0f, __fadd_rn(norm, 1e-6f)), max_norm);
    *norm_out = norm;
    *scale_out = coef > 1.0f ? 1.0f : coef;  // (a NaN fails the comparison and stays, as under torch.clamp)
  }
}

extern "C" int advhip_grad_norm_multi_f32(const advhip_norm_item* items, int32_t n_items, double max_norm, double* partials, int64_t n_partials,
                                          float* norm_out, float* scale_out, void* stream) {
  ADVHIP_REQUIRE(items && n_items > 0 && partials && norm_out && scale_out, "grad_norm_multi: bad arguments");
  ADVHIP_REQUIRE(max_norm > 0. && std::isfinite(max_norm), "grad_norm_multi: max_norm %g is not a finite number > 0", max_norm);
  long long total = 0;  // (every item is checked, and the partials' room, before the first launch)
  for (int i = 0; i < n_items; ++i) {
    ADVHIP_REQUIRE(items[i].grad && items[i].n > 0 && items[i].n < (1ll << 31), "grad_norm_multi: item %d: bad arguments", i);
    total += (items[i].n + NORM_PER_BLOCK - 1) / NORM_PER_BLOCK;
  }
  ADVHIP_REQUIRE(total <= n_partials, "grad_norm_multi: %lld partial sums needed, room for %lld", total, (long long)n_partials);
  long long first = 0;
  for (int base = 0; base < n_items; base += NORM_MAX_ITEMS) {
    NormArgs na;
    na.n = std::min(NORM_MAX_ITEMS, n_items - base);
    na.partials = partials + first;
    long long blocks = 0;
    for (int i = 0; i < na.n; ++i) {
      const advhip_norm_item& s = items[base + i];
      na.it[i] = NormItem{s.grad, (int)s.n, (int)blocks};
      blocks += (s.n + NORM_PER_BLOCK - 1) / NORM_PER_BLOCK;
      ADVHIP_REQUIRE(blocks < (1ll << 31), "grad_norm_multi: too many elements");
    }
    for (int i = na.n; i < NORM_MAX_ITEMS; ++i) na.it[i] = NormItem{nullptr, 0, 0x7FFFFFFF};
    hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, na);
    if (int rc = check_launch("grad_norm_multi")) return rc;
    first += blocks;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, total, (float)max_norm, norm_out, scale_out);
  return check_launch("grad_norm_finish");
}
