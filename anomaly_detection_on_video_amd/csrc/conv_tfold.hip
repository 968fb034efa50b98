// The temporal fold (ADVHIP_ALGO_TFOLD_BASE, include/advhip.h): a (kt,1,1) stride-1 conv with centred padding pt = kt/2 on
// T <= pt + 1 frames joins every (output frame t, input frame ti) pair by exactly one tap, dt = ti - t + pt, so
//   y[b, n, t, p] = sum_ci sum_ti W[n, ci, ti - t + pt] x[b, ci, ti, p]
// is a dense 1x1x1 conv on the SAME memory seen as (B, Cin*T, 1, H, W) -> (B, Cout*T, 1, H, W): channel k' = ci*T + ti in,
// n' = n*T + t out.  No tap lies in the zero padding any more: T*T MACs per position instead of kt*T (the I3D layers 2-4 run
// their temporal convs on T = 2 frames with kt = 3: 4 instead of 6).  This file holds the one statement of the applicability
// rule and the shape arithmetic (advhip_conv3d_tfold_desc) and the load-time operands; the launch itself is the ordinary
// unchecked 1x1x1 path of conv_igemm.hip on the folded descriptor.
#include <algorithm>

#include "common.h"

namespace advhip {

// w (Cout, Cin, kt, 1, 1) -> wf [Kpad'][Cout*T], wf[ci*T + ti][n*T + t] = w[n][ci][ti - t + pt], zero rows above Cin*T.
// One thread per output element (consecutive threads = consecutive columns: coalesced stores; the loads stride by Cin*kt, once
// per set of weights).
__global__ void pack_weight_tfold_kernel(const float* __restrict__ w, float* __restrict__ wf, int Cin, int kt, int pt, int T, int K,
                                         int Kpad, int N) {
  const long long total = (long long)Kpad * N;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i / N), n2 = (int)(i - (long long)k * N);
    float v = 0.f;
    if (k < K) {
      const int ci = k / T, ti = k - ci * T;
      const int n = n2 / T, t = n2 - n * T;
      const int dt = ti - t + pt;  // in [0, kt): |ti - t| <= T - 1 <= pt
      v = w[((long long)n * Cin + ci) * kt + dt];
    }
    wf[i] = v;
  }
}

__global__ void expand_scale_shift_tfold_kernel(const float* __restrict__ scale, const float* __restrict__ shift,
                                                float* __restrict__ scale_f, float* __restrict__ shift_f, int T, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) {
    scale_f[i] = scale[i / T];
    shift_f[i] = shift[i / T];
  }
}

}  // namespace advhip

using namespace advhip;

extern "C" int advhip_conv3d_tfold_desc(const advhip_conv3d_desc* d, advhip_conv3d_desc* folded) {
  if (int rc = advhip_conv3d_out_dims(d, nullptr, nullptr, nullptr)) return rc;
  ADVHIP_REQUIRE(folded != nullptr, "conv3d: ADVHIP_ALGO_TFOLD: null folded descriptor");
  ADVHIP_REQUIRE(d->kh == 1 && d->kw == 1 && d->ph == 0 && d->pw == 0,
                 "conv3d: ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs a (kt,1,1) conv without spatial padding (k=%d,%d,%d, p=%d,%d,%d)", d->kt, d->kh, d->kw, d->pt,
                 d->ph, d->pw);
  ADVHIP_REQUIRE(d->st == 1 && d->sh == 1 && d->sw == 1, "conv3d: ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs stride 1 (s=%d,%d,%d)", d->st, d->sh, d->sw);
  ADVHIP_REQUIRE(2 * d->pt + 1 == d->kt, "conv3d: ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs the centred padding pt = kt/2 of an odd kt (kt=%d, pt=%d)", d->kt, d->pt);
  ADVHIP_REQUIRE(d->T <= d->pt + 1, "conv3d: ADVHIP_ALGO_TFOLD is not instantiated for this conv: it needs T <= pt + 1 frames, one tap per (output, input) frame pair (T=%d, pt=%d)",
                 d->T, d->pt);
  ADVHIP_REQUIRE((long long)d->Cin * d->T < (1ll << 31) && (long long)d->Cout * d->T < (1ll << 31), "conv3d: ADVHIP_ALGO_TFOLD: folded channels overflow");
  int algo = d->algo;
  if (algo >= ADVHIP_ALGO_TFOLD_BASE && algo < ADVHIP_ALGO_TFOLD_BASE + 16) {
    const int tile = algo - ADVHIP_ALGO_TFOLD_BASE;
    ADVHIP_REQUIRE(tile >= 1 && tile <= 9 && tile != 5, "conv3d: algo %d is not instantiated in this library (ADVHIP_ALGO_TFOLD_BASE + tile id 1..4, 6..9 of the 2-deep LDS-DMA family)", d->algo);
    algo = ADVHIP_ALGO_DMA2_BASE + tile;
  }
  advhip_conv3d_desc f = *d;
  f.Cin = d->Cin * d->T;
  f.Cout = d->Cout * d->T;
  f.T = 1;
  f.kt = 1;
  f.pt = 0;
  f.algo = algo;
  *folded = f;
  return ADVHIP_OK;
}

extern "C" int advhip_conv3d_pack_weight_tfold_f32(const advhip_conv3d_desc* d, const float* w, float* w_folded, void* stream) {
  advhip_conv3d_desc f;
  if (int rc = advhip_conv3d_tfold_desc(d, &f)) return rc;
  ADVHIP_REQUIRE(w && w_folded, "pack_weight_tfold: null pointer");
  const int K = f.Cin, Kpad = advhip_conv3d_packed_rows(&f);
  if (Kpad < 0) return Kpad;
  const long long total = (long long)Kpad * f.Cout;
  const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(pack_weight_tfold_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, w, w_folded, d->Cin, d->kt, d->pt, d->T, K, Kpad, f.Cout);
  return check_launch("pack_weight_tfold");
}

extern "C" int advhip_conv3d_tfold_scale_shift_f32(const advhip_conv3d_desc* d, const float* scale, const float* shift, float* scale_folded,
                                                   float* shift_folded, void* stream) {
  advhip_conv3d_desc f;
  if (int rc = advhip_conv3d_tfold_desc(d, &f)) return rc;
  ADVHIP_REQUIRE(scale && shift && scale_folded && shift_folded, "tfold_scale_shift: null pointer");
  hipLaunchKernelGGL(expand_scale_shift_tfold_kernel, dim3((f.Cout + 255) / 256), dim3(256), 0, (hipStream_t)stream, scale, shift, scale_folded,
                     shift_folded, d->T, f.Cout);
  return check_launch("tfold_scale_shift");
}
