/*
 * advhip.h -- C ABI of libadvhip.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the
 * I3D-ResNet50 feature-extraction + MGFN MIL-scoring hot path of
 * jinmang2/anomaly_detection_on_video.
 *
 * The reference has no FFI: its hot path calls torch.nn modules.  Each entry point below names
 * the reference call site(s) it replaces (paths relative to /root/reference).  INTEGRATION.md
 * shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - all tensors are fp32, contiguous, channels-first (NCDHW / NCT) device pointers owned by
 *     the caller; nothing is allocated, freed or synchronised inside a call (graph-capturable)
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); launches are asynchronous
 *   - return value: 0 on success, a negative ADVHIP_E* code otherwise; no exceptions cross the
 *     ABI; advhip_last_error() returns a thread-local message for the last failure
 *   - no global mutable state besides that message: thread-compatible, one process per GPU
 */
#ifndef ADVHIP_H
#define ADVHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADVHIP_ABI_VERSION 2

#define ADVHIP_OK 0
#define ADVHIP_EINVAL (-1)   /* bad shape / null pointer / unsupported configuration */
#define ADVHIP_ELAUNCH (-2)  /* hipLaunch failed (message has hipGetErrorString) */
#define ADVHIP_ERANGE (-3)   /* tensor too large for 32-bit element indexing */

/* conv algorithm selector (advhip_conv3d_desc.algo) */
#define ADVHIP_ALGO_AUTO 0
#define ADVHIP_ALGO_IGEMM_128x128 1 /* generic implicit GEMM, 128(M) x 128(N) block tile */
#define ADVHIP_ALGO_IGEMM_128x64 2
#define ADVHIP_ALGO_IGEMM_64x64 3
#define ADVHIP_ALGO_IGEMM_64x128 4
#define ADVHIP_ALGO_IGEMM_128x128x32 5 /* same tiles, 32-deep k-tile (longer MFMA run per barrier) */
#define ADVHIP_ALGO_IGEMM_128x64x32 6
#define ADVHIP_ALGO_IGEMM_64x64x32 7
#define ADVHIP_ALGO_IGEMM_64x128x32 8
#define ADVHIP_ALGO_IGEMM_256x64 9 /* 256(M) x 64(N) x 16: four waves stacked along M (64 x 64 wave tiles); ADVHIP_ALGO_DMA2_BASE only */
/* + tile id 1..8: same tiles, gather arithmetic hoisted to scalar offsets + coordinate bit-mask (kernel <= 10^3) */
#define ADVHIP_ALGO_FAST_BASE 32
/* + tile id: the fast gather with LDS-DMA operand staging into a 3-deep ring (no 128x128x32) */
#define ADVHIP_ALGO_DMA_BASE 64
/* + tile id 2..4: the same with a 4-deep ring (three k-tiles in flight) */
#define ADVHIP_ALGO_DMA4_BASE 96
/* + tile id 5 (128x128x32) or 6 (128x64x32): OPT-IN split-bf16 arithmetic -- every fp32 operand as two bf16 terms,
 * three bf16 MFMAs (hi*hi + hi*lo + lo*hi) accumulated in fp32: 3/16 of the fp32 MFMA cycles, agreement with the
 * fp32 kernels ~1e-5 relative (inside the 1e-3 contract, not bit-comparable).  Takes the weights from
 * advhip_conv3d_pack_weight_bf16x3 instead of advhip_conv3d_pack_weight_f32.  Never chosen by ADVHIP_ALGO_AUTO. */
#define ADVHIP_ALGO_BF16X3_BASE 128
/* + tile id 1..4, 6..9: the LDS-DMA kernel with a 2-deep ring (one k-tile in flight): 16 KiB of LDS per 64x64x16
 * workgroup instead of 24 -> 8 resident workgroups per CU instead of 6 */
#define ADVHIP_ALGO_DMA2_BASE 160
/* the 2-deep LDS-DMA kernel, 128x64x16 tile, with m-tiles that span T (2 or 4 frames x 64 / 32 flattened spatial positions)
 * for (kt,1,1) stride-1 "same" convs: the temporal taps of a tile re-read the same activation rows from L1/L2 instead of
 * three far-apart tiles fetching them from HBM.  Unsplit; T even. */
#define ADVHIP_ALGO_TSPAN_128x64 192
/* the 2-deep LDS-DMA kernel for unsplit 1x1x1 stride-1 convs on 16-byte aligned rows, 128x64x16 tiles, with the last m-tile rows cut
 * into 64x64 tiles when the 128x64 tiles number a little more than a whole number of rounds of resident workgroups (6 per compute
 * unit): every workgroup of the last, partial round is then a short one.  Same K order per output as the plain tiles: bit-identical
 * results.  Launches below one round / on a round boundary are the plain 128x64 launch. */
#define ADVHIP_ALGO_MIXED_128x64 200
/* + tile id 1..4, 6..9 (those of ADVHIP_ALGO_DMA2_BASE): the TEMPORAL FOLD.  A (kt,1,1) stride-1 conv with padding pt = kt/2 on
 * T <= pt + 1 frames joins every (output frame t, input frame ti) pair by exactly one tap, dt = ti - t + pt, so it IS the dense
 * 1x1x1 conv (B, Cin*T, 1, H, W) -> Cout*T on the same memory (channel ci*T + ti in, n*T + t out) with the weights
 * W'[n*T + t][ci*T + ti] = W[n][ci][ti - t + pt]: T*T MACs per position instead of kt*T, none of them on the zero padding, the
 * input read once instead of once per tap, no gather mask.  The launch is ADVHIP_ALGO_DMA2_BASE + tile id on the descriptor of
 * advhip_conv3d_tfold_desc with the same `splits`; x, y, residual and the batch strides are the caller's own (a channel slice of
 * a wider buffer is still dense within a sample under the folded view); w_packed, ktab, scale and shift are the FOLDED operands
 * (advhip_conv3d_pack_weight_tfold_f32, advhip_conv3d_build_ktab on the folded descriptor, advhip_conv3d_tfold_scale_shift_f32).
 * Same non-zero terms per output in the same order (ci major, dt ascending).  No LayerNorm fold, no avgpool_out.  Never chosen
 * by ADVHIP_ALGO_AUTO. */
#define ADVHIP_ALGO_TFOLD_BASE 208
/* + tile id (ADVHIP_ALGO_IGEMM_128x64 or _64x64) + 8 * (W - 1), W = 1..3 workgroups per compute unit: a PERSISTENT, wave-specialised
 * kernel for unsplit 1x1x1 stride-1 convs on 16-byte aligned rows with K >= 64 (the `conv3` + residual launches,
 * src/i3d.py:85-89, 108-121): eight-wave workgroups that stay for the whole launch and walk a share of the output tiles; four waves
 * only multiply, four fetch the operands (plain loads -> registers -> a two-stage LDS ring, four k-tiles ahead, across tile
 * boundaries) and run the epilogue of the previous tile beside the next tile's MFMAs.  Same k order and accumulation chain as the
 * other families: bit-identical results.  No LayerNorm fold / GELU-backward operand.  OPT-IN and never chosen by ADVHIP_ALGO_AUTO
 * or the tuned table: measured slower than the one-tile kernels on the B = 32 plan (profiles/r04_persist_kernel_study.md). */
#define ADVHIP_ALGO_PERSIST_BASE 224
/* advhip_conv3d_s2w_bn_relu_maxpool233_f32 (and its workspace size) only: the stem launch SPLIT BY POOL WINDOW IN T.  The pool
 * windows whose two output frames have no temporal tap in the padding run the 2(t) x 4(h) x 16(w) bricks as before; the window at
 * either end of the clip runs frame by frame on 1(t) x 8(h) x 16(w) tiles, where a k-tile whose rows all carry a padded temporal
 * tap is padding for the whole workgroup and is skipped (fill, barrier, fragment reads, MFMAs): 23 of the 368 k-tiles of a sample
 * column at T = 16.  The max over such a window's two frames moves to the merge launch.  Whole k-tiles are skipped and K keeps
 * its order: every output sees the same non-zero terms in the same order, bit-identical results (for finite weights: a skipped
 * product is 0 * w).  Applies to kt = 5, pt = 2, st = 2, an even output T and an even number of 4-row bricks along h; any other
 * geometry runs the single launch.  Any other algo value on that entry point: the single launch. */
#define ADVHIP_ALGO_STEM_BORDER 256
/* Kernel families, as advhip_conv3d_algo_info reports them (DMA3 is ADVHIP_ALGO_DMA_BASE's 3-deep ring). */
#define ADVHIP_FAMILY_GENERIC 0
#define ADVHIP_FAMILY_FAST 1
#define ADVHIP_FAMILY_DMA3 2
#define ADVHIP_FAMILY_DMA4 3
#define ADVHIP_FAMILY_BF16X3 4
#define ADVHIP_FAMILY_DMA2 5
#define ADVHIP_FAMILY_TSPAN 6
#define ADVHIP_FAMILY_MIXED 7
#define ADVHIP_FAMILY_PERSIST 8

typedef struct advhip_conv3d_desc {
  int32_t B, Cin, T, H, W;    /* input  (B, Cin, T, H, W) */
  int32_t Cout, kt, kh, kw;   /* weight (Cout, Cin, kt, kh, kw), bias-free */
  int32_t st, sh, sw;         /* stride */
  int32_t pt, ph, pw;         /* zero padding */
  int32_t relu;               /* activation applied last: 0 none, 1 ReLU max(0,.), 2 GELU (erf form, nn.GELU());
                               * advhip_conv3d_bn_act_ex_f32 only: 3 = GELU, with GELU'(pre-activation) -- not the pre-activation -- written to
                               * the epilogue's y_preact (what the backward pass multiplies by); 4 = no activation, the result multiplied by the
                               * epilogue's dact_z tensor AS IS (a tensor saved by a code-3 forward: the GELU backward without erf / exp) */
  int32_t algo;               /* ADVHIP_ALGO_* */
  int32_t splits;             /* split-K factor: 0 = heuristic, 1 = none, n = n K-slices + reduce pass */
} advhip_conv3d_desc;

/* --- library ------------------------------------------------------------------------------ */
int advhip_abi_version(void);
const char* advhip_last_error(void);
/* "gfx950" -- the only code object in the library */
const char* advhip_target_arch(void);

/* --- I3D backbone ---------------------------------------------------------------------------
 * Output extents of a conv / pool (floor mode), the torch formula. */
int advhip_conv3d_out_dims(const advhip_conv3d_desc* d, int32_t* To, int32_t* Ho, int32_t* Wo);

/* Rows of the packed weight matrix: K = Cin*kt*kh*kw rounded up to a multiple of 32. */
int advhip_conv3d_packed_rows(const advhip_conv3d_desc* d);

/* What an implicit-GEMM algorithm id means: its kernel family (ADVHIP_FAMILY_*) and its block tile BM x BN x BK (outputs may be
 * NULL).  ADVHIP_EINVAL ("not instantiated") for an id this library has no kernel for.  An ADVHIP_ALGO_TFOLD_BASE id reports
 * the ADVHIP_ALGO_DMA2_BASE kernel its folded launch runs, ADVHIP_ALGO_AUTO the LDS-DMA 64 x 64 x 16 kernel it prefers.  Host only. */
int advhip_conv3d_algo_info(int32_t algo, int32_t* family, int32_t* BM, int32_t* BN, int32_t* BK);

/* Pack torch-layout weights w[Cout][Cin][kt][kh][kw] into the kernels' [Kpad][Cout] layout
 * (row k = ((ci*kt+dt)*kh+dh)*kw+dw, zero rows above K).  Done once per layer at load time: the
 * load-time analogue of model.load_state_dict (src/i3d.py:356-359). */
int advhip_conv3d_pack_weight_f32(const advhip_conv3d_desc* d, const float* w, float* w_packed,
                                  void* stream);

/* Split torch-layout fp32 weights into the bf16 images of the ADVHIP_ALGO_BF16X3_* kernels:
 * w_split = uint16[2][Cout][Kpad] (hi image, then lo image; k contiguous, zero above K); 4*Cout*Kpad bytes. */
int advhip_conv3d_pack_weight_bf16x3(const advhip_conv3d_desc* d, const float* w, void* w_split, void* stream);

/* Per-row gather table for one input size (d->T, d->H, d->W):
 * ktab[k] = {input element offset of tap k relative to the window origin, dt, dh, dw}; rows
 * above K are marked out-of-range so they contribute exact zeros, followed by the fast kernels'
 * compact table {byte offset, tap bit}.  int32[Kpad][4] + int32[Kpad][2] = 6*Kpad int32. */
int advhip_conv3d_build_ktab(const advhip_conv3d_desc* d, int32_t* ktab, void* stream);

/* Fold eval-mode BatchNorm into per-channel scale/shift:
 *   scale = gamma / sqrt(var + eps), shift = beta - mean * scale.
 * Replaces nn.BatchNorm3d in eval mode (src/i3d.py:75,84,88,210,271). */
int advhip_bn_fold_f32(const float* gamma, const float* beta, const float* mean, const float* var,
                       float eps, int32_t C, float* scale, float* shift, void* stream);

/* y = act( conv3d(x, w) * scale[c] + shift[c] (+ residual) )  -- one fused launch.
 * Replaces the nn.Conv3d -> nn.BatchNorm3d -> (+=residual) -> nn.ReLU module sequences of
 * Bottleneck.forward (src/i3d.py:98-121), the stem (src/i3d.py:303-305) and the downsample
 * branch (src/i3d.py:262-272).  `residual` may be NULL; otherwise it has y's shape.
 * fp32 MFMA (v_mfma_f32_16x16x4_f32): exact fp32 products, fp32 accumulation.
 * `workspace`: caller-owned device scratch of at least advhip_conv3d_workspace_bytes(d) bytes
 * (0 unless the (pinned or heuristic) configuration uses split-K: partial-sum slabs that a second
 * launch reduces in a fixed order, so results stay run-to-run bit-identical). */
int64_t advhip_conv3d_workspace_bytes(const advhip_conv3d_desc* d);
int advhip_conv3d_bn_act_f32(const advhip_conv3d_desc* d, const float* x, const float* w_packed,
                             const int32_t* ktab, const float* scale, const float* shift,
                             const float* residual, float* y, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* The same with explicit batch strides (in elements; 0 = dense): x and/or y may be a channel slice of a wider NCDHW
 * tensor, e.g. one half of a concatenation buffer -- how the layer-1 downsample branch is folded into conv3 (one conv
 * over [x ; h] written by their producers into one buffer, no torch.cat, no residual round trip).  The residual and the
 * split-K slabs stay dense; a strided y runs unsplit. */
int advhip_conv3d_bn_act_strided_f32(const advhip_conv3d_desc* d, const float* x, int64_t x_batch_stride,
                                     const float* w_packed, const int32_t* ktab, const float* scale, const float* shift,
                                     const float* residual, float* y, int64_t y_batch_stride, void* workspace,
                                     int64_t workspace_bytes, void* stream);

/* The same with the extra epilogue operands the MGFN scorer's GEMM-shaped layers need, all optional (a 1x1 Conv1d over a
 * (C, B*T) activation is this conv on a (1, C, 1, 1, B*T) tensor; src/models/mgfn/modeling_mgfn.py:49-64, 150-205):
 *   y_preact (nullable, y's shape / batch stride): receives the value BEFORE the activation -- z of h = GELU(z), kept for
 *            the backward pass while y gets h (MGFNFeedForward in_conv -> GELU, :53-56);
 *   dact_z   (nullable, y's shape, dense): the result is multiplied by GELU'(dact_z) -- the backward of that GELU fused into
 *            the GEMM that produces dL/dh (dL/dz = (W_out^T . dL/dy) * GELU'(z)).
 *   ln_u / ln_mu / ln_rs (nullable, together): the channel-LayerNorm fold for a 1x1x1 conv -- with w_packed holding
 *            W.diag(g) and ln_u[n] its row sums, v = acc * ln_rs[m] - ln_u[n] * ln_mu[m] * ln_rs[m] turns the conv of the RAW
 *            activation into W.LN(x) minus the W.b term (put W.b + bias in `shift`): MGFNLayerNorm (:36-46) never
 *            materialises; ln_mu / ln_rs are per position m (advhip_chan_stats_f32).
 * A zero-filled struct = advhip_conv3d_bn_act_strided_f32. */
typedef struct advhip_conv3d_epilogue {
  float* y_preact;
  const float* dact_z;
  const float* ln_u;
  const float* ln_mu;
  const float* ln_rs;
  /* ABI 2.  Nullable: a caller-owned block of arrival counters for the in-launch split-K reduction, 4 bytes per output tile
   * (65 536 bytes cover every shape of the I3D / MGFN plans).  Contract: ZERO when first handed over, used by one stream at a
   * time, never written by the caller afterwards -- each launch leaves it zero (the last arriver of a tile resets its word), so
   * no memset node runs ahead of the launch.  Without it (or if it is too small) the counters live at the head of
   * `workspace` and are cleared by a memset before every launch. */
  void* splitk_counters;
  int64_t splitk_counter_bytes;
  /* ABI 2.  Nullable: (B, Cout) -- the launch writes the mean of act(conv * scale + shift (+ residual)) over each sample's
   * positions here INSTEAD of y (which may then be null): layer4's last conv3 + bn3 + residual + ReLU and the
   * nn.AdaptiveAvgPool3d((1,1,1)) behind it (src/i3d.py:111-121, 314) in one launch.  1x1x1 stride-1 convs on <= 128
   * positions per sample, Cout % 64 == 0, x 16-byte aligned, none of the operands above; bit for bit
   * advhip_global_avgpool_f32 of the conv's own output. */
  float* avgpool_out;
} advhip_conv3d_epilogue;
int advhip_conv3d_bn_act_ex_f32(const advhip_conv3d_desc* d, const float* x, int64_t x_batch_stride, const float* w_packed,
                                const int32_t* ktab, const float* scale, const float* shift, const float* residual, float* y,
                                int64_t y_batch_stride, const advhip_conv3d_epilogue* ep, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* --- the temporal fold (ADVHIP_ALGO_TFOLD_BASE) ---------------------------------------------------------------------------------
 * advhip_conv3d_tfold_desc: the one statement of the rule.  ADVHIP_EINVAL (the message names the rule broken) unless d is a
 * (kt,1,1) conv, strides 1, ph = pw = 0, 2 pt + 1 = kt, T <= pt + 1 (the Bottleneck conv1s with a temporal kernel of layers
 * 2-4, src/i3d.py:71-75, 144-146, whose inputs have T = 2 after maxpool2); otherwise *folded = d with Cin*T input channels,
 * Cout*T output channels, T = 1, kt = 1, pt = 0, and algo ADVHIP_ALGO_DMA2_BASE + tile for a TFOLD id (any other algo value is
 * copied).  Host arithmetic only.  Callers size and build w_packed rows and the gather table from `folded`
 * (advhip_conv3d_packed_rows / advhip_conv3d_build_ktab).
 * advhip_conv3d_pack_weight_tfold_f32: torch-layout weights w[Cout][Cin][kt][1][1] of d -> the folded conv's packed operand
 * w_folded[Kpad'][Cout*T], row ci*T + ti, column n*T + t = w[n][ci][ti - t + pt], zero rows above Cin*T.  Once per (weights, T).
 * advhip_conv3d_tfold_scale_shift_f32: scale_folded[n*T + t] = scale[n], likewise shift (Cout*T entries each). */
int advhip_conv3d_tfold_desc(const advhip_conv3d_desc* d, advhip_conv3d_desc* folded);
int advhip_conv3d_pack_weight_tfold_f32(const advhip_conv3d_desc* d, const float* w, float* w_folded, void* stream);
int advhip_conv3d_tfold_scale_shift_f32(const advhip_conv3d_desc* d, const float* scale, const float* shift, float* scale_folded,
                                        float* shift_folded, void* stream);

/* mu[n] = mean over channels of x[c, n], rs[n] = 1 / (sqrt(biased variance over channels) + eps) for a (C, N) activation:
 * the statistics of MGFNLayerNorm (modeling_mgfn.py:43-46: division by std + eps, not sqrt(var + eps)). */
int advhip_chan_stats_f32(const float* x, float* mu, float* rs, int32_t C, int64_t N, float eps, void* stream);

/* --- conv + max-pool fused (the two nn.MaxPool3d of I3Res50.forward_single, src/i3d.py:303-309) -------------------
 * Pooled extents of conv(d) followed by a floor-mode, padding-0 max-pool with window pk* and stride ps*. */
int advhip_conv3d_pool_out_dims(const advhip_conv3d_desc* d, int32_t pkt, int32_t pkh, int32_t pkw, int32_t pst,
                                int32_t psh, int32_t psw, int32_t* Tp, int32_t* Hp, int32_t* Wp);

/* y = MaxPool3d(k=(2,3,3), s=(2,2,2), p=0)( relu( conv3d(x, w) * scale + shift ) ): the stem conv1 -> bn1 -> relu ->
 * maxpool1 of src/i3d.py:303-306 without writing the un-pooled activation (822 MB at B = 32) to HBM.  The conv runs on
 * m-tiles that are 2(t) x 4(h) x 16(w) bricks of output positions; each brick writes the maxima of the pooling windows
 * it touches (27 per channel) to `workspace`, and a small second launch maxes the 1, 2 or 4 partials of every pooled
 * output: the same fp32 conv values as the unfused pair, so the result is bit-identical to advhip_conv3d_bn_act_f32
 * (relu) + advhip_maxpool3d_f32.  x / y may be channel slices of wider tensors (batch strides in elements, 0 = dense).
 * d->relu and d->algo / d->splits are ignored (ReLU is part of the op; one tile configuration). */
int64_t advhip_conv3d_relu_maxpool233_workspace_bytes(const advhip_conv3d_desc* d);
/* Host arithmetic only: the k-tiles of `bk` packed rows (row k = ((ci*kt+dt)*kh+dh)*kw+dw) that hold at least one row k < K whose
 * temporal tap lies inside the clip for output frame ot, ascending, into tiles[] (nullable; up to ceil(K / bk) entries) and their
 * count into *n_tiles.  Every other k-tile multiplies zero padding at every position of that frame: what the frame-uniform tiles
 * of ADVHIP_ALGO_STEM_BORDER skip (bk = 16).  A frame with no padded tap gets every k-tile. */
int advhip_conv3d_active_ktiles(const advhip_conv3d_desc* d, int32_t ot, int32_t bk, int32_t* tiles, int32_t* n_tiles);
int advhip_conv3d_bn_relu_maxpool233_f32(const advhip_conv3d_desc* d, const float* x, int64_t x_batch_stride,
                                         const float* w_packed, const int32_t* ktab, const float* scale, const float* shift,
                                         float* y, int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                         void* stream);

/* --- the same stem with 16-byte gather pieces: column-parity planes of the input ------------------------------------------------
 * The stem's stride-2 window along w makes its A gather one 4-byte LDS-DMA per (tap, position), and the issue slots those
 * instructions share with the MFMAs are what bounds the kernel.  With the input rewritten as column-parity planes
 *   xs[b, c, t, h, par, 2 + j] = x[b, c, t, h, 2 j + par]   (advhip_split_w_f32; WP = advhip_split_w_plane_floats(W) = W/2 + 4
 *   floats per plane, zero columns either side)
 * tap dw of four consecutive output columns reads four CONSECUTIVE floats of plane (dw - pw) & 1: one 16-byte piece per lane,
 * two whole k-rows of the tile per wave-instruction (4x fewer A instructions).  Same K order, operands and accumulation as
 * advhip_conv3d_bn_relu_maxpool233_f32: bit-identical results.  Needs stride 2, an odd kernel <= 9 with padding kw/2 along w,
 * W even and an output width that is a multiple of 4 (the I3D stem: 7 / 2 / 3, 224 -> 112).  ktab_s2w: int32[2 * Kpad]. */
int32_t advhip_split_w_plane_floats(int32_t W);
int advhip_split_w_f32(const float* x, float* xs, int64_t rows, int32_t W, void* stream);
int advhip_conv3d_s2w_build_ktab(const advhip_conv3d_desc* d, int32_t* ktab_s2w, void* stream);
int advhip_conv3d_s2w_bn_relu_maxpool233_f32(const advhip_conv3d_desc* d, const float* xs, int64_t xs_batch_stride,
                                             const float* w_packed, const int32_t* ktab_s2w, const float* scale, const float* shift,
                                             float* y, int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                             void* stream);

/* TenCrop + float + normalise + the layout permutes (advhip_tencrop_normalize_u8 below) writing those planes directly for
 * crop-clips [first_crop_clip, first_crop_clip + count) of a video: xs (count, C, frames_per_clip, crop, 2, crop/2 + 4).  The
 * real-data path in front of advhip_conv3d_s2w_bn_relu_maxpool233_f32: the planes cost the pass nothing extra, and the values
 * are those of advhip_tencrop_normalize_u8 (same arithmetic per pixel), so the features equal the fp32 pipeline's bit for bit. */
int advhip_tencrop_normalize_planes_u8(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                       int32_t frames_per_clip, int32_t crop, int64_t first_crop_clip, int64_t count, float mean,
                                       float stdv, void* stream);
/* ... for windows that start every `clip_stride` frames (advhip_tencrop_normalize_u8_strided below); the call above is
 * clip_stride = frames_per_clip. */
int advhip_tencrop_normalize_planes_u8_strided(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                               int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int64_t first_crop_clip,
                                               int64_t count, float mean, float stdv, void* stream);
/* ... for a crop subset (advhip_tencrop_normalize_u8_crops below): crop-clip = clip * ncrops + j, [first, first + count) within
 * windows * ncrops; the call above is the identity set. */
int advhip_tencrop_normalize_planes_u8_crops(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                             int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int32_t ncrops,
                                             uint64_t crops_packed, int64_t first_crop_clip, int64_t count, float mean, float stdv,
                                             void* stream);
/* ... sampling every `frame_step`-th frame (advhip_tencrop_normalize_u8_sampled below); the call above is frame_step = 1. */
int advhip_tencrop_normalize_planes_u8_sampled(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                               int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                               int32_t ncrops, uint64_t crops_packed, int64_t first_crop_clip, int64_t count, float mean,
                                               float stdv, void* stream);

/* --- the same stem, fed by resized uint8 frames (src/gtransforms.py:29-38,57-73 + extract_features.py:83-89 in the load stage)
 * frames: uint8 (F, FH, FW, Cin) -- what the decoder + GroupResize hand over -- F a whole number of clips of d->T frames.
 * Sample b of the launch (d->B of them) is crop-clip first_crop_clip + b = clip * 10 + crop in torchvision's TenCrop order
 * (top-left, top-right, bottom-left, bottom-right, centre, then the same five mirrored along w); d->H / d->W are the crop size.
 * The gather reads the crop's pixels as bytes (`buffer_load_ubyte ... lds`), the operand of the matrix pipe is the pixel value
 * (exact in fp32), sum w (pixel - mean) = acc - mean * (sum of the weights of the taps inside the clip) with that sum tabulated
 * per border class, and 1/std is folded into the BN scale: neither the fp32 ten-crop tensor (385 MB per 40 crop-clips) nor
 * the un-pooled stem output exists.
 *   advhip_conv3d_u8_table_sizes: element counts of the two tables below (int32 / float)
 *   advhip_conv3d_u8_build_tables: ktab_u8 = gather offsets (as stored + mirrored); corr = -mean * (sum of the weights of the
 *     taps inside the clip) per border class (per dimension: taps before the clip * (p + 1) + taps past its end) and channel;
 *     once per (weights, FH, FW, clip dims)
 * Result: within fp32 rounding of advhip_tencrop_normalize_u8 + advhip_conv3d_bn_relu_maxpool233_f32 (tests: 2e-5). */
int advhip_conv3d_u8_table_sizes(const advhip_conv3d_desc* d, int64_t* ktab_ints, int64_t* corr_floats);
int advhip_conv3d_u8_build_tables(const advhip_conv3d_desc* d, int32_t FH, int32_t FW, const float* w_packed, float mean,
                                  int32_t* ktab_u8, float* corr, void* stream);
int advhip_conv3d_u8_tencrop_bn_relu_maxpool233_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                    int32_t FW, int64_t first_crop_clip, const float* w_packed,
                                                    const int32_t* ktab_u8, const float* corr,
                                                    const float* scale, const float* shift, float stdv, float* y,
                                                    int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                                    void* stream);
/* Overlapping windows: clip w = frames [w * clip_stride, w * clip_stride + d->T), 1 <= clip_stride <= d->T, and the buffer holds
 * whole windows, F = (n - 1) * clip_stride + d->T (the caller appends the LoopPad frames of a short last window).  The stride is
 * one launch argument of the same kernel (the gather tables depend on the geometry only); clip_stride = d->T is the call above. */
int advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                            int32_t FW, int32_t clip_stride, int64_t first_crop_clip,
                                                            const float* w_packed, const int32_t* ktab_u8, const float* corr,
                                                            const float* scale, const float* shift, float stdv, float* y,
                                                            int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                                            void* stream);
/* A crop SUBSET of the ten: `ncrops` (1..10) strictly ascending TenCrop indices (0-3 corners, 4 centre, 5-9 the same of the
 * mirrored frame), entry j in bits [4 j, 4 j + 4) of `crops_packed`, the bits above zero.  Sample b of the launch is crop-clip
 * first_crop_clip + b = (clip g / ncrops, crop entry g % ncrops); first_crop_clip + d->B <= windows * ncrops.  The set is one
 * by-value launch argument of the same kernel (no table in memory); every row is bit for bit the row the ten-crop call gives
 * for that (clip, crop).  (10, 0x9876543210) is the call above.  A malformed set is refused (ADVHIP_EINVAL) before any launch. */
int advhip_conv3d_u8_tencrop_bn_relu_maxpool233_crops_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                          int32_t FW, int32_t clip_stride, int32_t ncrops, uint64_t crops_packed,
                                                          int64_t first_crop_clip, const float* w_packed, const int32_t* ktab_u8,
                                                          const float* corr, const float* scale, const float* shift, float stdv, float* y,
                                                          int64_t y_batch_stride, void* workspace, int64_t workspace_bytes, void* stream);
/* Temporal sampling: clip w = frames w * clip_stride + t * frame_step, t in [0, d->T) -- every frame_step-th frame of a span of
 * d->T * frame_step frames.  frame_step >= 1, 1 <= clip_stride <= d->T * frame_step, and the buffer holds whole windows: F >=
 * (d->T - 1) * frame_step + 1 with (F - ((d->T - 1) * frame_step + 1)) % clip_stride == 0 (the caller puts a short last window's
 * LoopPad frames into the slots that window samples).  The step is scalar set-up of the same kernel (window origin and the
 * temporal term of the gather table, which advhip_conv3d_u8_build_tables_sampled builds for that frame_step: a table built for
 * one step must not be used with another); rows are bit for bit what the call above gives for the sampled frames as a video
 * of their own.  frame_step = 1 is the call above.  Refused (ADVHIP_EINVAL) before any launch. */
int advhip_conv3d_u8_build_tables_sampled(const advhip_conv3d_desc* d, int32_t FH, int32_t FW, int32_t frame_step, const float* w_packed,
                                          float mean, int32_t* ktab_u8, float* corr, void* stream);
int advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                            int32_t FW, int32_t clip_stride, int32_t frame_step, int32_t ncrops,
                                                            uint64_t crops_packed, int64_t first_crop_clip, const float* w_packed,
                                                            const int32_t* ktab_u8, const float* corr, const float* scale, const float* shift,
                                                            float stdv, float* y, int64_t y_batch_stride, void* workspace,
                                                            int64_t workspace_bytes, void* stream);

/* The same stem from WHOLE PIXELS: K runs tap-major (k' = tap * 3 + c), one 4-byte LDS-DMA per (tap, position) fetches the
 * pixel's three channel bytes at the pixel's byte address (a third of the gather instructions of the byte form for the same
 * K; LDS-DMA and ds_read take byte-granular addresses on gfx950), the byte select is part of the LDS read address.  Cin = 3,
 * Cout = 64.  `readable_bytes`: bytes readable from `frames` on; must be >= F*FH*FW*3 + 1 (the last pixel's 4-byte piece).
 *   w_taps: the weights re-ordered tap-major (built from w_packed), ktab_taps: pixel offsets per tap (as stored + mirrored). */
int advhip_conv3d_u8_taps_table_sizes(const advhip_conv3d_desc* d, int64_t* ktab_ints, int64_t* corr_floats, int64_t* w_taps_floats);
int advhip_conv3d_u8_taps_build_tables(const advhip_conv3d_desc* d, int32_t FH, int32_t FW, const float* w_packed, float mean,
                                       int32_t* ktab_taps, float* corr, float* w_taps, void* stream);
int advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                         int32_t FW, int64_t readable_bytes, int64_t first_crop_clip,
                                                         const float* w_taps, const int32_t* ktab_taps, const float* corr,
                                                         const float* scale, const float* shift, float stdv, float* y,
                                                         int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                                         void* stream);
/* ... over windows every `clip_stride` frames, as advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32. */
int advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_strided_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                                 int32_t FW, int32_t clip_stride, int64_t readable_bytes,
                                                                 int64_t first_crop_clip, const float* w_taps, const int32_t* ktab_taps,
                                                                 const float* corr, const float* scale, const float* shift, float stdv,
                                                                 float* y, int64_t y_batch_stride, void* workspace,
                                                                 int64_t workspace_bytes, void* stream);
/* ... for a crop subset, as advhip_conv3d_u8_tencrop_bn_relu_maxpool233_crops_f32. */
int advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_crops_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                               int32_t FW, int32_t clip_stride, int32_t ncrops, uint64_t crops_packed,
                                                               int64_t readable_bytes, int64_t first_crop_clip, const float* w_taps,
                                                               const int32_t* ktab_taps, const float* corr, const float* scale,
                                                               const float* shift, float stdv, float* y, int64_t y_batch_stride,
                                                               void* workspace, int64_t workspace_bytes, void* stream);
/* ... sampling every `frame_step`-th frame, as advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32 (tables for that step). */
int advhip_conv3d_u8_taps_build_tables_sampled(const advhip_conv3d_desc* d, int32_t FH, int32_t FW, int32_t frame_step,
                                               const float* w_packed, float mean, int32_t* ktab_taps, float* corr, float* w_taps,
                                               void* stream);
int advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_sampled_f32(const advhip_conv3d_desc* d, const uint8_t* frames, int64_t F, int32_t FH,
                                                                 int32_t FW, int32_t clip_stride, int32_t frame_step, int32_t ncrops,
                                                                 uint64_t crops_packed, int64_t readable_bytes, int64_t first_crop_clip,
                                                                 const float* w_taps, const int32_t* ktab_taps, const float* corr,
                                                                 const float* scale, const float* shift, float stdv, float* y,
                                                                 int64_t y_batch_stride, void* workspace, int64_t workspace_bytes,
                                                                 void* stream);

/* y = MaxPool3d(k=(2,1,1), s=(2,1,1))( act( conv3d(x, w) * scale + shift (+ residual) ) ) for a 1x1x1 stride-1 conv
 * (Cin a multiple of 32) in ONE launch: the last Bottleneck of layer1 followed by maxpool2 (src/i3d.py:111-121, 309).
 * Each m-tile holds both frames of a pooling pair, so the pooling is exact inside the epilogue: the un-pooled
 * activation is neither written nor read back.  `residual` (nullable) has the UN-pooled conv output's shape, dense. */
int advhip_conv3d_bn_act_maxpool211_f32(const advhip_conv3d_desc* d, const float* x, int64_t x_batch_stride,
                                        const float* w_packed, const int32_t* ktab, const float* scale, const float* shift,
                                        const float* residual, float* y, int64_t y_batch_stride, void* stream);

/* nn.MaxPool3d with zero padding=0, floor mode (src/i3d.py:212-217, 306, 309). */
int advhip_maxpool3d_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, int32_t H,
                         int32_t W, int32_t kt, int32_t kh, int32_t kw, int32_t st, int32_t sh,
                         int32_t sw, void* stream);

/* nn.MaxPool3d with padding (implicit -inf, at most half the window; floor mode): the stem pool k(1,3,3) s(1,2,2) p(0,1,1)
 * of the pytorchvideo ResNet that `i3d_8x8_r50` names (src/i3d.py:339-350).  Dense x and y. */
int advhip_maxpool3d_padded_f32(const float* x, float* y, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W, int32_t kt,
                                int32_t kh, int32_t kw, int32_t st, int32_t sh, int32_t sw, int32_t pt, int32_t ph, int32_t pw,
                                void* stream);

/* The same, y being a channel slice of a wider tensor (y_batch_stride in elements, 0 = dense). */
int advhip_maxpool3d_strided_f32(const float* x, float* y, int64_t y_batch_stride, int32_t B, int32_t C, int32_t T, int32_t H,
                                 int32_t W, int32_t kt, int32_t kh, int32_t kw, int32_t st, int32_t sh, int32_t sw, void* stream);

/* nn.AdaptiveAvgPool3d((1,1,1)) (src/i3d.py:244, 314): x (rows, n) -> y (rows), mean over n. */
int advhip_global_avgpool_f32(const float* x, float* y, int64_t rows, int32_t n, void* stream);

/* --- batched strided GEMM (fp32 MFMA) ---------------------------------------------------------------------------------
 * C[b,m,n] = epi( alpha * sum_k A[b,m,k] * B[b,k,n] ), element (b,m,k) of A at A + b*sAb + m*sAm + k*sAk (strides in
 * elements; one of sAm / sAk and one of sBk / sBn must be 1), likewise B and C.  Replaces the torch.bmm pair of
 * NonLocalBlock.forward (src/i3d.py:171-178) and the Conv1d / Linear / einsum contractions of the MGFN scorer and their
 * backward products (src/models/mgfn/modeling_mgfn.py:49-64, 96-123, 150-205).  Epilogue, in this order (every pointer
 * nullable): LayerNorm fold  v = v*ln_rs[b,n] - ln_u[m]*ln_mu[b,n]*ln_rs[b,n]  (W.diag(g) applied to RAW columns x equals
 * W.LN(x) minus the bias term when ln_u = W.g row sums: MGFNLayerNorm over channels, modeling_mgfn.py:36-46);
 * + bias_m[m] + bias_n[n];  act (0 none, 1 ReLU, 2 GELU-erf);  + beta * residual (C's strides). */
typedef struct advhip_gemm_desc {
  int32_t M, N, K, batch;
  int64_t sAb, sAm, sAk;
  int64_t sBb, sBk, sBn;
  int64_t sCb, sCm, sCn;
  float alpha, beta;
  int32_t act;
  const float* bias_m;
  const float* bias_n;
  const float* ln_u;
  const float* ln_mu;
  const float* ln_rs;
  const float* residual;
} advhip_gemm_desc;
int advhip_bgemm_f32(const advhip_gemm_desc* d, const float* A, const float* B, float* C, void* stream);

/* C[s][m][n] = sum over K slice s of A[m][k] * B[n][k]: both operands k-contiguous with row pitches lda / ldb (elements, any
 * value >= K: a 16-byte LDS-DMA piece takes any 4-byte aligned address on gfx950; K a multiple of 16; 4-byte aligned bases).
 * The weight gradient dW[o][c] = sum_n dY[o][n] X[c][n] of the MGFN scorer's GEMM-shaped layers, whose activations are stored
 * (channel, position): no transposed copies; and the token conv's tap products on the scorer's input rows as stored (2 049-float
 * pitch, modeling_mgfn.py:81-93).  LDS-DMA row copies, fp32 MFMA.  splits > 1 cuts K into slices written to C + s * slab_stride (the caller sums them). */
int advhip_gemm_nt_f32(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                       int64_t ldc, int32_t splits, int64_t slab_stride, void* stream);

/* The same product with the row sums of A beside it: rowsum_a[s][m] = sum over K slice s of A[m][k] (nullable) -- the bias
 * gradient db[o] = sum_n dY[o][n] of the same layer (autograd of nn.Conv1d's bias, modeling_mgfn.py:53-56, 101, 155, 167) out of
 * the fragments the n-tile-0 workgroups hold anyway, instead of a second pass over dY.  `tile`: 0 = heuristic, 1 = 64 x 64,
 * 2 = 128 x 64, 3 = 128 x 128 output tile per workgroup. */
int advhip_gemm_nt_rowsum_f32(const float* A, const float* B, float* C, float* rowsum_a, int32_t M, int32_t N, int32_t K,
                              int64_t lda, int64_t ldb, int64_t ldc, int32_t splits, int64_t slab_stride, int32_t tile,
                              void* stream);

/* The same with the K slices summed INSIDE the launch: every (tile, slice) workgroup publishes its partial tile (write-through
 * stores) into `workspace`, the workgroup that arrives last at the tile's counter sums the slices in slice order (run-to-run
 * bit-identical) and writes C (M x N, pitch ldc) and rowsum_a (M, nullable) once -- no slabs, no second pass.
 * `workspace`: 256-byte aligned, advhip_gemm_nt_workspace_bytes(M, N, splits, tile) bytes, whose first 64 KiB (the arrival
 * counters: at most 16 384 output tiles) are ZERO on entry; the launch leaves them zero, so a workspace zero-filled once
 * serves every later launch -- of any shape -- on the same stream. */
int64_t advhip_gemm_nt_workspace_bytes(int32_t M, int32_t N, int32_t splits, int32_t tile);
int advhip_gemm_nt_reduced_f32(const float* A, const float* B, float* C, float* rowsum_a, int32_t M, int32_t N, int32_t K,
                               int64_t lda, int64_t ldb, int64_t ldc, int32_t splits, int32_t tile, void* workspace,
                               int64_t workspace_bytes, void* stream);

/* Few output tiles (the 64- and 128-channel layers' weight gradients: M x N of a few 64 x 64 tiles, K = all positions): there
 * the last arriver's serial sum is the whole tail of the launch, so the slices go to `slabs` = [splits][M*N (+ M row sums when
 * with_rowsum)] and advhip_sum_slabs_f32 (dst[i] = sum in slice order of src[s*stride + i]) reduces product AND row sums
 * in one further launch. */
int advhip_gemm_nt_slabs_f32(const float* A, const float* B, float* slabs, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                             int32_t splits, int32_t tile, int32_t with_rowsum, void* stream);
int advhip_sum_slabs_f32(const float* slabs, float* out, int64_t n, int32_t splits, int64_t stride, void* stream);
/* Many such products in ONE launch: item i writes slice s of A_i B_i^T (64 x 64 tiles, as advhip_gemm_nt_slabs_f32 with tile 1) to
 * C_i + s * slab_stride (row pitch N_i) and, when rowsum_i is given, the slice's row sums of A_i to rowsum_i + s * slab_stride;
 * all items contract over the same K in the same number of slices.  With C_i / rowsum_i laid out back to back inside one
 * [splits][slab_stride] matrix, ONE advhip_sum_slabs_f32 reduces every product and every row sum.  `items` is a HOST array (it
 * travels in the kernel arguments, 32 items per launch): the weight and bias gradients of all narrow layers of an MGFN training
 * step (autograd of nn.Conv1d, modeling_mgfn.py:49-64,101-108,150-193) at the end of the backward pass. */
typedef struct advhip_nt_item {
  const float* A;  /* (M, K), row pitch lda */
  const float* B;  /* (N, K), row pitch ldb */
  float* C;
  float* rowsum;   /* nullable */
  int32_t M, N;
  int64_t lda, ldb;
} advhip_nt_item;
int advhip_gemm_nt_group_slabs_f32(const advhip_nt_item* items, int32_t n_items, int32_t K, int32_t splits, int64_t slab_stride, void* stream);

/* y[r, :] = softmax(x[r, :] * scale) over rows of n contiguous floats (F.softmax(theta_phi * dim_inner**-0.5, dim=-1),
 * src/i3d.py:174-175; the attention softmax of GlanceAttention, modeling_mgfn.py:115-120).  x == y allowed. */
int advhip_softmax_rows_f32(const float* x, float* y, int64_t rows, int32_t n, float scale, void* stream);

/* --- MGFN body: fused element-wise / reduction kernels on (C, N) activations (channels outermost) --------------------
 * MGFNLayerNorm over the channel dim (modeling_mgfn.py:36-46): y = (x - mean_c) / (sqrt(var_biased_c) + eps) * g[c] + b[c]
 * per position n; mu / rs (= 1 / (std + eps)) per position are returned for the backward pass. */
int advhip_chan_layernorm_fwd_f32(const float* x, const float* g, const float* b, float* y, float* mu, float* rs, int32_t C,
                                  int64_t N, float eps, void* stream);
/* Its backward: dx (C, N), and per-block partial sums of dg / db as [advhip_chan_layernorm_bwd_partial_rows(N)][C] matrices
 * (the caller sums the rows: fixed order, no atomics). */
int64_t advhip_chan_layernorm_bwd_partial_rows(int64_t N);
int advhip_chan_layernorm_bwd_f32(const float* dy, const float* x, const float* g, const float* mu, const float* rs, float* dx,
                                  float* dg_partial, float* db_partial, int32_t C, int64_t N, float eps, void* stream);

/* nn.BatchNorm1d in training mode on a (C, N) activation (FocusAttention.norm, modeling_mgfn.py:162, 174): batch statistics
 * per channel row, y = (x - mean) * rsqrt(var_biased + eps) * gamma + beta; mean / var are returned (running-statistics
 * update by the caller, backward).  Backward: dx, dgamma, dbeta. */
int advhip_bn_rows_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* var, int32_t C,
                           int64_t N, float eps, void* stream);
int advhip_bn_rows_bwd_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* var, float* dx,
                           float* dgamma, float* dbeta, int32_t C, int64_t N, float eps, void* stream);

/* The same three with the fusions a training step's launch count asks for (bit-identical arithmetic):
 *   advhip_bn_rows_fwd_running_f32: also updates nn.BatchNorm1d's running_mean / running_var in place (nullable, together:
 *     running = (1 - momentum) * running + momentum * batch, the variance unbiased) -- torch's five small launches;
 *   advhip_bn_rows_bwd_add_f32 / advhip_chan_layernorm_bwd_add_f32: dx = backward + add (nullable, dx's shape) -- the
 *     gradient of the block's skip connection (y = f(norm(x)) + x) without autograd's separate add; the LayerNorm form writes
 *     its per-block partial sums as ONE [rows][2C] matrix (dg in columns [0, C), db in [C, 2C)): one reduction for both. */
int advhip_bn_rows_fwd_running_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* var,
                                   float* running_mean, float* running_var, float momentum, int32_t C, int64_t N, float eps,
                                   void* stream);
int advhip_bn_rows_bwd_add_f32(const float* dy, const float* x, const float* gamma, const float* mean, const float* var,
                               const float* add, float* dx, float* dgamma, float* dbeta, int32_t C, int64_t N, float eps, void* stream);
int advhip_chan_layernorm_bwd_add_f32(const float* dy, const float* x, const float* g, const float* mu, const float* rs,
                                      const float* add, float* dx, float* dgb_partial, int32_t C, int64_t N, float eps, void* stream);

/* A whole `x = x + FFN(LN(x))` step of a NARROW block in one launch (MGFNLayerNorm -> Conv1d(C, 4C, 1) -> GELU -> Conv1d(4C, C, 1) -> + x,
 * modeling_mgfn.py:36-64, 147, 205), C = 64 or 128 channels, N a multiple of 64 positions, activations (C, N) with the positions contiguous:
 *   forward : w1 = in_conv.weight (4C, C), w2 = out_conv.weight (C, 4C) AS STORED; writes y and what the backward pass keeps: xh = LN(x),
 *             mu / rs (N), h = GELU(W1 xh + b1) and z = GELU'(W1 xh + b1), both (4C, N);
 *   backward: w2_packed / w1_packed = the forward GEMMs' packed operands [4C][C] / [C][4C] (advhip_conv3d_pack_weight_f32); writes
 *             dz = (W2^T dy) * z (4C, N) -- what the weight gradients dW1 = dz xh^T, db1 = rowsum(dz) contract with (dW2 = dy h^T) --,
 *             dx = LayerNorm backward of W1^T dz + dy (the skip connection), and dgb_partial [advhip_ffn_block_partial_rows(N)][2C]: per-workgroup
 *             partial sums of dg (columns [0, C)) and db ([C, 2C)), to be column-summed (advhip_colsum_f32 / _group).
 * The same arithmetic as advhip_chan_layernorm_fwd_f32 + two advhip_conv3d_bn_act_ex_f32 launches (activation code 3, then bias + residual) and
 * their three backward launches; sums inside a dot product run in another order (agreement ~1e-6). */
int64_t advhip_ffn_block_partial_rows(int64_t N);
int advhip_ffn_block_fwd_f32(const float* x, const float* ln_g, const float* ln_b, float eps, const float* w1, const float* b1,
                             const float* w2, const float* b2, float* xh, float* mu, float* rs, float* h, float* z, float* y, int32_t C,
                             int64_t N, void* stream);
int advhip_ffn_block_bwd_f32(const float* dy, const float* x, const float* ln_g, const float* mu, const float* rs, float eps, const float* z,
                             const float* w2_packed, const float* w1_packed, float* dz, float* dx, float* dgb_partial, int32_t C, int64_t N,
                             void* stream);

/* The packed operand of a Conv1d's transposed conv (its input gradient dX = conv1d(dY; W'), W'[c][o][j] = W[o][c][k-1-j];
 * autograd of nn.Conv1d, modeling_mgfn.py:101,155) straight from the parameter w (Cout, Cin, k):
 * w_packed[(o*k + j)][c] = w[o][c][k-1-j], rows padded with zeros to a multiple of 32 -- one launch instead of flip +
 * transpose + pack. */
int advhip_conv1d_pack_weight_dx_f32(const float* w, float* w_packed, int32_t Cout, int32_t Cin, int32_t k, void* stream);

/* Every packed operand a training step needs, in one launch: item i packs the Conv1d parameter `src` (Cout, Cin, k) into `dst`,
 * mode 0 = advhip_conv3d_pack_weight_f32's [roundup32(Cin*k)][Cout] (the forward GEMM's operand), mode 1 =
 * advhip_conv1d_pack_weight_dx_f32's [roundup32(Cout*k)][Cin] (the input gradient's).  `items_dev` is an array in DEVICE memory;
 * tile_begin = the exclusive prefix sum of advhip_pack_item_tiles over the items, n_tiles their total.  Replaces the per-layer
 * weight re-packs autograd's forward of nn.Conv1d hides inside MIOpen (modeling_mgfn.py:101-108,155,183-193). */
typedef struct advhip_pack_item {
  const float* src;
  float* dst;
  int32_t Cout, Cin, k;
  int32_t mode;
  int32_t tile_begin;
  int32_t reserved;
} advhip_pack_item;
int64_t advhip_pack_item_tiles(int32_t Cout, int32_t Cin, int32_t k, int32_t mode);
int advhip_pack_weights_multi_f32(const advhip_pack_item* items_dev, int32_t n_items, int32_t n_tiles, void* stream);

/* MGFNFeatureAmplifier (modeling_mgfn.py:81-93) after the GEMM of the stacked tap matrices: y[o, r, t] = sum_j z[j, o, r, t + j - 1]
 * (zero outside [0, T)) + bias[o] + ratio * (sum_j wm[o][j] * mag[r, t + j - 1] + bm[o]) for z (3, O, rows, T), mag = the magnitude
 * channel read in place: element (r, t) at mag[(r * T + t) * mag_stride].  Backward: dz (3, O, rows, T), d_bias (O), d_wm (O, 3),
 * d_bm (O) -- the magnitude itself gets no gradient (it is input data). */
int advhip_amp_combine_fwd_f32(const float* z, const float* bias, const float* mag, int64_t mag_stride, const float* wm, const float* bm,
                               float ratio, float* y, int32_t O, int64_t rows, int32_t T, void* stream);
int advhip_amp_combine_bwd_f32(const float* dy, const float* mag, int64_t mag_stride, float ratio, float* dz, float* d_bias, float* d_wm,
                               float* d_bm, int32_t O, int64_t rows, int32_t T, void* stream);

/* --- Padded batches of sequences of unequal length (inference: batched validation) ---------------------------------------------
 * A batch of videos of unequal length is a (C, rows, T) activation with T = the longest and one length per row, row_lens (device
 * int32[rows], 1 <= len <= T; validated by the caller, clamped to T here -- nothing is ever indexed past T).  The four operators that
 * read a position's neighbours in time take the lengths; all of them STORE 0 at t >= len (they never multiply by a mask, so
 * NaN / uninitialised values behind a row's end cannot reach a real position) and write every element of their output.  For a
 * row with len = T each computes exactly what its entry point without lengths computes.  Forward only.
 *
 * advhip_amp_combine_fwd_lens_f32: advhip_amp_combine_fwd_f32 whose taps stop at the row's end; z and mag at t >= len are never read. */
int advhip_amp_combine_fwd_lens_f32(const float* z, const float* bias, const float* mag, int64_t mag_stride, const float* wm, const float* bm,
                                    float ratio, float* y, int32_t O, int64_t rows, int32_t T, const int32_t* row_lens, void* stream);
/* x (C, rows, T) in place: x[c, r, t] = 0 for t >= row_lens[r]; only those elements are touched.  What stands in front of a k = 3
 * conv (a GEMM of the conv kernels, which know no lengths) whose input's tails a pointwise layer has filled. */
int advhip_mask_tail_f32(float* x, int32_t C, int64_t rows, int32_t T, const int32_t* row_lens, void* stream);
/* One launch fills a padded batch: video v, stored (ncrops, lens[v], width) at element src_offsets[v] of `store`, goes to
 * dst[v, c, t < lens[v], :] of dst (n_videos, ncrops, Tmax, width).  Rows t >= lens[v] of dst are left as they are. */
int advhip_pack_padded_f32(const float* store, const int64_t* src_offsets, const int32_t* lens, float* dst, int32_t n_videos, int32_t ncrops,
                           int32_t Tmax, int32_t width, void* stream);
/* A shuffled training step's input in one launch: dst (b0 + b1, R) fp32 gets src0[idx0[i]] in row i < b0 and src1[idx1[i]] in row
 * b0 + i, for stores src0 (n0, R) and src1 (n1, R) and device int64 index vectors; dst_lab0[i] = lab0[idx0[i]] and dst_lab1[i] =
 * lab1[idx1[i]] beside them (lab / dst_lab of a store: both or neither).  b1 = 0: no second store (its arguments are not read).
 * A copy of bits: NaN payloads, -0.0 and denormals arrive as they are.  An index outside [0, n) reads nothing; its row of dst and
 * its label are NaN, and no other row changes.  16-byte accesses when the stores, dst and R * 4 are 16-byte multiples, 4-byte ones
 * otherwise (any 4-byte-aligned view works); element offsets are 64-bit.  b0 + b1 <= 65535. */
int advhip_gather_batch_f32(const float* src0, const int64_t* idx0, const float* lab0, int64_t n0, int32_t b0, const float* src1,
                            const int64_t* idx1, const float* lab1, int64_t n1, int32_t b1, float* dst, float* dst_lab0,
                            float* dst_lab1, int64_t R, void* stream);

/* dst[c] = sum over r, in row order, of src[r][c]: the per-block partial sums the backward kernels above leave to the caller
 * (rows = a few hundred blocks). */
int advhip_colsum_f32(const float* src, float* dst, int64_t rows, int32_t cols, void* stream);
/* The same for many matrices in one launch (`items`: a HOST array, 64 per launch, carried in the kernel arguments): all partial-sum
 * matrices of a backward pass at its end.  period > 0: the columns are [cols / period groups][period] and leave de-interleaved --
 * element j < period - 1 of group h at dst[h * (period - 1) + j], the last element of every group at
 * dst[(cols / period) * (period - 1) + h]: advhip_dwconv_t_bwd_f32's per-head (K filter taps | bias) sums as the filter gradient
 * followed by the bias gradient (period = K + 1). */
typedef struct advhip_colsum_item {
  const float* src;
  float* dst;
  int64_t rows;
  int32_t cols;
  int32_t period;
} advhip_colsum_item;
int advhip_colsum_group_f32(const advhip_colsum_item* items, int32_t n_items, void* stream);

/* torch.optim.Adam's update (L2 weight decay added to the gradient, no amsgrad; /root/reference/src/runner.py:53-59) for many fp32
 * tensors in one launch per 80 of them (`items`: a HOST array, carried in the kernel arguments -- graph-capturable as is):
 *   g' = g + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * (fp32 arithmetic; 1 - beta and lr / (1 - beta^t) formed in double and rounded once, as torch's Python code does)
 * with t = *step: a device-side fp32 counter (torch's capturable Adam keeps one per parameter) that the caller has already
 * incremented for this step. */
typedef struct advhip_adam_item {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  const float* step;
  int64_t n;
} advhip_adam_item;
int advhip_adam_multi_f32(const advhip_adam_item* items, int32_t n_items, double lr, double beta1, double beta2, double eps,
                          double weight_decay, void* stream);

/* The same update with its two per-step scalars in DEVICE memory, where a replay of a captured launch reads them live:
 *   lr = *lr_dev (a double: lr / (1 - b1^t) is still formed in double and rounded once);
 *   g  = grad * *grad_scale_dev first, as one separately rounded fp32 product (torch's in-place `g.mul_(coef)` of
 *        clip_grad_norm_), unless grad_scale_dev is null.  `grad` itself is not written.
 * Everything after the scaled gradient is the arithmetic of advhip_adam_multi_f32: with *lr_dev == lr and no scale (or 1.0) the
 * results are bit for bit the same. */
int advhip_adam_multi_dev_f32(const advhip_adam_item* items, int32_t n_items, const double* lr_dev, const float* grad_scale_dev, double beta1,
                              double beta2, double eps, double weight_decay, void* stream);

/* Global L2 norm of many fp32 tensors and clip_grad_norm_'s factor, on the device (`items`: a HOST array, carried in the kernel
 * arguments, 240 tensors per launch):
 *   *norm_out  = (float)sqrt(sum of squares), the squares formed and added in double (no overflow at |g| > 1.8e19);
 *   *scale_out = min(1, max_norm / (*norm_out + 1e-6)) in torch's fp32 operations and order: (1 / (norm + 1e-6f)) * (float)max_norm,
 *                clamped from above; a NaN stays a NaN, an infinite norm gives 0.
 * Stage 1 writes one double per 4096 consecutive elements of a tensor to `partials` (room for n_partials of them; needed:
 * the sum over the items of ceil(n / 4096)), stage 2 is one workgroup that adds them.  All orders are fixed and there are no
 * atomics: the same inputs give the same bits.  max_norm: finite, > 0. */
typedef struct advhip_norm_item {
  const float* grad;
  int64_t n;
} advhip_norm_item;
int advhip_grad_norm_multi_f32(const advhip_norm_item* items, int32_t n_items, double max_norm, double* partials, int64_t n_partials,
                               float* norm_out, float* scale_out, void* stream);

/* The operand of a k = 3, padding 1 Conv1d's weight gradient (autograd of nn.Conv1d, modeling_mgfn.py:101,155):
 * u[(c*3 + j), r, t] = x[c, r, t + j - 1] (zero outside [0, T)), x (C, rows, T) -> u (3C, rows, T); dW = dY . u^T by
 * advhip_gemm_nt_f32.  T a multiple of 4. */
int advhip_unfold3_f32(const float* x, float* u, int32_t C, int64_t rows, int32_t T, void* stream);

/* FocusAttention.rel_pos (modeling_mgfn.py:169-171, 176-178): depth-wise temporal conv, one K-tap filter per head, on a
 * (C, rows, T) activation whose channel c belongs to head c % H: out[c,r,t] = bias[h] + sum_j w[h][j] * v[c,r,t+j-K/2]
 * (zero padding).  K in {3, 5}. */
int advhip_dwconv_t_fwd_f32(const float* v, const float* w, const float* bias, float* out, int32_t C, int32_t H, int64_t rows,
                            int32_t T, int32_t K, void* stream);
/* Backward: dv, and partial[(C / H) * chunks][H][K + 1] = per-block sums of (dout * v shifted by tap j, j < K; dout) of channel
 * c = c_idx * H + h -- the caller adds the (C / H) * chunks rows (advhip_colsum_f32; chunks = advhip_dwconv_t_bwd_chunks(C, rows)). */
int32_t advhip_dwconv_t_bwd_chunks(int32_t C, int64_t rows);
/* advhip_dwconv_t_fwd_f32 on a padded batch ("Padded batches" below): row r of (C, rows, T) ends at row_lens_per_row[r]; the taps
 * stop there, out is 0 behind it.  n_rows = the number of lengths, which must be `rows`. */
int advhip_dwconv_t_fwd_lens_f32(const float* v, const float* w, const float* bias, float* out, int32_t C, int32_t H, int64_t rows,
                                 int32_t T, int32_t K, const int32_t* row_lens_per_row, int64_t n_rows, void* stream);
int advhip_dwconv_t_bwd_f32(const float* dout, const float* v, const float* w, float* dv, float* partial, int32_t C, int32_t H,
                            int64_t rows, int32_t T, int32_t K, void* stream);

/* GlanceAttention's core on (C, B, T) activations (modeling_mgfn.py:113-122: q * scale, sim = q^T k, softmax over the keys, out =
 * v attn^T, "b h n d -> b (h d) n"), T = 32 clips, dim_head = 64: qkv (3 * heads * 64, B, T) -- the to_qkv conv's output,
 * q rows then k rows then v rows -- -> out (heads * 64, B, T), the softmax p (B, heads, T, T) kept for the backward pass; one
 * workgroup per (sequence, head).  Backward: dqkv from dout, qkv and p.  torch: scale + bmm + softmax + bmm + layout copy
 * forward, ten launches backward. */
int advhip_glance_attention_fwd_f32(const float* qkv, float* out, float* p, int32_t heads, int64_t B, int32_t T, int32_t dim_head,
                                    float scale, void* stream);
int advhip_glance_attention_bwd_f32(const float* dout, const float* qkv, const float* p, float* dqkv, int32_t heads, int64_t B,
                                    int32_t T, int32_t dim_head, float scale, void* stream);

/* The same core for ANY T (dim_head = 64) -- the validation pass scores a whole video, T = n_clips
 * (/root/reference/src/runner.py:42-50 -> modeling_mgfn.py:107-123): one workgroup per (32-query tile, sequence, head), key / value
 * tiles of 32 clips through LDS with an online softmax; the T x T attention matrix never exists in memory.  lse (B, heads, T) =
 * log-sum-exp of every row of scale * q^T k (nullable: inference) replaces p for the backward pass, which recomputes the softmax
 * tile by tile from qkv, out and lse (dq per query tile, dk / dv per key tile: every output written once, sums in tile order). */
int advhip_glance_attention_fwd_anyt_f32(const float* qkv, float* out, float* lse, int32_t heads, int64_t B, int32_t T, int32_t dim_head,
                                         float scale, void* stream);
int advhip_glance_attention_bwd_anyt_f32(const float* dout, const float* qkv, const float* out, const float* lse, float* dqkv, int32_t heads,
                                         int64_t B, int32_t T, int32_t dim_head, float scale, void* stream);
/* The any-T forward on a padded batch ("Padded batches" above): sequence b still starts at column b * T but has row_lens[b] keys
 * and queries; out is 0 for the queries behind them.  The same two kernels (chosen per launch from T, as above) with the length in
 * T's place: a sequence with row_lens[b] = T gets the bits of advhip_glance_attention_fwd_anyt_f32.  No lse, no backward. */
int advhip_glance_attention_fwd_lens_f32(const float* qkv, float* out, const int32_t* row_lens, int32_t heads, int64_t B, int32_t T,
                                         int32_t dim_head, float scale, void* stream);

/* A per-input-channel affine map x -> mul[c] x[c] + add[c] folded into the 1x1 layer W (O, C) (+ bias, nullable) that follows it:
 *   Wf[o][c] = W[o][c] mul[c];  bias_f[o] = bias[o] + sum_c W[o][c] add[c] (add nullable: 0);  rowsum[o] = sum_c Wf[o][c] (nullable).
 * Eval-mode nn.BatchNorm1d in front of FocusAttention.to_v (modeling_mgfn.py:162, 173-174; mul / add = advhip_bn_fold_f32's scale / shift)
 * and MGFNLayerNorm's (g, b) in front of MGFNFeedForward.in_conv at inference (modeling_mgfn.py:36-64): operand-build time, once per
 * set of weights -- the scoring pass itself then has no normalisation launch and no torch arithmetic for these layers. */
int advhip_fold_affine_f32(const float* W, const float* mul, const float* add, const float* bias, float* Wf, float* bias_f, float* rowsum,
                           int32_t O, int32_t C, void* stream);

/* The scorer's head on the body's (C, N) layout (modeling_mgfn.py:387-389: permute -> nn.LayerNorm(C) -> nn.Linear(C, 1) -> sigmoid):
 * xn (N, C) = LayerNorm over C of y (C, N) -- transposed through LDS, so that the MIL head reads rows --, score[n] =
 * sigmoid(xn[n, :] . fc_w + fc_b[0]); mean / rstd (N) kept for the backward pass.  Backward: dy (C, N) from d_xn (N, C) and
 * d_score (N) (either nullable), and partial[advhip_head_ln_fc_partial_rows(N)][3 C + 1] = per-block sums of
 * (d ln_g | d ln_b | d fc_w | d fc_b) for the caller to add up. */
int64_t advhip_head_ln_fc_partial_rows(int64_t N);
int advhip_head_ln_fc_fwd_f32(const float* y, const float* ln_g, const float* ln_b, const float* fc_w, const float* fc_b, float* xn,
                              float* mean, float* rstd, float* score, int32_t C, int64_t N, float eps, void* stream);
int advhip_head_ln_fc_bwd_f32(const float* d_xn, const float* d_score, const float* y, const float* ln_g, const float* ln_b,
                              const float* fc_w, const float* mean, const float* rstd, const float* score, float* dy, float* partial,
                              int32_t C, int64_t N, void* stream);

/* --- MIL scorer (MGFN head) -----------------------------------------------------------------
 * Fused magnitude / score reduction of magnitude_selection_and_score_prediction
 * (src/models/mgfn/modeling_mgfn.py:314-319): for features (bs*ncrops, T, F) and per-crop scores
 * (bs*ncrops, T): mag[b,t] = mean_c ||features[b*ncrops+c, t, :]||_2, sc[b,t] = mean_c scores. */
int advhip_mil_magnitude_f32(const float* features, const float* scores, float* mag, float* sc,
                             int32_t bs, int32_t ncrops, int32_t T, int32_t F, void* stream);
/* The crop mean of a padded batch's per-crop scores (n_videos * ncrops, Tmax), scattered into a flat per-clip buffer:
 * dst[dst_offsets[v] + t] = (sum_c scores[(v * ncrops + c) * Tmax + t]) / ncrops for t < lens[v] -- summed in crop order from 0.f,
 * one division: the bits of advhip_mil_magnitude_f32's sc.  Nothing else of dst is written. */
int advhip_crop_mean_scatter_f32(const float* scores, const int32_t* lens, const int64_t* dst_offsets, float* dst, int32_t n_videos,
                                 int32_t ncrops, int32_t Tmax, void* stream);

/* Top-k over T of mag*keep (ties -> lowest index first, as torch.topk on CPU/ROCm for distinct
 * values; modeling_mgfn.py:345-346), gather of the k selected feature rows for every crop in
 * crop-major order (modeling_mgfn.py:349-355) and mean of the k selected scores (:359-362).
 *   mag, keep, sc : (n, T)         features : (n*ncrops, T, F)   [row = video*ncrops + crop]
 *   idx  : (n, k) int64            sel      : (ncrops*n, k, F)   [row = crop*n + video]
 *   score: (n)                     keep may be NULL (all ones).   k <= min(16, T); T has no bound but int32 (n * T elements addressed as size_t). */
int advhip_mil_topk_select_f32(const float* mag, const float* keep, const float* sc,
                               const float* features, int64_t* idx, float* sel, float* score,
                               int32_t n, int32_t ncrops, int32_t T, int32_t F, int32_t k,
                               void* stream);

/* Backward of the gather + score mean: scatter-add of d_sel into d_features (must be
 * zero-initialised by the caller) and of d_score/k into d_sc. */
int advhip_mil_topk_select_bwd_f32(const int64_t* idx, const float* d_sel, const float* d_score,
                                   float* d_features, float* d_sc, int32_t n, int32_t ncrops,
                                   int32_t T, int32_t F, int32_t k, void* stream);

/* Backward of advhip_mil_magnitude_f32 w.r.t. features and scores:
 *   d_features[r,t,:] += d_mag[b,t]/ncrops * features[r,t,:]/||features[r,t,:]||,
 *   d_scores[r,t]     += d_sc[b,t]/ncrops                      (r = b*ncrops + c). */
int advhip_mil_magnitude_bwd_f32(const float* features, const float* d_mag, const float* d_sc,
                                 float* d_features, float* d_scores, int32_t bs, int32_t ncrops,
                                 int32_t T, int32_t F, void* stream);

/* Fused loss reductions (src/loss/base.py:7-48, src/loss/mgfn.py:7-47, modeling_mgfn.py:406-418).
 * Inputs: scores (bs,T) video-level scores; abn/nor_score (n) top-k mean scores (n = bs/2);
 *         a_feat/n_feat (ncrops*n, k, F) selected features; labels (n) each.
 * out[0..7] = {total, bce, con, con_a, con_n, smooth, sparse, mgfn}.
 * `ws` is caller scratch of advhip_mgfn_loss_ws_floats(...) floats (holds the L1 norms). */
int64_t advhip_mgfn_loss_ws_floats(int32_t n, int32_t ncrops, int32_t k);
int advhip_mgfn_loss_fwd_f32(const float* scores, const float* abn_score, const float* nor_score,
                             const float* a_feat, const float* n_feat, const float* abn_labels,
                             const float* nor_labels, float* ws, float* out, int32_t bs, int32_t T,
                             int32_t ncrops, int32_t k, int32_t F, void* stream);

/* Gradients of out[0] (times *d_loss) w.r.t. scores, abn/nor_score, a_feat, n_feat. */
int advhip_mgfn_loss_bwd_f32(const float* d_loss, const float* scores, const float* abn_score,
                             const float* nor_score, const float* a_feat, const float* n_feat,
                             const float* abn_labels, const float* nor_labels, const float* ws,
                             float* d_scores, float* d_abn_score, float* d_nor_score,
                             float* d_a_feat, float* d_n_feat, int32_t bs, int32_t T,
                             int32_t ncrops, int32_t k, int32_t F, void* stream);

/* --- feature post-processing (on-device analogues of host numpy code) -------------------------
 * segment(): (n_clips, ncrops, C) -> (ncrops, seg, C) linspace-bucket means
 * (extract_features.py:171-183). */
int advhip_segment_features_f32(const float* feats, float* out, int32_t n_clips, int32_t ncrops,
                                int32_t C, int32_t seg, void* stream);

/* FeatureDataset.add_magnitude (src/dataset.py:121-124): (rows, C) -> (rows, C+1), last column
 * = L2 norm of the row. */
int advhip_add_magnitude_f32(const float* feats, float* out, int64_t rows, int32_t C, void* stream);

/* The same channel with numpy's bits: feats (a, b, C) contiguous -> out (a, b, C+1), or (b, a, C+1) when `transpose` is 1 (a
 * test video (T, ncrops, C) stored the way the scorer reads it).  out[..., :C] is the input bit for bit; out[..., C] equals
 * np.linalg.norm(feats, axis=2) of the float32 array BIT FOR BIT (advhip_add_magnitude_f32 sums in another order and agrees
 * to 1e-6).  numpy's arithmetic, every operation rounded to fp32 on its own (no FMA):
 *   s[i] = x[i] * x[i]
 *   sum  = 0.0f + pw(s, C), where pw(a, n) is
 *            n < 8         : 0.0f + a[0] + a[1] + ... in order
 *            8 <= n <= 128 : r[j] = a[j] (j < 8); for i = 8, 16, ... < n - n % 8: r[j] += a[i + j];
 *                            res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then res += a[i] for the last n % 8
 *            n > 128       : n2 = n / 2; n2 -= n2 % 8; pw(a, n2) + pw(a + n2, n - n2)
 *   out  = sqrt(sum), correctly rounded
 * C <= 8192: numpy reduces in chunks of 8192 elements and the order changes above that; a larger C is refused
 * (ADVHIP_EINVAL, advhip_last_error), as are null pointers, before anything is launched. */
int advhip_add_magnitude_np_f32(const float* feats, float* out, int64_t a, int32_t b, int32_t C,
                                int32_t transpose, void* stream);

/* Host only: the blocks of at most 128 elements the recursion above ends in for a row of C (1 <= C <= 8192), in order, as
 * (start, len, adds) int32 triples into `leaves` (room for 128 triples); `adds` = how many pending partial sums are added once
 * that block's sum is known (the tree of `+` walked with a stack).  This is the table the kernel sums by. */
int advhip_add_magnitude_np_leaves(int32_t C, int32_t* leaves, int32_t* n_leaves);

/* --- live scoring: per-camera feature rings -------------------------------------------------------
 * State owned by the caller, all on the device: ring fp32 (n_cam, ncrops, W, C + 1), counts int64 (n_cam,) = the clips pushed
 * so far per camera, latest fp32 (n_cam,).
 * THE SLOT RULE: the clip pushed when a camera's count is k lies in slot k % W.  A camera at count k therefore holds its last
 * len = min(k, W) clips, and entry t of that window (oldest first, t < len) lies in slot (k - len + t) % W.
 *
 * One new clip for each of n DISTINCT cameras: feats (n, ncrops, C) fp32, cam_ids int32 (n,) on the device.  For c = cam_ids[i]
 * and slot = counts[c] % W: ring[c, k, slot, :C] = feats[i, k] bit for bit and ring[c, k, slot, C] = the row's L2 magnitude by
 * advhip_add_magnitude_np_f32's rule (numpy's bits; C <= 8192, a larger C is refused); a second launch of the same call then
 * does counts[c] += 1.  An id outside [0, n_cam) writes nothing and advances nothing (the kernels check it).  The same id twice
 * in one call is the caller's error: the two clips land in one slot and the count advances by one. */
int advhip_ring_push_f32(const float* feats, const int32_t* cam_ids, float* ring, int64_t* counts, int32_t n, int32_t n_cam,
                         int32_t ncrops, int32_t W, int32_t C, void* stream);
/* The windows of the nb listed cameras as a padded batch: for c = cam_ids[v] and len = min(counts[c], W, Tmax),
 * dst[v, k, t, :] = the camera's entry t of its last len (the slot rule) for t < len, dst (nb, ncrops, Tmax, C1) fp32 with
 * C1 = C + 1.  Rows t >= len are left as they are (advhip_pack_padded_f32's contract); a camera at count 0 or an id outside
 * [0, n_cam) writes nothing.  A copy of bits by 4-byte accesses: rows of C1 = 2049 floats start at 4-byte boundaries only. */
int advhip_ring_windows_f32(const float* ring, const int64_t* counts, const int32_t* cam_ids, float* dst, int32_t nb, int32_t n_cam,
                            int32_t ncrops, int32_t W, int32_t Tmax, int32_t C1, void* stream);
/* latest[cam_ids[v]] = (sum_k scores[(v * ncrops + k) * Tmax + lens[v] - 1]) / ncrops: the crop mean of the newest clip of
 * listed camera v, by advhip_crop_mean_scatter_f32's rule (crop order from 0.f, one division: its bits).  lens int32 (nb,) in
 * 1 .. Tmax and cam_ids int32 (nb,), distinct, index `latest`: the caller has validated both.  Nothing else of latest is written. */
int advhip_crop_mean_last_f32(const float* scores, const int32_t* lens, const int32_t* cam_ids, float* latest, int32_t nb,
                              int32_t ncrops, int32_t Tmax, void* stream);

/* --- live frames: per-camera rings of resized uint8 frames, due clips gathered on the device -------
 * State owned by the caller, all on the device: ring uint8 (n_cam, R, frame_bytes) = every camera's last R frames (resized,
 * packed RGB: frame_bytes = FH * FW * 3), counts int64 (n_cam,) = the frames pushed so far per camera.  R = frames_per_clip *
 * frame_step is the span of a clip.
 * THE SLOT RULE: the frame pushed when a camera's count is k lies in slot k % R.
 * THE WINDOW RULE: a camera at count k >= R has a window of frames_per_clip entries, oldest first; entry t is frame number
 * k - R + t * frame_step of the camera's series and lies in slot (k + t * frame_step) % R.
 * THE DUE RULE (the host's, no kernel knows it): a clip is due after the push that brings a camera's count to k iff k >= R and
 * (k - R) % clip_stride == 0, 1 <= clip_stride <= R.  It is window w = (k - R) / clip_stride of the camera's series taken as an
 * offline video: frames[w * clip_stride : w * clip_stride + R : frame_step], byte for byte.  No LoopPad runs live: a camera
 * below R frames has no clip.
 *
 * Both calls are copies of bits in advhip_gather_batch_f32's form (a frame cut into chunks, all of a lane's loads before its
 * stores, 64-bit byte offsets).  The access width is chosen from both data pointers and frame_bytes: 16 bytes when all three
 * are multiples of 16 (the working frame is: 256 * 340 * 3 = 261 120), 4 bytes when multiples of 4, else single bytes; never
 * an unaligned wide access.  Null pointers, non-positive sizes and more than 65 535 frame rows in one launch are refused.
 *
 * One new frame for each of n DISTINCT cameras: frames uint8 (n, frame_bytes) contiguous, cam_ids int32 (n,) on the device.  For
 * c = cam_ids[i]: ring[c, counts[c] % R] = frames[i]; a second launch of the same call then does counts[c] += 1.  An id outside
 * [0, n_cam) writes nothing and advances nothing.  The same id twice in one call is the caller's error. */
int advhip_frame_ring_push_u8(const uint8_t* frames, const int32_t* cam_ids, uint8_t* ring, int64_t* counts, int32_t n, int32_t n_cam,
                              int32_t R, int64_t frame_bytes, void* stream);
/* The windows of the nb listed cameras as back-to-back clips: dst uint8 (nb * frames_per_clip, frame_bytes); rows
 * [v * frames_per_clip, (v + 1) * frames_per_clip) are the window of c = cam_ids[v] by the window rule.  The rows of a camera
 * whose count is below R, or whose id is outside [0, n_cam), are left as they are.  R != frames_per_clip * frame_step is refused. */
int advhip_frame_ring_windows_u8(const uint8_t* ring, const int64_t* counts, const int32_t* cam_ids, uint8_t* dst, int32_t nb,
                                 int32_t n_cam, int32_t R, int64_t frame_bytes, int32_t frames_per_clip, int32_t frame_step,
                                 void* stream);

/* --- live frames: motion gate -- a still camera's due window repeats its previous clip --------------
 * THE RULE.  Two numbers: pixel_delta (tau, 0 .. 255) and limit (changed bytes a still frame may have, 0 .. frame_bytes).
 * State owned by the caller, per camera, on the device: an anchor frame uint8 (frame_bytes) and one row int32[4] =
 * {still, epoch, changed, peak}, which starts as {-1, 0, -1, 0}.  For every pushed frame f of camera c (at ring size):
 *   1. n = the number of byte positions i with |f[i] - anchor[i]| > tau, compared as integers: both signs count, |d| == tau
 *      is not changed.
 *   2. still == -1 (no anchor yet) or n > limit: the frame MOVES.  anchor := f, still := 0, epoch += 1 (it wraps at 2^32),
 *      peak := 0, changed := n, or -1 where there was no anchor.
 *   3. otherwise the frame is STILL: still := min(still + 1, 2^30), changed := n, peak := max(peak, n); the anchor stays.
 * A due window of span R is QUIET iff still + 1 >= R: all R frames under it lie within the tolerance of one anchor frame.
 * The decision (the host's, from a read-back of {still, epoch}; no kernel knows it), with ref_epoch[c] (or none) and holds[c]:
 * a quiet window is HELD iff ref_epoch[c] == epoch and (max_hold is none or holds[c] < max_hold), then holds[c] += 1; an
 * extracted quiet window does ref_epoch[c] := epoch, holds[c] := 0; an extracted window that is not quiet does ref_epoch[c] :=
 * none, holds[c] := 0.  So the first quiet window after any motion is always extracted -- it is the reference of the still
 * scene --, only later quiet windows under the same anchor repeat it, a clip that contains motion is never repeated, and slow
 * drift, measured against the fixed anchor, eventually moves.  A reset does still := -1, epoch += 1.
 *
 * One update for each of n DISTINCT cameras, n <= n_cam: frames uint8 (n, frame_bytes), cam_ids int32 (n,), anchor uint8
 * (n_cam, frame_bytes), state int32 (n_cam, 4), scratch int32 of at least n_cam * ceil(frame_bytes / 1024) entries (the chunks
 * of a frame at single-byte accesses; its contents mean nothing between calls).  Three launches, integers only, no atomics:
 * every workgroup stores the count of its chunk, one workgroup per frame adds them and applies steps 2 and 3, a predicated
 * copy in advhip_frame_ring_push_u8's form moves the anchor.  The access width is chosen as there, from frames, anchor and
 * frame_bytes.  An id outside [0, n_cam) writes nothing.  frame_bytes < 2^31; the rings and counts are not touched. */
int advhip_frame_gate_update_u8(const uint8_t* frames, const int32_t* cam_ids, uint8_t* anchor, int32_t* state, int32_t* scratch,
                                int32_t n, int32_t n_cam, int64_t frame_bytes, int32_t pixel_delta, int32_t limit, void* stream);
/* Holding: the newest clip of each of n DISTINCT cameras again.  For c = cam_ids[i] with counts[c] >= 1, every crop's row of C1
 * floats, magnitude channel included, is copied bit for bit from slot (counts[c] - 1) % W to slot counts[c] % W of ring (n_cam,
 * ncrops, W, C1) (one wavefront per row; at W == 1 the two are one slot and nothing is copied); a second launch then does
 * counts[c] += 1.  A camera at count 0 or an id outside [0, n_cam) writes nothing and advances nothing. */
int advhip_ring_repeat_f32(const int32_t* cam_ids, float* ring, int64_t* counts, int32_t n, int32_t n_cam, int32_t ncrops, int32_t W,
                           int32_t C1, void* stream);

/* Clip pre-processing on the device: uint8 frames (N, T, C, H, W) -> fp32 (N, C, T, H, W) with
 * y = (x - mean) / std.  Replaces PILToTensor().float() + GroupNormalize(114.75, 57.375)
 * (src/dataset.py:175-183) and the permute of extract_features.py:83, so that only uint8 pixels
 * cross PCIe.  H*W must be a multiple of 4. */
int advhip_normalize_permute_u8(const uint8_t* x, float* y, int64_t N, int32_t T, int32_t C,
                                int32_t H, int32_t W, float mean, float stdv, void* stream);

/* The whole clip pre-processing after the resize, on the device: TenCrop (four corners + centre, then the same five of
 * the horizontally flipped frame: src/gtransforms.py:20-26 -> torchvision.transforms.TenCrop), PILToTensor().float(),
 * (x - mean) / std (src/gtransforms.py:57-73), LoopPad(frames_per_clip) (src/gtransforms.py:115-132) and the permutes
 * of src/dataset.py:195 + extract_features.py:83.
 *   frames: uint8 (F, H, W, C), the resized frames as decoded (HWC);  y: fp32 (ceil(F / fpc) * 10, C, fpc, crop, crop),
 *   row = clip * 10 + crop index.  Only the resized uint8 frames cross PCIe: 1/23 of the fp32 ten-crop bytes. */
int advhip_tencrop_normalize_u8(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                int32_t frames_per_clip, int32_t crop, float mean, float stdv, void* stream);
/* Dense extraction: the same pass over overlapping windows.  Window w = frames [w * clip_stride, w * clip_stride +
 * frames_per_clip), 1 <= clip_stride <= frames_per_clip; n = 1 + max(0, ceil((F - frames_per_clip) / clip_stride)) windows; only
 * the last can be short (len = F - (n - 1) * clip_stride frames) and reads frame (n - 1) * clip_stride + t % len (LoopPad).
 * y: fp32 (n * 10, C, fpc, crop, crop).  No frame is duplicated in memory: the stride is part of the index arithmetic.
 * clip_stride = frames_per_clip is the call above. */
int advhip_tencrop_normalize_u8_strided(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                        int32_t frames_per_clip, int32_t clip_stride, int32_t crop, float mean, float stdv,
                                        void* stream);
/* The same pass for a crop SUBSET: `ncrops` (1..10) strictly ascending TenCrop indices, entry j in bits [4 j, 4 j + 4) of
 * `crops_packed`, the bits above zero (10, 0x9876543210 = the call above).  y: fp32 (n * ncrops, C, fpc, crop, crop), row
 * clip * ncrops + j = row clip * 10 + entry j of the ten-crop pass, bit for bit.  A malformed set is refused before the launch. */
int advhip_tencrop_normalize_u8_crops(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                      int32_t frames_per_clip, int32_t clip_stride, int32_t crop, int32_t ncrops, uint64_t crops_packed,
                                      float mean, float stdv, void* stream);
/* Temporal sampling: frame t of window w is frames[w * clip_stride + t * frame_step] -- every frame_step-th frame of a span of
 * frames_per_clip * frame_step frames.  frame_step >= 1, 1 <= clip_stride <= frames_per_clip * frame_step (above it frames would
 * lie in no span); n = 1 + max(0, ceil((F - frames_per_clip * frame_step) / clip_stride)) windows; only the last can be short:
 * len = min(frames_per_clip, ceil((F - (n - 1) * clip_stride) / frame_step)) sampled frames, and frame t >= len is
 * frames[(n - 1) * clip_stride + (t % len) * frame_step] (LoopPad).  Row w = the row of the call above for those sampled frames
 * as a one-clip video, bit for bit; frame_step = 1 is the call above.  Refused (ADVHIP_EINVAL) before the launch. */
int advhip_tencrop_normalize_u8_sampled(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                        int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop, int32_t ncrops,
                                        uint64_t crops_packed, float mean, float stdv, void* stream);

/* --- normalisation modes of the two TenCrop passes (src/gtransforms.py:57-112) ---
 * ADVHIP_NORM_STANDARDIZE:    y = (x - mean[c]) / std[c]                 (GroupStandardizationTenCrop with per-channel lists)
 * ADVHIP_NORM_PIXEL_MINMAX:   y = (x - mn) / (mx - mn) * r + lo           (GroupPixelMinmaxTenCrop: mn, mx over all C * crop * crop
 *                                                                          values of the (frame, crop); r = float(hi - lo), the
 *                                                                          subtraction in double)
 * ADVHIP_NORM_CHANNEL_MINMAX: the same with mn, mx, lo, r per channel     (GroupRGBChannelMinmaxTenCrop: r[c] = float(hi[c]) -
 *                                                                          float(lo[c]))
 * Every operation is one separately rounded fp32 operation (no FMA, a true division).  A constant crop / channel gives 0 / 0 = NaN,
 * as the reference does; nothing is guarded.  The backbone hands it on as torch does -- NaN in, NaN out, confined to its crop-clip: the
 * ReLU (activation code 1) and the window maxima / mean of every conv epilogue propagate NaN, and no other sample of a launch changes. */
#define ADVHIP_NORM_STANDARDIZE 0
#define ADVHIP_NORM_PIXEL_MINMAX 1
#define ADVHIP_NORM_CHANNEL_MINMAX 2

/* The statistics of the min-max modes.  frames: resized uint8 (F, H, W, C).  stats: uint8 (ceil(F / frame_pitch), 6, C, 2) =
 * (min, max) per channel of the six windows that hold the pixels of TenCrop's ten crops -- top-left, top-right, bottom-left,
 * bottom-right, centre (the Python-rounded half offsets of the passes) and the centre of the mirrored frame, whose left edge is
 * W - crop - (the centre's): the centre's own only where W - crop is even -- of frames 0, frame_pitch, 2 frame_pitch, ...
 * Crop j < 5 reads window j, a mirrored corner 5..8 the opposite corner's window (j - 5) ^ 1, crop 9 window 5.
 * Integer min / max on the bytes: exact, no atomics, the same bits on every run.  The pixel mode reduces the C pairs at look-up. */
int advhip_crop_minmax_u8(const uint8_t* frames, uint8_t* stats, int32_t F, int32_t H, int32_t W, int32_t C, int32_t crop,
                          int32_t frame_pitch, void* stream);

/* advhip_tencrop_normalize_u8_sampled / advhip_tencrop_normalize_planes_u8_sampled with a mode: the same rows, layouts, LoopPad
 * rule, crop sets and frame addressing.  a, b: HOST triples of doubles, (mean, std) or (lo, hi) per channel as the caller states
 * them (C <= 3; channel c reads entry c).  stats / stats_pitch: the table above for the min-max modes (ignored by
 * ADVHIP_NORM_STANDARDIZE); stats_pitch must divide clip_stride and frame_step, so that every sampled frame is one the table
 * holds -- frame f reads entry f / stats_pitch, and a LoopPad copy of a frame its statistics.
 * ADVHIP_EINVAL before anything launches: a null pointer, an unknown mode, a zero std, lo >= hi (pixel mode: in any channel;
 * channel mode: in every channel -- the reference's own condition), stats_pitch < 1 or not a divisor, and everything the
 * `_sampled` calls refuse. */
int advhip_tencrop_normalize_u8_modes(const uint8_t* frames, float* y, int32_t F, int32_t H, int32_t W, int32_t C,
                                      int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop, int32_t ncrops,
                                      uint64_t crops_packed, int32_t mode, const double* a, const double* b, const uint8_t* stats,
                                      int32_t stats_pitch, void* stream);
int advhip_tencrop_normalize_planes_u8_modes(const uint8_t* frames, float* xs, int32_t F, int32_t H, int32_t W, int32_t C,
                                             int32_t frames_per_clip, int32_t clip_stride, int32_t frame_step, int32_t crop,
                                             int32_t ncrops, uint64_t crops_packed, int64_t first_crop_clip, int64_t count,
                                             int32_t mode, const double* a, const double* b, const uint8_t* stats,
                                             int32_t stats_pitch, void* stream);

/* Per-window scores (n_windows,) -> per-frame scores (n_frames,): window w covers frames [w * clip_stride, w * clip_stride +
 * frames_per_clip); the score of a frame is the mean of the scores of the windows covering it (fp32, added in ascending window
 * order, one division by their count).  0 < n_frames <= (n_windows - 1) * clip_stride + frames_per_clip.  clip_stride =
 * frames_per_clip gives np.repeat(scores, frames_per_clip) (src/runner.py:66-76) bit for bit.  Every argument is checked before
 * the launch. */
int advhip_frame_scores_f32(const float* scores, float* out, int64_t n_windows, int32_t frames_per_clip, int32_t clip_stride,
                            int64_t n_frames, void* stream);

/* The resize in front of all that: GroupResize(256, Image.BILINEAR) (src/gtransforms.py:9-18, applied in src/dataset.py:175-183),
 * i.e. PIL Image.resize of every decoded frame, byte for byte (Pillow's 8-bit two-pass resampler).
 *   src: uint8 (F, H, W, C) decoded frames, C == 3;  dst: uint8 (F, OH, OW, C).
 *   xbounds int32 (OW, 2) = (first source column, tap count), xcoef int32 (OW, xksize): the horizontal table; ybounds / ycoef /
 *   yksize: the vertical one (source rows as Pillow computes them); coefficients are 2^22 fixed point (resize.py builds them).
 *   The horizontal pass runs iff OW != W and computes source rows [row0, row0 + rows) into ws (uint8 (F, rows, OW, C)), or all
 *   H rows straight into dst when OH == H; the vertical pass runs iff OH != H, from ws (or src).  Neither: dst = a copy of src.
 * Two launches on `stream` at most; every argument is checked before the first. */
int advhip_resize_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F, int32_t H, int32_t W, int32_t C, int32_t OH,
                     int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds,
                     const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, void* stream);
/* The same for every frame_step-th frame: source frames 0, frame_step, 2 frame_step, ... of src (F_src, H, W, C) into a compact
 * dst (ceil(F_src / frame_step), OH, OW, C) -- a source frame pitch in both passes; ws: uint8 (ceil(F_src / frame_step), rows, OW,
 * C), the sampled frames only.  Each output frame is byte for byte the call above's for that source frame; frame_step = 1 is
 * the call above. */
int advhip_resize_u8_sampled(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int32_t H, int32_t W,
                             int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                             const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, void* stream);

/* --- decoded frames as the decoder has them: Y'CbCr 4:2:0 --------------------------------------------------------------------
 * Compact 8-bit frames first (surfaces with a row pitch, plane offsets, NV21 / YV12 and 10-bit samples follow below).
 * A frame is uint8 (3H/2, W), H and W even, row pitch == W: rows [0, H) are Y; NV12 then holds H/2 rows of interleaved (Cb, Cr)
 * pairs, I420 (yuv420p) the (H/2, W/2) Cb plane followed by the (H/2, W/2) Cr plane.  Chroma is nearest: pixel (y, x) uses sample
 * (y >> 1, x >> 1).  The conversion is integer, in int32, with 2^16 fixed-point coefficients passed by value (the library holds
 * no table; resize.py derives them from the luma weights and the range):
 *   yi = cy (Y - yoff) + 2^15
 *   R = clip8((yi + crv (Cr - 128)) >> 16)
 *   G = clip8((yi - cgu (Cb - 128) - cgv (Cr - 128)) >> 16)          (arithmetic shifts)
 *   B = clip8((yi + cbu (Cb - 128)) >> 16)
 * yoff is 16 (limited range) or 0 (full range), 0 < cy < 2^18 and 0 <= every other coefficient < 2^18 (every sum is exact in int32).
 * This is a definition of its own, not swscale's bytes: the RGB entry points above remain the reference-parity path. */
#define ADVHIP_YUV420_NV12 0
#define ADVHIP_YUV420_I420 1

/* The conversion alone: source frames 0, frame_step, 2 frame_step, ... of src (F_src, 3H/2, W) -> packed RGB dst
 * (ceil(F_src / frame_step), H, W, 3).  One launch; a lane converts the two (or four) adjacent pixels that share a chroma
 * sample.  Every argument is checked before the launch. */
int advhip_yuv420_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t F_src, int32_t frame_step, int32_t H, int32_t W, int32_t layout,
                            int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream);
/* advhip_resize_u8_sampled on 4:2:0 source frames (F_src, 3H/2, W): dst is byte for byte what that call makes of the frames the
 * call above converts, and the full-size RGB frames never exist -- the horizontal pass converts each tap's pixel as it reads it
 * (Y row row0 + y, chroma row (row0 + y) >> 1), the vertical pass is the RGB resize's own.  C is the output's channel count (3).
 * ws as there: uint8 (F, rows, OW, 3) when both passes run.  Where no horizontal pass runs (OW == W) the conversion launch runs
 * first: into ws, uint8 (F, H, W, 3), when OH != H, else straight into dst.  Two launches at most, every argument checked first. */
int advhip_resize_yuv420_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int32_t H, int32_t W,
                            int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                            const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0, int32_t rows, int32_t layout,
                            int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream);

/* --- decoder surfaces: 4:2:0 frames described by byte geometry and sample depth ---------------------------------------------
 * What a hardware decoder or an AVFrame hands over, read in place.  A source frame is a run of frame_pitch bytes (source frame f
 * starts at byte f * frame_pitch of src); inside it, with every offset, pitch and step in bytes from the frame's first byte:
 *   luma (y, x)            at y_offset + y * y_pitch + x * sb
 *   Cb of chroma (r, c)    at cb_offset + r * chroma_pitch + c * chroma_step,   Cr the same from cr_offset
 * where sb is the sample size: 1 at bits = 8; 2 at bits = 10, a little-endian 16-bit word whose value is (word >> shift) & 1023
 * (shift 6: P010; shift 0: yuv420p10le; the other bits are ignored).  Pixel (y, x) uses chroma sample (y >> 1, x >> 1).
 * The layouts are nothing but these numbers:  NV12 chroma_step = 2 sb, cr_offset = cb_offset + sb;  NV21 cb_offset = cr_offset +
 * sb;  I420 / YV12 chroma_step = sb with the two planes in either order.
 * Rules (each refused by name before any launch): H and W even and >= 2; bits 8 or 10; shift in [0, 6] and 0 at 8 bits;
 * chroma_step sb or 2 sb, and with 2 sb the two chroma offsets exactly sb apart; y_pitch >= W sb; chroma_pitch >= (W / 2)
 * chroma_step; no negative offset; every plane ends at or before frame_pitch; at 10 bits src, frame_pitch and every offset and
 * pitch are even.
 * The conversion at depth b = bits, with S = 8 + b and 2^S fixed-point coefficients passed by value:
 *   yi = cy (Y - yoff) + 2^(S-1)
 *   R = clip8((yi + crv (Cr - 2^(b-1))) >> S)
 *   G = clip8((yi - cgu (Cb - 2^(b-1)) - cgv (Cr - 2^(b-1))) >> S)      (arithmetic shifts)
 *   B = clip8((yi + cbu (Cb - 2^(b-1))) >> S)
 * yoff is 16 * 2^(b-8) (limited range) or 0 (full range); the coefficient bounds are those above (every sum is below 2^30).  At
 * b = 8 this is the formula above, and the compact frame as a surface gives the bytes of the calls above.
 *
 * The conversion alone, as advhip_yuv420_to_rgb_u8: one launch.  Where the alignment of src, frame_pitch, the offsets, the
 * pitches and dst allows it, a lane converts four pixels from one load of four Y samples; otherwise two. */
int advhip_yuv420_surface_to_rgb_u8(const uint8_t* src, uint8_t* dst, int64_t F_src, int32_t frame_step, int64_t frame_pitch, int32_t H,
                                    int32_t W, int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset,
                                    int64_t cr_offset, int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv,
                                    int32_t cgu, int32_t cgv, int32_t cbu, void* stream);
/* advhip_resize_yuv420_u8 on surfaces: dst is byte for byte advhip_resize_u8_sampled of what the call above converts.  ws, the
 * tables and the launches are as there. */
int advhip_resize_yuv420_surface_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int32_t frame_step, int64_t frame_pitch,
                                    int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef,
                                    int32_t xksize, const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, int32_t row0,
                                    int32_t rows, int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset,
                                    int64_t cr_offset, int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv,
                                    int32_t cgu, int32_t cgv, int32_t cbu, void* stream);

/* --- regions of interest: a source box per output frame (PIL Image.resize(size, resample, box=)) ----------------------------
 * The three resize entry points above with a table set per output frame.  resize.py (box_coefficients, roi_tables) builds one
 * set per box -- Pillow's precompute_coeffs with the box held as C floats -- and stacks n_tables of them, every axis padded with
 * zero coefficients to the largest ksize of that axis:
 *   xbounds int32 (n_tables, OW, 2), xcoef int32 (n_tables, OW, xksize), ybounds int32 (n_tables, OH, 2), ycoef int32 (n_tables,
 *   OH, yksize);  rowspan int32 (n_tables, 2) ON THE DEVICE = (row0, rows): the source rows table t's vertical pass reads, i.e.
 *   the rows its horizontal pass computes;  ws_rows = the largest `rows`, 1 <= ws_rows <= H.
 * Output frame i < N reads source frame src_of[i] (src_of int32 (N,) on the device; null: frame i * frame_step, and then
 * (N - 1) * frame_step < F_src) with table table_of[i] (int32 (N,) on the device; null: table 0 for every frame).  Both passes
 * always run (an axis Pillow would skip carries the identity table: bounds (i, 1), coefficient 2^22), so there are exactly two
 * launches: the horizontal pass writes rows [0, rows) of frame i's slab of ws, uint8 (N, ws_rows, OW, 3), the vertical pass reads
 * them.  dst uint8 (N, OH, OW, C), C == 3, frame i byte for byte Pillow's box resize of its source frame.
 * An output frame whose source index is outside [0, F_src) or whose table index is outside [0, n_tables) is not written and
 * nothing is read for it.  Every argument the host can see is checked before the first launch; a rowspan entry outside the frame
 * or above ws_rows cannot be (it is device memory): the kernels then count no taps for that table, as for a foreign bounds entry. */
int advhip_resize_roi_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of, int32_t frame_step,
                         const int32_t* table_of, int32_t n_tables, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW,
                         const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds, const int32_t* ycoef,
                         int32_t yksize, const int32_t* rowspan, int32_t ws_rows, void* stream);
/* The same from compact 4:2:0 frames (F_src, 3H/2, W), converted tap by tap as in advhip_resize_yuv420_u8. */
int advhip_resize_roi_yuv420_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of,
                                int32_t frame_step, const int32_t* table_of, int32_t n_tables, int32_t H, int32_t W, int32_t C, int32_t OH,
                                int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize, const int32_t* ybounds,
                                const int32_t* ycoef, int32_t yksize, const int32_t* rowspan, int32_t ws_rows, int32_t layout, int32_t yoff,
                                int32_t cy, int32_t crv, int32_t cgu, int32_t cgv, int32_t cbu, void* stream);
/* The same from decoder surfaces, with the geometry and the rules of advhip_resize_yuv420_surface_u8. */
int advhip_resize_roi_surface_u8(const uint8_t* src, uint8_t* dst, uint8_t* ws, int64_t F_src, int64_t N, const int32_t* src_of,
                                 int32_t frame_step, const int32_t* table_of, int32_t n_tables, int64_t frame_pitch, int32_t H, int32_t W,
                                 int32_t C, int32_t OH, int32_t OW, const int32_t* xbounds, const int32_t* xcoef, int32_t xksize,
                                 const int32_t* ybounds, const int32_t* ycoef, int32_t yksize, const int32_t* rowspan, int32_t ws_rows,
                                 int32_t bits, int32_t shift, int64_t y_offset, int64_t y_pitch, int64_t cb_offset, int64_t cr_offset,
                                 int64_t chroma_pitch, int32_t chroma_step, int32_t yoff, int32_t cy, int32_t crv, int32_t cgu, int32_t cgv,
                                 int32_t cbu, void* stream);

/* Weighted ROC counts: what the frame-level ROC / PR curves of src/runner.py:62-79 are made of, from one item per clip.
 *   scores fp32 (M,), pos / neg int32 (M,) non-negative weights (the positive / negative frames an item stands for), 1 <= M < 2^31.
 *   thresholds fp32 (M,), tps / fps int64 (M,), meta int64 (4,) = {G, non-finite scores, sum of pos, sum of neg}.
 * Entry g < G is the g-th distinct score in descending order: thresholds[g] is that score (a copy of one of the inputs that carry
 * it), tps[g] / fps[g] the sums of pos / neg over all items whose score is >= it; entries [G, M) are not written.  Two scores
 * are one entry iff they are equal as floats (np.diff(float64(s)) != 0): -0.0 and +0.0 are one entry (either sign may come
 * back), denormals are values of their own.  An item with pos = neg = 0 still makes, or joins, the entry of its score.
 * NaN / +-inf scores are counted into meta[1]; when that is not zero the rest of the output is unspecified (every write stays
 * inside the arrays).  All sums are int64; every result is an integer or a copied input, the same for every run.
 * Method: uint32 keys whose ascending order is the floats' descending one, a stable LSD radix sort of (key, item) in four 8-bit
 * passes (tile histograms, a scan of the (digit, tile) table, a stable scatter), then an int64 scan of (pos, neg, group end)
 * over the sorted order that writes one entry per group end.  Multi-block scans are reduce / scan of the partials / apply as
 * separate launches: no workgroup waits on another.  One 32-byte memset and 14 to 36 launches on `stream` (24 at M = 70 000);
 * nothing synchronises.  workspace: advhip_roc_counts_ws_bytes(M) bytes (ADVHIP_EINVAL for an M outside the range), 8-byte aligned,
 * scratch only.  Null pointers, M < 1 and a short workspace: ADVHIP_EINVAL before anything is launched. */
int64_t advhip_roc_counts_ws_bytes(int64_t M);
int advhip_roc_counts(const float* scores, const int32_t* pos, const int32_t* neg, int64_t M, float* thresholds, int64_t* tps,
                      int64_t* fps, int64_t* meta, void* workspace, int64_t workspace_bytes, void* stream);

/* Anomaly events from per-frame scores: smoothing, two thresholds with hysteresis, gap merge, minimum length, event list.
 * The input is a ragged batch of V videos flattened into N = offsets[V] positions, 1 <= N < 2^31: video v is
 * [offsets[v], offsets[v + 1]) (offsets: device int64 (V + 1,), non-decreasing from 0 to N; a length of 0 is allowed and gives no
 * events).  No step looks across a video boundary.  The rule, for a video x of L frames:
 *   1. smooth   window w odd, 1 <= w <= 1023, h = (w - 1) / 2: y[t] = (sum of x[u], u = max(0, t - h) .. min(L - 1, t + h)) / count,
 *               the sum in fp32 in ascending u starting from +0.0f, one fp32 division by the count (advhip_frame_scores_f32's
 *               convention).  w = 1 returns x's bits, except that -0.0 becomes +0.0.  NaN and +-inf propagate as IEEE does.
 *   2. flags    active[t] = y[t] >= low, strong[t] = y[t] >= high; a NaN is neither, -0.0 >= 0.0 is true.  low <= high, both finite.
 *   3. candidates  maximal runs of active frames; two runs separated by at most merge_gap frames that are not active are one
 *               candidate, as a chain (merge_gap >= 0, 0: no merging).  Equivalently: frame t starts a candidate iff it is active
 *               and no frame of [t - merge_gap - 1, t - 1] inside its video is, and ends one by the mirror image.
 *   4. keep     a candidate iff it holds a strong frame and end - start >= min_len (min_len >= 1).
 *   5. record   in (video, start) order: video, start, end (frames local to the video, end exclusive), peak (the largest y of the
 *               interval, NaN ignored: a copied float), peak_frame (the first frame whose y equals the peak), mean (the float64
 *               sum of y[start:end] divided by the length, rounded to fp32; the frames of merged gaps are included, so a NaN
 *               there gives a NaN mean).
 * advhip_smooth_scores_f32 is step 1: out fp32 (N,), not the scores themselves.  One launch.
 * advhip_score_events is steps 2 to 5 on the smoothed scores: ev_int int32 (cap, 4) = {video, start, end, peak_frame}, ev_f fp32
 * (cap, 2) = {peak, mean}, counts int32 (V,) = events per video, meta int64 (2,) = {events found, events written = min(found,
 * cap)}; rows from meta[1] on are not written.  cap = sum of ceil(L_v / 2) holds every possible result (merge_gap = 0, min_len = 1,
 * every second frame active).  Every output is an integer, a copied float, or a sum in a fixed order: the same bits in every run
 * (the float64 sum of an event: 64 strided partial sums in ascending frame order, then a fixed tree over them).
 * Method: exclusive max-scans of (active ? position : -1) forward and over the reversed order give the nearest active frame on
 * either side, whose apply step writes the start / end marks; a scan of the marks numbers the candidates; one wave per candidate
 * reduces it in a loop; a scan of the keep flags compacts the events.  Multi-block scans are reduce / scan of the partials /
 * apply as separate launches: no workgroup waits on another.  One memset of counts and 5 to 21 launches on `stream` (13 at
 * N = 2^20); nothing synchronises.  workspace: advhip_score_events_ws_bytes(N, V) bytes (about 16 N), 8-byte aligned, scratch only.
 * Refused with ADVHIP_EINVAL before anything is launched: null pointers, N outside [1, 2^31), V < 1, an even window or one
 * outside [1, 1023], low > high or a threshold that is not finite, merge_gap < 0, min_len < 1, cap < 1, a short workspace.  The
 * offsets are read on the device only; whatever they hold, no access leaves the arrays. */
int advhip_smooth_scores_f32(const float* scores, const int64_t* offsets, int64_t V, int64_t N, int32_t window, float* out, void* stream);
int64_t advhip_score_events_ws_bytes(int64_t N, int64_t V);
int advhip_score_events(const float* smoothed, const int64_t* offsets, int64_t V, int64_t N, float low, float high, int32_t merge_gap,
                        int32_t min_len, int32_t* ev_int, float* ev_f, int64_t cap, int32_t* counts, int64_t* meta, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* --- live events: the rule above, streaming, with state per camera ----------------------------------------------------------
 * A camera's series x[0 .. n) holds one sample per call that lists it (a clip score of live scoring: advhip_crop_mean_last_f32's
 * `latest`).  With h = (smooth - 1) / 2, y[t] is final once sample t + h has been fed, and is step 1's y[t] of any longer series
 * (the window [max(0, t - h), t + h], fp32 ascending from +0.0f, one division); every update finalises at most one y.  Over the
 * final y in order: an active sample (y >= low) opens a candidate or extends the open one; an inactive sample at t closes it when
 * t - last_active > merge_gap; a NaN is neither active nor strong.  In an open candidate: strong = any y >= high; peak = the
 * largest y of an active sample and peak_frame its first position; a float64 running sum of every final y since start (gap
 * samples included, ascending from 0.0) is copied at each active sample.  On close: end = last_active + 1, mean = (float)(copy /
 * (double)(end - start)); a closed candidate that is strong with end - start >= min_len is an event, steps 4 and 5 of the rule.
 * THE EMISSION RULE: the event [s, e) is written by the update that brings the camera's sample count to e + merge_gap + h + 1; a
 * camera emits at most one event per update.  Emitted events plus what finish closes are the offline rule's events of the whole
 * series: integers and peak bits equal, the mean the ascending float64 sum (within one fp32 ulp of advhip_score_events').
 *
 * State, all on the device, owned and zero-initialised by the caller except where stated:
 *   ring        fp32  (n_cam, smooth)   the last `smooth` samples, sample k in slot k % smooth
 *   samples     int64 (n_cam,)          samples fed since the last finish / reset (below 2^31: positions are int32)
 *   cand_int    int32 (n_cam, 5)        {start (-1: no candidate is open; initialise to -1), last_active, peak_frame, strong,
 *                                        generation}; the three fields in the middle are -1, -1, 0 while nothing is open
 *   cand_peak   fp32  (n_cam,)          the open candidate's peak (0 while nothing is open)
 *   cand_sum    fp64  (n_cam, 2)        {running sum, its copy at last_active} (0 while nothing is open)
 *   alert       int32 (n_cam,)          1 iff a candidate is open, strong, and last_active + 1 - start >= min_len
 *   open_start  int32 (n_cam,)          the open candidate's start, or -1 (initialise to -1)
 *   log_int     int32 (n_cam, K, 4)     {generation, start, end, peak_frame}; event number j of a camera lies in slot j % K
 *   log_f       fp32  (n_cam, K, 2)     {peak, mean}
 *   emitted     int64 (n_cam,)          events written so far (never reset: the log keeps the last K)
 * alert and open_start describe the final part of the curve: they trail the newest sample by h (smooth = 1: no delay).
 *
 * One launch for nb DISTINCT listed cameras (cam_ids int32 (nb,) on the device), one wavefront per camera (the ring row staged in
 * LDS, one lane runs the ordered sum and the state machine): no atomics, no workgroup waits on another, the same bits in every
 * run.  mode ADVHIP_LIVE_EVENTS_UPDATE: one new sample each, scores[cam_ids[v]] when by_camera is 1 (scores fp32 (n_cam,)), else
 * scores[v] (scores fp32 (nb,)).  ADVHIP_LIVE_EVENTS_FINISH: the pending min(h, n) samples are finalised with windows clipped at
 * n - 1 (a loop of at most h steps), the open candidate is closed and emitted if it qualifies, then the camera is cleared: samples
 * 0, generation + 1, nothing open.  ADVHIP_LIVE_EVENTS_RESET: cleared the same way without finalising or emitting.  scores is
 * not read by the last two (it may be null).  Only the listed cameras' state is written; an id outside [0, n_cam), or a camera
 * whose samples lie outside [0, 2^31 - 1) (finish / reset: [0, 2^31 - 1]) or whose emitted is negative, writes nothing; every log
 * index is bounded by K.  The same id twice in one call is the caller's error.
 * Refused with ADVHIP_EINVAL before anything is launched: null pointers, an unknown mode, nb < 1, n_cam < 1, K < 1, an even smooth
 * or one outside [1, 1023], merge_gap < 0, min_len < 1, a threshold that is not finite, low > high, by_camera not 0 or 1. */
#define ADVHIP_LIVE_EVENTS_CAND_INTS 5
#define ADVHIP_LIVE_EVENTS_UPDATE 0
#define ADVHIP_LIVE_EVENTS_FINISH 1
#define ADVHIP_LIVE_EVENTS_RESET 2
int advhip_live_events_update_f32(const float* scores, const int32_t* cam_ids, float* ring, int64_t* samples, int32_t* cand_int,
                                  float* cand_peak, double* cand_sum, int32_t* alert, int32_t* open_start, int32_t* log_int,
                                  float* log_f, int64_t* emitted, int32_t nb, int32_t n_cam, int32_t K, int32_t smooth, float low,
                                  float high, int32_t merge_gap, int32_t min_len, int32_t by_camera, int32_t mode, void* stream);

/* --- which kernel form a scorer launch takes ---------------------------------------------------------------------------------
 * The normalisation and depth-wise entry points above each pick one of several kernels from the channel count, the row length
 * and the alignment of their operands.  These are those rules, as pure host functions that the launchers themselves call: the
 * answer IS the kernel the launch runs.  Nothing is launched and no pointer is read.  `aligned16` (0 / 1): whether every operand
 * the launcher looks at starts on a 16-byte boundary --
 *   bn_rows fwd: x, y;  bwd: dy, x, dx, add
 *   chan_layernorm fwd: x, y, mu, rs;  bwd: dy, x, dx, mu, rs, add
 *   head_ln_fc fwd: y, xn, mean, rstd, score;  bwd: y, d_xn, d_score, mean, rstd, score, dy
 *   dwconv_t fwd: v, out;  bwd: dout, v, dv           (a null operand counts as aligned).
 * advhip_chan_stats_f32 and advhip_dwconv_t_fwd_lens_f32 have one form each and no query. */
#define ADVHIP_BN_ROWS_GENERIC 0    /* three reads of the row, any N */
#define ADVHIP_BN_ROWS_REG256X4 1   /* the row resident in registers: 256 threads x 4 float4, N <= 4 096 */
#define ADVHIP_BN_ROWS_REG256X12 2  /* 256 threads x 12 float4, N <= 12 288 */
#define ADVHIP_BN_ROWS_REG1024X4 3  /* 1 024 threads x 4 float4, N <= 16 384, fewer than 512 rows */
int32_t advhip_bn_rows_form(int32_t C, int64_t N, int32_t aligned16);
/* 0 = the generic kernel, otherwise the channels per thread of the 16-byte form (1, 2 or 16: C = 64, 128, 1 024) */
int32_t advhip_chan_layernorm_form(int32_t C, int64_t N, int32_t aligned16);
/* 0 = the generic kernel, 1 = the 16-byte form (C = 1 024) */
int32_t advhip_head_ln_fc_form(int32_t C, int64_t N, int32_t aligned16);
/* 0 = one element per thread, 1 = four consecutive t per thread (T % 4 == 0); the same rule forward and backward, K = 3 and 5 */
int32_t advhip_dwconv_t_form(int32_t T, int32_t aligned16);

/* The pooling launchers' rules, in the same way.  advhip_maxpool3d_strided_f32 (and advhip_maxpool3d_f32, which is it with a dense
 * y) picks its kernel from the row length W, the window and the stride, and from `y_padded` (0 / 1): whether y_batch_stride leaves
 * elements between consecutive samples of y (a stride of 0 or of exactly one sample is dense).  advhip_maxpool3d_padded_f32 has
 * one kernel, the generic one, and no query. */
#define ADVHIP_MAXPOOL_GENERIC 0  /* one thread per output element, any window, stride and padding */
#define ADVHIP_MAXPOOL_ROW233 1   /* k(2,3,3) s(2,2,2) on even rows of <= 128 floats (fewer than 64 outputs): one wavefront per output row */
#define ADVHIP_MAXPOOL_TEMPORAL 2 /* k(kt,1,1) s(st,1,1) into a dense y: four outputs per thread */
int32_t advhip_maxpool3d_form(int32_t W, int32_t kt, int32_t kh, int32_t kw, int32_t st, int32_t sh, int32_t sw, int32_t y_padded);
/* advhip_global_avgpool_f32: 1 = rows of n <= 128 positions, added as two 64-lane butterflies; 0 = longer rows, lanes stride the row */
int32_t advhip_global_avgpool_form(int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* ADVHIP_H */
