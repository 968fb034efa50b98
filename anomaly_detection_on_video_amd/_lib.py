"""ctypes binding of libadvhip.so (include/advhip.h).

The shared library is built in-tree by `anomaly_detection_on_video_amd.build` (hipcc,
--offload-arch=gfx950) and is the ONLY compute path of this package for the ops it covers:
there is no eager / CPU fallback.  If the library is missing, or a tensor is not on a GPU, the
callers raise -- loudly -- instead of silently computing somewhere else.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libadvhip.so")

ALGO_AUTO = 0
ALGO_IGEMM_128x128 = 1
ALGO_IGEMM_128x64 = 2
ALGO_IGEMM_64x64 = 3
ALGO_IGEMM_64x128 = 4
ALGO_IGEMM_128x128x32 = 5
ALGO_IGEMM_128x64x32 = 6
ALGO_IGEMM_64x64x32 = 7
ALGO_IGEMM_64x128x32 = 8
ALGO_IGEMM_256x64 = 9  # 256 x 64 x 16, four waves stacked along M; the 2-deep LDS-DMA family only
ALGO_FAST_BASE = 32  # + tile id: scalar-offset / tap-mask gather (<= 32 taps)
IGEMM_ALGOS = (1, 2, 3, 4, 5, 6, 7, 8)
FAST_ALGOS = tuple(ALGO_FAST_BASE + a for a in IGEMM_ALGOS)
ALGO_DMA_BASE = 64  # + tile id: fast gather + LDS-DMA staging into a 3-deep ring (no 128x128x32)
DMA_ALGOS = tuple(ALGO_DMA_BASE + a for a in (1, 2, 3, 4, 6, 7, 8))
ALGO_DMA4_BASE = 96  # + tile id 2..4: 4-deep ring
DMA4_ALGOS = tuple(ALGO_DMA4_BASE + a for a in (2, 3, 4))
ALGO_BF16X3_BASE = 128  # + tile id 5 (128x128x32) / 6 (128x64x32): opt-in split-bf16 arithmetic (3 bf16 MFMAs per fragment)
BF16X3_ALGOS = tuple(ALGO_BF16X3_BASE + a for a in (5, 6))
ALGO_DMA2_BASE = 160  # + tile id: LDS-DMA kernel, 2-deep ring (less LDS, more resident workgroups)
DMA2_ALGOS = tuple(ALGO_DMA2_BASE + a for a in (1, 2, 3, 4, 6, 7, 8, 9))
ALGO_TSPAN_128x64 = 192  # (kt,1,1) convs: 128x64 tile of 2 or 4 frames x flattened spatial positions
ALGO_MIXED_128x64 = 200  # unsplit 1x1x1 stride-1 convs: 128x64 tiles + 64x64 tiles for the last, partial round of workgroups
ALGO_TFOLD_BASE = 208  # + tile id of the 2-deep LDS-DMA family: (kt,1,1) convs on T <= kt//2 + 1 frames as the dense 1x1x1 conv (B, Cin*T, 1, H, W) -> Cout*T
TFOLD_ALGOS = tuple(ALGO_TFOLD_BASE + a for a in (1, 2, 3, 4, 6, 7, 8, 9))
ALGO_PERSIST_BASE = 224  # + tile id (2: 128x64, 3: 64x64) + 8 * (workgroups per CU - 1), 1..3: persistent wave-specialised kernel (opt-in), unsplit 1x1x1 stride-1 convs, K >= 64
PERSIST_ALGOS = tuple(ALGO_PERSIST_BASE + t + 8 * (w - 1) for w in (1, 2, 3) for t in (2, 3))
ALGO_STEM_BORDER = 256  # the planes-form stem + maxpool1 only: launch split by pool window in t, border windows on frame-uniform tiles that skip all-padding k-tiles


NORM_STANDARDIZE, NORM_PIXEL_MINMAX, NORM_CHANNEL_MINMAX = 0, 1, 2  # ADVHIP_NORM_*: the modes of the `_modes` TenCrop passes


def is_tfold(algo: int) -> bool:
    return ALGO_TFOLD_BASE <= algo < ALGO_TFOLD_BASE + 16


FAMILIES = ("generic", "fast", "dma3", "dma4", "bf16x3", "dma2", "tspan", "mixed", "persist")  # ADVHIP_FAMILY_* of include/advhip.h, by value


def algo_info(algo: int):
    """(family name, BM, BN, BK) of an implicit-GEMM algorithm id: advhip_conv3d_algo_info (a TFOLD id reports its folded DMA2 launch)."""
    out = [C.c_int32() for _ in range(4)]
    check(load().advhip_conv3d_algo_info(algo, *(C.byref(o) for o in out)), "conv3d_algo_info")
    return (FAMILIES[out[0].value],) + tuple(o.value for o in out[1:])


def algo_tile(algo: int):
    """(BM, BN, BK) of an implicit-GEMM algorithm id, as the library's own table has it (raises for an id without a kernel)."""
    return algo_info(algo)[1:]


class HipExtensionError(RuntimeError):
    pass


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "B", "Cin", "T", "H", "W", "Cout", "kt", "kh", "kw", "st", "sh", "sw", "pt", "ph", "pw",
        "relu", "algo", "splits")]


_P = C.c_void_p
_I = C.c_int32
_L = C.c_int64


class ConvEpilogue(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("y_preact", "dact_z", "ln_u", "ln_mu", "ln_rs", "splitk_counters")] + [("splitk_counter_bytes", C.c_int64)]
                + [("avgpool_out", C.c_void_p)])


class ColsumItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int32), ("period", C.c_int32)]


class AdamItem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("param", "grad", "exp_avg", "exp_avg_sq", "step")] + [("n", C.c_int64)]


class NormItem(C.Structure):
    _fields_ = [("grad", C.c_void_p), ("n", C.c_int64)]


class NtItem(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("A", "B", "C", "rowsum")] + [("M", C.c_int32), ("N", C.c_int32), ("lda", C.c_int64), ("ldb", C.c_int64)]


class GemmDesc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("M", "N", "K", "batch")]
                + [(n, C.c_int64) for n in ("sAb", "sAm", "sAk", "sBb", "sBk", "sBn", "sCb", "sCm", "sCn")]
                + [("alpha", C.c_float), ("beta", C.c_float), ("act", C.c_int32)]
                + [(n, C.c_void_p) for n in ("bias_m", "bias_n", "ln_u", "ln_mu", "ln_rs", "residual")])


# name -> (restype, argtypes); every symbol include/advhip.h declares
SIGNATURES = {
    "advhip_abi_version": (C.c_int, []),
    "advhip_last_error": (C.c_char_p, []),
    "advhip_target_arch": (C.c_char_p, []),
    "advhip_conv3d_out_dims": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "advhip_conv3d_packed_rows": (C.c_int, [C.POINTER(ConvDesc)]),
    "advhip_conv3d_algo_info": (C.c_int, [_I] + [C.POINTER(_I)] * 4),
    "advhip_conv3d_pack_weight_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "advhip_conv3d_pack_weight_bf16x3": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "advhip_conv3d_build_ktab": (C.c_int, [C.POINTER(ConvDesc), _P, _P]),
    "advhip_conv3d_tfold_desc": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(ConvDesc)]),
    "advhip_conv3d_pack_weight_tfold_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P]),
    "advhip_conv3d_tfold_scale_shift_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P]),
    "advhip_bn_fold_f32": (C.c_int, [_P, _P, _P, _P, C.c_float, _I, _P, _P, _P]),
    "advhip_conv3d_workspace_bytes": (_L, [C.POINTER(ConvDesc)]),
    "advhip_conv3d_bn_act_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _P, _P, _P, _P, _P, _P, _P, _L, _P]),
    "advhip_conv3d_bn_act_strided_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _P, _P, _P, _P, _P, _P, _L, _P, _L, _P]),
    "advhip_conv3d_pool_out_dims": (C.c_int, [C.POINTER(ConvDesc)] + [_I] * 6 + [C.POINTER(_I)] * 3),
    "advhip_conv3d_relu_maxpool233_workspace_bytes": (_L, [C.POINTER(ConvDesc)]),
    "advhip_conv3d_active_ktiles": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _P, _P]),
    "advhip_conv3d_bn_relu_maxpool233_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _P, _P, _P, _P, _P, _L, _P, _L, _P]),
    "advhip_split_w_plane_floats": (_I, [_I]),
    "advhip_split_w_f32": (C.c_int, [_P, _P, _L, _I, _P]),
    "advhip_conv3d_s2w_build_ktab": (C.c_int, [C.POINTER(ConvDesc), _P, _P]),
    "advhip_conv3d_s2w_bn_relu_maxpool233_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _P, _P, _P, _P, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_table_sizes": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "advhip_conv3d_u8_build_tables": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _P, C.c_float, _P, _P, _P]),
    "advhip_conv3d_u8_taps_table_sizes": (C.c_int, [C.POINTER(ConvDesc), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "advhip_conv3d_u8_taps_build_tables": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _P, C.c_float, _P, _P, _P, _P]),
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _L, _L, _P, _P, _P, _P, _P,
                                                                       C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _L, _P, _P, _P, _P, _P,
                                                                  C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_strided_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _L, _L, _P, _P, _P, _P, _P,
                                                                               C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_crops_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _I, C.c_uint64, _L, _L, _P, _P, _P,
                                                                             _P, _P, C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_crops_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _I, C.c_uint64, _L, _P, _P, _P, _P,
                                                                        _P, C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_strided_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _L, _P, _P, _P, _P, _P,
                                                                          C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_build_tables_sampled": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _I, _P, C.c_float, _P, _P, _P]),
    "advhip_conv3d_u8_taps_build_tables_sampled": (C.c_int, [C.POINTER(ConvDesc), _I, _I, _I, _P, C.c_float, _P, _P, _P, _P]),
    "advhip_conv3d_u8_taps_tencrop_bn_relu_maxpool233_sampled_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _I, _I, C.c_uint64, _L, _L, _P, _P,
                                                                               _P, _P, _P, C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_u8_tencrop_bn_relu_maxpool233_sampled_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _I, _I, _I, _I, _I, C.c_uint64, _L, _P, _P, _P,
                                                                          _P, _P, C.c_float, _P, _L, _P, _L, _P]),
    "advhip_conv3d_bn_act_maxpool211_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _P, _P, _P, _P, _P, _P, _L, _P]),
    "advhip_bgemm_f32": (C.c_int, [C.POINTER(GemmDesc), _P, _P, _P, _P]),
    "advhip_gemm_nt_f32": (C.c_int, [_P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _L, _P]),
    "advhip_gemm_nt_rowsum_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _L, _I, _P]),
    "advhip_gemm_nt_workspace_bytes": (_L, [_I, _I, _I, _I]),
    "advhip_gemm_nt_reduced_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _L, _L, _I, _I, _P, _L, _P]),
    "advhip_gemm_nt_slabs_f32": (C.c_int, [_P, _P, _P, _I, _I, _I, _L, _L, _I, _I, _I, _P]),
    "advhip_sum_slabs_f32": (C.c_int, [_P, _P, _L, _I, _L, _P]),
    "advhip_gemm_nt_group_slabs_f32": (C.c_int, [C.POINTER(NtItem), _I, _I, _I, _L, _P]),
    "advhip_softmax_rows_f32": (C.c_int, [_P, _P, _L, _I, C.c_float, _P]),
    "advhip_conv3d_bn_act_ex_f32": (C.c_int, [C.POINTER(ConvDesc), _P, _L, _P, _P, _P, _P, _P, _P, _L, C.POINTER(ConvEpilogue), _P, _L, _P]),
    "advhip_chan_stats_f32": (C.c_int, [_P, _P, _P, _I, _L, C.c_float, _P]),
    "advhip_maxpool3d_f32": (C.c_int, [_P, _P] + [_I] * 11 + [_P]),
    "advhip_maxpool3d_padded_f32": (C.c_int, [_P, _P] + [_I] * 14 + [_P]),
    "advhip_maxpool3d_strided_f32": (C.c_int, [_P, _P, _L] + [_I] * 11 + [_P]),
    "advhip_global_avgpool_f32": (C.c_int, [_P, _P, _L, _I, _P]),
    "advhip_chan_layernorm_fwd_f32": (C.c_int, [_P] * 6 + [_I, _L, C.c_float, _P]),
    "advhip_chan_layernorm_bwd_partial_rows": (_L, [_L]),
    "advhip_chan_layernorm_bwd_f32": (C.c_int, [_P] * 8 + [_I, _L, C.c_float, _P]),
    "advhip_bn_rows_fwd_f32": (C.c_int, [_P] * 6 + [_I, _L, C.c_float, _P]),
    "advhip_bn_rows_bwd_f32": (C.c_int, [_P] * 8 + [_I, _L, C.c_float, _P]),
    "advhip_bn_rows_fwd_running_f32": (C.c_int, [_P] * 8 + [C.c_float, _I, _L, C.c_float, _P]),
    "advhip_bn_rows_bwd_add_f32": (C.c_int, [_P] * 9 + [_I, _L, C.c_float, _P]),
    "advhip_chan_layernorm_bwd_add_f32": (C.c_int, [_P] * 8 + [_I, _L, C.c_float, _P]),
    "advhip_conv1d_pack_weight_dx_f32": (C.c_int, [_P, _P, _I, _I, _I, _P]),
    "advhip_amp_combine_fwd_f32": (C.c_int, [_P, _P, _P, _L, _P, _P, C.c_float, _P, _I, _L, _I, _P]),
    "advhip_amp_combine_bwd_f32": (C.c_int, [_P, _P, _L, C.c_float, _P, _P, _P, _P, _I, _L, _I, _P]),
    "advhip_colsum_f32": (C.c_int, [_P, _P, _L, _I, _P]),
    "advhip_colsum_group_f32": (C.c_int, [C.POINTER(ColsumItem), _I, _P]),
    "advhip_adam_multi_f32": (C.c_int, [C.POINTER(AdamItem), _I, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    # (items, n_items, lr_dev (double*), grad_scale_dev (float*, may be null), beta1, beta2, eps, weight_decay, stream)
    "advhip_adam_multi_dev_f32": (C.c_int, [C.POINTER(AdamItem), _I, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, _P]),
    # (items, n_items, max_norm, partials (double*), n_partials, norm_out, scale_out, stream)
    "advhip_grad_norm_multi_f32": (C.c_int, [C.POINTER(NormItem), _I, C.c_double, _P, _L, _P, _P, _P]),
    "advhip_pack_item_tiles": (C.c_int64, [_I, _I, _I, _I]),
    "advhip_pack_weights_multi_f32": (C.c_int, [_P, _I, _I, _P]),
    "advhip_unfold3_f32": (C.c_int, [_P, _P, _I, _L, _I, _P]),
    "advhip_dwconv_t_fwd_f32": (C.c_int, [_P] * 4 + [_I, _I, _L, _I, _I, _P]),
    "advhip_dwconv_t_bwd_chunks": (_I, [_I, _L]),
    "advhip_dwconv_t_bwd_f32": (C.c_int, [_P] * 5 + [_I, _I, _L, _I, _I, _P]),
    "advhip_glance_attention_fwd_f32": (C.c_int, [_P, _P, _P, _I, _L, _I, _I, C.c_float, _P]),
    "advhip_glance_attention_bwd_f32": (C.c_int, [_P, _P, _P, _P, _I, _L, _I, _I, C.c_float, _P]),
    "advhip_ffn_block_partial_rows": (_L, [_L]),
    "advhip_ffn_block_fwd_f32": (C.c_int, [_P, _P, _P, C.c_float, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _L, _P]),
    "advhip_ffn_block_bwd_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_float, _P, _P, _P, _P, _P, _P, _I, _L, _P]),
    "advhip_glance_attention_fwd_anyt_f32": (C.c_int, [_P, _P, _P, _I, _L, _I, _I, C.c_float, _P]),
    "advhip_glance_attention_bwd_anyt_f32": (C.c_int, [_P, _P, _P, _P, _P, _I, _L, _I, _I, C.c_float, _P]),
    "advhip_fold_affine_f32": (C.c_int, [_P] * 7 + [_I, _I, _P]),
    "advhip_head_ln_fc_partial_rows": (_L, [_L]),
    "advhip_head_ln_fc_fwd_f32": (C.c_int, [_P] * 9 + [_I, _L, C.c_float, _P]),
    "advhip_head_ln_fc_bwd_f32": (C.c_int, [_P] * 11 + [_I, _L, _P]),
    "advhip_mil_magnitude_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "advhip_mil_topk_select_f32": (C.c_int, [_P] * 7 + [_I] * 5 + [_P]),
    "advhip_mil_topk_select_bwd_f32": (C.c_int, [_P] * 5 + [_I] * 5 + [_P]),
    "advhip_mil_magnitude_bwd_f32": (C.c_int, [_P] * 5 + [_I] * 4 + [_P]),
    "advhip_mgfn_loss_ws_floats": (_L, [_I, _I, _I]),
    "advhip_mgfn_loss_fwd_f32": (C.c_int, [_P] * 9 + [_I] * 5 + [_P]),
    "advhip_mgfn_loss_bwd_f32": (C.c_int, [_P] * 14 + [_I] * 5 + [_P]),
    "advhip_segment_features_f32": (C.c_int, [_P, _P, _I, _I, _I, _I, _P]),
    "advhip_add_magnitude_f32": (C.c_int, [_P, _P, _L, _I, _P]),
    "advhip_add_magnitude_np_f32": (C.c_int, [_P, _P, _L, _I, _I, _I, _P]),
    "advhip_add_magnitude_np_leaves": (C.c_int, [_I, C.POINTER(_I), C.POINTER(_I)]),
    "advhip_tencrop_normalize_planes_u8": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _L, _L, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_u8": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_planes_u8_strided": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _L, _L, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_u8_strided": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_planes_u8_crops": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, _L, _L, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_u8_crops": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_planes_u8_sampled": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, _L, _L, C.c_float, C.c_float, _P]),
    "advhip_tencrop_normalize_u8_sampled": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, C.c_float, C.c_float, _P]),
    "advhip_crop_minmax_u8": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "advhip_tencrop_normalize_u8_modes": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, _I, C.POINTER(C.c_double),
                                                    C.POINTER(C.c_double), _P, _I, _P]),
    "advhip_tencrop_normalize_planes_u8_modes": (C.c_int, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, C.c_uint64, _L, _L, _I,
                                                           C.POINTER(C.c_double), C.POINTER(C.c_double), _P, _I, _P]),
    "advhip_frame_scores_f32": (C.c_int, [_P, _P, _L, _I, _I, _L, _P]),
    "advhip_normalize_permute_u8": (C.c_int, [_P, _P, _L, _I, _I, _I, _I, C.c_float, C.c_float, _P]),
    "advhip_resize_u8": (C.c_int, [_P, _P, _P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "advhip_resize_u8_sampled": (C.c_int, [_P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _P]),
    "advhip_yuv420_to_rgb_u8": (C.c_int, [_P, _P, _L, _I, _I, _I, _I] + [_I] * 6 + [_P]),
    "advhip_resize_yuv420_u8": (C.c_int, [_P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I] + [_I] * 6 + [_P]),
    # (..., frame_pitch, H, W, [resize arguments,] bits, shift, y_offset, y_pitch, cb_offset, cr_offset, chroma_pitch, chroma_step, coefficients)
    "advhip_yuv420_surface_to_rgb_u8": (C.c_int, [_P, _P, _L, _I, _L, _I, _I] + [_I, _I, _L, _L, _L, _L, _L, _I] + [_I] * 6 + [_P]),
    "advhip_resize_yuv420_surface_u8": (C.c_int, [_P, _P, _P, _L, _I, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _I, _I, _I]
                                        + [_I, _I, _L, _L, _L, _L, _L, _I] + [_I] * 6 + [_P]),
    # (src, dst, ws, F_src, N, src_of, frame_step, table_of, n_tables, [frame_pitch,] H, W, C, OH, OW, the stacked tables, rowspan, ws_rows, ...)
    "advhip_resize_roi_u8": (C.c_int, [_P, _P, _P, _L, _L, _P, _I, _P, _I] + [_I] * 5 + [_P, _P, _I, _P, _P, _I, _P, _I] + [_P]),
    "advhip_resize_roi_yuv420_u8": (C.c_int, [_P, _P, _P, _L, _L, _P, _I, _P, _I] + [_I] * 5 + [_P, _P, _I, _P, _P, _I, _P, _I] + [_I] * 7 + [_P]),
    "advhip_resize_roi_surface_u8": (C.c_int, [_P, _P, _P, _L, _L, _P, _I, _P, _I, _L] + [_I] * 5 + [_P, _P, _I, _P, _P, _I, _P, _I]
                                     + [_I, _I, _L, _L, _L, _L, _L, _I] + [_I] * 6 + [_P]),
    "advhip_roc_counts_ws_bytes": (_L, [_L]),
    # (scores, pos, neg, M, thresholds, tps, fps, meta, workspace, workspace_bytes, stream)
    "advhip_roc_counts": (C.c_int, [_P, _P, _P, _L, _P, _P, _P, _P, _P, _L, _P]),
    # padded batches of sequences of unequal length (batched validation): row lengths are a device int32 array
    "advhip_glance_attention_fwd_lens_f32": (C.c_int, [_P, _P, _P, _I, _L, _I, _I, C.c_float, _P]),
    "advhip_dwconv_t_fwd_lens_f32": (C.c_int, [_P] * 4 + [_I, _I, _L, _I, _I, _P, _L, _P]),
    "advhip_amp_combine_fwd_lens_f32": (C.c_int, [_P, _P, _P, _L, _P, _P, C.c_float, _P, _I, _L, _I, _P, _P]),
    "advhip_mask_tail_f32": (C.c_int, [_P, _I, _L, _I, _P, _P]),
    "advhip_pack_padded_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "advhip_crop_mean_scatter_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    # (src0, idx0, lab0, n0, b0, src1, idx1, lab1, n1, b1, dst, dst_lab0, dst_lab1, R, stream): rows of two stores by index, one launch
    "advhip_gather_batch_f32": (C.c_int, [_P, _P, _P, _L, _I, _P, _P, _P, _L, _I, _P, _P, _P, _L, _P]),
    # anomaly events from per-frame scores of a ragged batch: (scores, offsets, V, N, window, out, stream)
    "advhip_smooth_scores_f32": (C.c_int, [_P, _P, _L, _L, _I, _P, _P]),
    "advhip_score_events_ws_bytes": (_L, [_L, _L]),
    # (smoothed, offsets, V, N, low, high, merge_gap, min_len, ev_int, ev_f, cap, counts, meta, workspace, workspace_bytes, stream)
    "advhip_score_events": (C.c_int, [_P, _P, _L, _L, C.c_float, C.c_float, _I, _I, _P, _P, _L, _P, _P, _P, _L, _P]),
    # live scoring: (feats, cam_ids, ring, counts, n, n_cam, ncrops, W, C, stream) / (ring, counts, cam_ids, dst, nb, n_cam, ncrops, W, Tmax, C1, stream)
    # / (scores, lens, cam_ids, latest, nb, ncrops, Tmax, stream)
    "advhip_ring_push_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "advhip_ring_windows_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "advhip_crop_mean_last_f32": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _P]),
    # live frames: (frames, cam_ids, ring, counts, n, n_cam, R, frame_bytes, stream) / (ring, counts, cam_ids, dst, nb, n_cam, R, frame_bytes,
    # frames_per_clip, frame_step, stream)
    "advhip_frame_ring_push_u8": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _P]),
    "advhip_frame_ring_windows_u8": (C.c_int, [_P, _P, _P, _P, _I, _I, _I, _L, _I, _I, _P]),
    # motion gate: (frames, cam_ids, anchor, state, scratch, n, n_cam, frame_bytes, pixel_delta, limit, stream) / (cam_ids, ring, counts, n,
    # n_cam, ncrops, W, C1, stream)
    "advhip_frame_gate_update_u8": (C.c_int, [_P, _P, _P, _P, _P, _I, _I, _L, _I, _I, _P]),
    "advhip_ring_repeat_f32": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    # live events: (scores, cam_ids, ring, samples, cand_int, cand_peak, cand_sum, alert, open_start, log_int, log_f, emitted, nb, n_cam, K,
    # smooth, low, high, merge_gap, min_len, by_camera, mode, stream)
    "advhip_live_events_update_f32": (C.c_int, [_P] * 12 + [_I, _I, _I, _I, C.c_float, C.c_float, _I, _I, _I, _I, _P]),
    # which kernel form a scorer launch takes: (C, N, aligned16) / (T, aligned16) -> form id (include/advhip.h); nothing is launched
    "advhip_bn_rows_form": (_I, [_I, _L, _I]),
    "advhip_chan_layernorm_form": (_I, [_I, _L, _I]),
    "advhip_head_ln_fc_form": (_I, [_I, _L, _I]),
    "advhip_dwconv_t_form": (_I, [_I, _I]),
    # which pooling kernel a launch takes: (W, kt, kh, kw, st, sh, sw, y_padded) / (n) -> form id
    "advhip_maxpool3d_form": (_I, [_I] * 8),
    "advhip_global_avgpool_form": (_I, [_I]),
}

# advhip_live_events_update_f32: the modes and the width of cand_int (ADVHIP_LIVE_EVENTS_* of include/advhip.h)
LIVE_EVENTS_UPDATE, LIVE_EVENTS_FINISH, LIVE_EVENTS_RESET, LIVE_EVENTS_CAND_INTS = 0, 1, 2, 5

# advhip_bn_rows_form's answers (ADVHIP_BN_ROWS_* of include/advhip.h)
BN_ROWS_GENERIC, BN_ROWS_REG256X4, BN_ROWS_REG256X12, BN_ROWS_REG1024X4 = 0, 1, 2, 3

# advhip_maxpool3d_form's answers (ADVHIP_MAXPOOL_* of include/advhip.h)
MAXPOOL_GENERIC, MAXPOOL_ROW233, MAXPOOL_TEMPORAL = 0, 1, 2

_lib: Optional[C.CDLL] = None


def load(path: Optional[str] = None) -> C.CDLL:
    """dlopen the C-ABI library and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise HipExtensionError(
            f"{p} not found: the HIP extension has not been built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or "
            "`python -m anomaly_detection_on_video_amd.build`). There is no CPU fallback."
        )
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # pragma: no cover
            raise HipExtensionError(f"{p} does not export {name}; rebuild the extension") from e
        fn.restype = res
        fn.argtypes = args
    if lib.advhip_abi_version() != 2:
        raise HipExtensionError(f"{p}: ABI version {lib.advhip_abi_version()} != 2; rebuild the extension")
    if path is None:
        _lib = lib
    return lib


ON_FAILURE: list = []  # callables run when an entry point reports an error (ops drops per-stream state a failed launch may have left dirty)


def check(rc: int, what: str = "advhip") -> None:
    if rc != 0:
        msg = load().advhip_last_error().decode("utf-8", "replace")
        for hook in ON_FAILURE:
            try:
                hook()
            except Exception:  # pragma: no cover - a clean-up hook must not mask the error being reported
                pass
        raise HipExtensionError(f"{what} failed (code {rc}): {msg}")


def require_gpu(*tensors: torch.Tensor, contiguous: bool = True) -> None:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.is_cuda:
            if dev is None:
                dev = t.device
                if dev.index is not None and dev.index != torch.cuda.current_device():
                    # kernels launch on the CURRENT device: a tensor elsewhere would be read through peer access (or
                    # fault) on a stream that orders nothing on its own device
                    raise HipExtensionError(
                        f"tensor on {dev} but the current device is cuda:{torch.cuda.current_device()}: "
                        "call torch.cuda.set_device (one process per GPU)")
            elif t.device != dev:
                raise HipExtensionError(f"tensors on different devices: {dev} and {t.device}")
        if not t.is_cuda:
            raise HipExtensionError(
                "this op runs only as a HIP kernel on an AMD GPU; got a tensor on "
                f"'{t.device}'. Move the module and its inputs to cuda (there is no CPU fallback)."
            )
        if t.dtype not in (torch.float32, torch.int64, torch.int32, torch.uint8):
            raise HipExtensionError(f"unsupported dtype {t.dtype}; the kernels compute in fp32")
        if contiguous and not t.is_contiguous():
            raise HipExtensionError("HIP kernels need contiguous tensors")


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream(dev=None) -> int:
    """Raw hipStream_t of torch's current stream on `dev` (a tensor, a device, or None = the current device)."""
    if isinstance(dev, torch.Tensor):
        dev = dev.device
    return torch.cuda.current_stream(dev).cuda_stream
