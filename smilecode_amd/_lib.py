"""ctypes binding of libmodet_hip.so (the C ABI declared in include/modet_hip.h).

The product path has NO fallback: if the library is missing or a call fails this module
raises.  ``load()`` is cheap after the first call.  ctypes drops the GIL for the duration
of each call (CDLL), the library itself is stateless/re-entrant.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# MODET_HIP_LIB: load another build of the same library (A/B timing of kernel variants on one box, tools/ab_kernels.py)
LIB_PATH = os.environ.get("MODET_HIP_LIB") or os.path.join(_HERE, "lib", "libmodet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "modet_hip.h")       # the core family's (FAMILIES below)

P, I, I64, F, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t

class LeafJob(C.Structure):
    """modet_leaf_job_t (include/modet_hip.h)"""
    _fields_ = [("part", P), ("outer", I64), ("outer_stride", I64), ("rows", I64), ("row_stride", I64),
                ("col_group_stride", I64), ("ncols", I), ("col_group", I), ("dst", P * 4), ("n", I * 4)]


# name -> (restype, argtypes); mirrors include/modet_hip.h one to one
SIGNATURES = {
    "modet_hip_version": (I, []),
    "modet_hip_strerror": (C.c_char_p, [I]),
    "modet_qk_fwd": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "modet_qk_bwd_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_qk_bwd": (I, [P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_qk_fwd_f64": (I, [P, P, P, P, I, I, I, I, I, I, P]),
    "modet_qk_bwd_ws_bytes_f64": (SZ, [I, I, I, I, I]),
    "modet_qk_bwd_f64": (I, [P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_na_fwd": (I, [P, P, P, P, P, I, I, I, I, I, I, F, P]),
    "modet_na_bwd_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_na_bwd_partial_rows": (I64, [I, I, I, I, I, I]),
    "modet_na_bwd": (I, [P, P, P, P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, F, P]),
    "modet_na_fwd_t": (I, [P, P, I, P, P, P, I, I, I, I, I, I, F, P]),
    "modet_na_bwd_t": (I, [P, P, I, P, P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, F, P]),
    "modet_conv3d_kernel_family": (I, [I, I, I, I, I, I, I]),
    "modet_conv3d_kernel_family_v": (I, [I, I, I, I, I, I, I, I]),
    "modet_conv3d_ws_bytes": (SZ, [I, I]),
    "modet_conv3d_fwd": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, P, P]),
    "modet_conv3d_fwd_bounded": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, P, P]),
    "modet_conv3d_stats_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_normin_stats_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_fwd_stats": (I, [P, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_fwd_stats_bounded": (I, [P, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_fwd_normin": (I, [P, P, P, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_bwd_data": (I, [P, P, P, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_bwd_weight_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_bwd_weight": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_conv3d_bwd_weight_act": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_step_ctx_create": (I, [C.POINTER(P)]),
    "modet_step_ctx_destroy": (I, [P]),
    "modet_conv3d_prepack_record": (I, [P, I]),
    "modet_conv3d_prepack_arena_bytes": (SZ, [P]),
    "modet_conv3d_prepack_begin": (I, [P, P, SZ, P]),
    "modet_conv3d_prepack_end": (I, [P]),
    "modet_conv3d_bwd_weight_defer": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_wgrad_defer_flush": (I, [P, P]),
    "modet_conv3d_wgrad_defers_operands": (I, [I, I, I, I, I, I]),
    "modet_instnorm_ws_bytes": (SZ, [I, I64, I]),
    "modet_instnorm_lrelu_fwd": (I, [P, P, P, P, P, SZ, I, I64, I, F, P]),
    "modet_instnorm_lrelu_fwd_stats": (I, [P, P, P, P, P, SZ, I, I64, I, F, P]),
    "modet_instnorm_stats": (I, [P, P, P, P, SZ, P, SZ, I, I64, I, F, P]),
    "modet_conv3d_bwd_data_instats_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_bwd_data_instats": (I, [P, P, P, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_instnorm_lrelu_bwd_rows": (I, [P, P, P, P, P, P, SZ, P, SZ, I, I64, I, P]),
    "modet_instnorm_lrelu_bwd": (I, [P, P, P, P, P, P, SZ, I, I64, I, P]),
    "modet_lrelu_bwd": (I, [P, P, P, I64, P]),
    "modet_avgpool2_fwd": (I, [P, P, I, I, I, I, I, P]),
    "modet_avgpool2_fwd_x16": (I, [P, P, I, I, I, I, I, P]),
    "modet_instnorm_lrelu_apply_pool": (I, [P, P, P, P, P, I, I, I, I, I, P]),
    "modet_instnorm_lrelu_bwd_pool": (I, [P, P, P, I, P, P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_instnorm_lrelu_bwd_amax": (I, [P, P, P, P, P, P, SZ, I, I64, I, P, P]),
    "modet_instnorm_lrelu_bwd_rows_amax": (I, [P, P, P, P, P, P, SZ, P, SZ, I, I64, I, P, P]),
    "modet_instnorm_lrelu_bwd_pool_amax": (I, [P, P, P, I, P, P, P, P, P, SZ, I, I, I, I, I, P, P]),
    "modet_conv3d_bwd_data_amax": (I, [P, P, P, P, SZ, I, I, I, I, I, I, P, P, P]),
    "modet_conv3d_bwd_data_instats_amax": (I, [P, P, P, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P, P]),
    "modet_conv3d_bwd_weight_amax": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, P, P, P]),
    "modet_conv3d_bwd_weight_normin_ok": (I, [I, I, I, I, I, I]),
    "modet_conv3d_bwd_weight_normin": (I, [P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P, P, P]),
    "modet_avgpool2_bwd": (I, [P, P, P, I, I, I, I, I, P]),
    "modet_proj_ln_fwd": (I, [P, P, P, P, P, P, I64, I, I, F, P]),
    "modet_proj_ln_bwd_ws_bytes": (SZ, [I64, I, I]),
    "modet_proj_ln_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, SZ, I64, I, I, F, P]),
    "modet_proj_ln_bwd_pair_ws_bytes": (SZ, [I64, I, I]),
    "modet_proj_ln_fwd_pair": (I, [P, P, P, P, P, P, P, P, I64, I, I, F, P]),
    "modet_proj_ln_bwd_pair_partial_rows": (I64, [I64, I, I]),
    "modet_leaf_reduce_many": (I, [P, I, P]),
    "modet_proj_ln_bwd_pair": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, SZ, I64, I, I, F, P]),
    "modet_proj_ln_fwd_t": (I, [P, I, P, P, P, P, P, I, I64, I, I, F, P]),
    "modet_proj_ln_bwd_pair_t": (I, [P, I, P, P, P, I, P, P, P, P, P, P, P, P, P, P, SZ, I64, I, I, F, P]),
    "modet_warp_fwd": (I, [P, P, P, I, I, I, I, I, I, I, P]),
    "modet_warp_fwd_o16": (I, [P, P, P, I, I, I, I, I, P]),
    "modet_warp_fwd_t": (I, [P, I, P, P, I, I, I, I, I, I, P]),
    "modet_warp_bwd_t": (I, [P, I, P, P, P, P, I, I, I, I, I, I, I, P]),
    "modet_warp_bwd_acc": (I, [P, I, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "modet_warp_bwd_det_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_warp_bwd_det": (I, [P, I, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_warp_bwd_dsrc_tiles_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_warp_bwd_dsrc_tiles": (I, [P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_warp_bwd_tiles": (I, [P, I, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_warp_bwd": (I, [P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "modet_upsample2_fwd": (I, [P, P, I, I, I, I, I, F, P]),
    "modet_upsample2_bwd": (I, [P, P, I, I, I, I, I, F, P]),
    "modet_upsample2_bwd_sep_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_upsample2_bwd_sep": (I, [P, P, P, SZ, I, I, I, I, I, F, P]),
    "modet_ncdhw_to_cl": (I, [P, P, I, I, I64, P]),
    "modet_cl_to_ncdhw": (I, [P, P, I, I, I64, P]),
    "modet_cwm_tail_fwd": (I, [P, P, P, I64, I, P]),
    "modet_cwm_tail_bwd": (I, [P, P, P, P, P, I64, I, P]),
    "modet_ncc_ws_bytes": (SZ, [I, I, I, I]),
    "modet_ncc_fwd_bwd": (I, [P, P, P, P, P, SZ, I, I, I, I, P]),
    "modet_ncc_fwd_bwd_win": (I, [P, P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_ncc_box_ws_bytes": (SZ, [I, I, I, I, I, I, I]),
    "modet_ncc_fwd_bwd_box": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, P]),
    "modet_grad3d_ws_bytes": (SZ, [I, I, I, I]),
    "modet_grad3d_fwd_bwd": (I, [P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_grad3d_fwd_bwd_cl": (I, [P, P, P, P, SZ, I, I, I, I, I, F, P]),
    "modet_ncc_fwd_bwd_win_scaled": (I, [P, P, P, P, P, SZ, I, I, I, I, I, F, P]),
    "modet_scale_by_dev_scalar": (I, [P, P, P, I64, P]),
    "modet_adam_amsgrad_step": (I, [P, P, P, P, P, I64, F, F, F, F, I, F, P]),
    "modet_corr3d_ws_bytes": (SZ, [I, I, I, I, I]),
    "modet_corr3d_fwd": (I, [P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_corr3d_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_label_warp_counts": (I, [P, P, P, P, P, I, I, I, I, P]),
    "modet_jacdet_nonpos_count": (I, [P, P, P, I, I, I, I, P]),
    "modet_conv3d_bf16_ws_bytes": (SZ, [I, I]),
    "modet_conv3d_bf16_stats_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_bf16_kernel_family": (I, [I, I, I, I, I, I, I, I]),
    "modet_conv3d_bf16_fwd": (I, [P, I, P, P, P, P, SZ, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_bf16_bwd_data": (I, [P, P, P, I, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_conv3d_bf16_bwd_weight_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "modet_conv3d_bf16_bwd_weight": (I, [P, I, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    "modet_conv3d_bf16_bwd_weight_defer": (I, [P, I, P, P, P, P, SZ, I, I, I, I, I, I, P, P]),
    "modet_instnorm_bf16_ws_bytes": (SZ, [I, I64, I]),
    "modet_instnorm_lrelu_fwd_stats_bf16": (I, [P, P, I, P, P, P, SZ, I, I64, I, F, P]),
    "modet_instnorm_lrelu_bwd_bf16": (I, [P, I, P, P, P, P, P, SZ, I, I64, I, P]),
    "modet_instnorm_lrelu_bwd_pool_bf16": (I, [P, P, P, I, P, P, P, P, P, SZ, I, I, I, I, I, P]),
    "modet_instnorm_lrelu_fwd_stats_pool_bf16": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, F, P]),
    "modet_cast_bf16": (I, [P, P, I64, I, P]),
}


def _header(name):
    return os.path.join(os.path.dirname(_HERE), "include", name)


# every ABI family of the one library, in the order they were added: name -> (header path, {entry point: (restype, argtypes)}).
# Each table mirrors its header one to one; the families beside the frozen core each have a header of their own.
FAMILIES = {
    "core": (HEADER_PATH, SIGNATURES),
    "mind": (_header("modet_hip_losses.h"), {
        "modet_mind_ws_bytes": (SZ, [I, I, I, I, I]),
        "modet_mind_descriptor": (I, [P, P, P, SZ, I, I, I, I, I, I, P]),
        "modet_mind_fwd_bwd": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, F, P]),
    }),
    "mi": (_header("modet_hip_mi.h"), {
        "modet_mi_ws_bytes": (SZ, [I, I, I, I, I]),
        "modet_mi_fwd_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, F, F, F, F, P]),
        "modet_lmi_fwd_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, F, F, F, I, F, P]),
    }),
    "ssim": (_header("modet_hip_ssim.h"), {
        "modet_ssim_ws_bytes": (SZ, [I, I, I, I, I]),
        "modet_ssim_fwd_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, F, P]),
    }),
    "reg": (_header("modet_hip_reg.h"), {
        "modet_reg_ws_bytes": (SZ, [I, I, I, I, I, I]),
        "modet_reg_fwd_bwd": (I, [P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
    }),
    "vecint": (_header("modet_hip_vecint.h"), {
        "modet_vecint_fwd": (I, [P, P, P, P, I, I, I, I, I, P]),
        "modet_vecint_ws_bytes": (SZ, [I, I, I, I, I, F]),
        "modet_vecint_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, F, P]),
    }),
    "surface": (_header("modet_hip_surface.h"), {
        "modet_surface_ws_bytes": (SZ, [I, I, I, I]),
        "modet_surface_distances": (I, [P, P, P, P, P, SZ, I, I, I, I, F, P]),
    }),
    "posenc": (_header("modet_hip_posenc.h"), {
        "modet_posenc_ws_bytes": (SZ, [I, I, I, I, I, I]),
        "modet_posenc_fwd_pair": (I, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, P]),
        "modet_posenc_bwd_data_pair": (I, [P, P, P, P, P, I, I, I, I, I, I, P]),
        "modet_posenc_bwd_params_pair": (I, [P, P, P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
    }),
    "convs2": (_header("modet_hip_convs2.h"), {
        "modet_convs2_ws_bytes": (SZ, [I, I, I, I, I, I, I]),
        "modet_convs2_fwd": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
        "modet_convs2_bwd_data": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
        "modet_convs2_bwd_weight": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
        "modet_cat_channels2_fwd": (I, [P, P, P, I64, I, I, P]),
        "modet_cat_channels2_bwd": (I, [P, P, P, I64, I, I, P]),
    }),
    "deconv": (_header("modet_hip_deconv.h"), {
        "modet_deconv4s2_ws_bytes": (SZ, [I, I, I, I, I, I, I]),
        "modet_deconv4s2_fwd": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
        "modet_deconv4s2_bwd_data": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
        "modet_deconv4s2_bwd_weight": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, I, I, F, P]),
    }),
    "pcnet": (_header("modet_hip_pcnet.h"), {
        "modet_pcnet_upsample_fwd": (I, [P, P, I, I, I, I, I, I, I, P]),
        "modet_pcnet_upsample_bwd": (I, [P, P, I, I, I, I, I, I, I, P]),
        "modet_pcnet_dfi_gate_fwd": (I, [P, P, P, I64, I, P]),
        "modet_pcnet_dfi_gate_bwd": (I, [P, P, P, P, P, I64, I, P]),
        "modet_pcnet_nff_ws_bytes": (SZ, [I, I64, I, I]),
        "modet_pcnet_nff_pool": (I, [P, P, P, P, P, P, P, P, SZ, I, I64, I, P]),
        "modet_pcnet_nff_gate_fwd": (I, [P, P, P, P, P, I, I, P]),
        "modet_pcnet_nff_gate_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, SZ, I, I, P]),
        "modet_pcnet_nff_apply_fwd": (I, [P, P, P, P, P, P, I, I64, I, P]),
        "modet_pcnet_nff_apply_bwd_gate": (I, [P, P, P, P, P, P, P, SZ, I, I64, I, P]),
        "modet_pcnet_nff_apply_bwd": (I, [P, P, P, P, P, P, P, P, P, P, P, P, P, I, I64, I, P]),
        "modet_pcnet_add": (I, [P, P, P, I64, P]),
    }),
    "prpp": (_header("modet_hip_prpp.h"), {
        "modet_prpp_upcat_fwd": (I, [P, P, P, I, I, I, I, I, I, P]),
        "modet_prpp_upcat_bwd": (I, [P, P, P, I, I, I, I, I, I, P]),
        "modet_prpp_relu_fwd": (I, [P, P, I64, P]),
        "modet_prpp_relu_add_fwd": (I, [P, P, P, I64, P]),
        "modet_prpp_relu_bwd": (I, [P, P, P, I64, P]),
        "modet_prpp_stack_ws_bytes": (SZ, [I, I, I, I, I]),
        "modet_prpp_stack_fwd": (I, [P, P, P, P, SZ, I, I, I, I, I, P]),
        "modet_prpp_stack_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, P]),
        "modet_prpp_compose_ws_bytes": (SZ, [I, I, I, I]),
        "modet_prpp_compose_fwd": (I, [P, P, P, I, I, I, I, I, I, I, P]),
        "modet_prpp_compose_bwd": (I, [P, P, P, P, P, P, SZ, I, I, I, I, I, I, I, P]),
    }),
    "resize": (_header("modet_hip_resize.h"), {
        "modet_resize_fwd": (I, [P, P, I, I, I, I, I, I, I, I, F, P]),
        "modet_resize_bwd": (I, [P, P, I, I, I, I, I, I, I, I, F, P]),
        "modet_resize_pyramid_fwd": (I, [P, P, P, P, I, I, I, I, P]),
        "modet_resize_pyramid_bwd": (I, [P, P, P, P, P, I, I, I, I, P]),
    }),
    "segdice": (_header("modet_hip_segdice.h"), {
        "modet_segdice_ws_bytes": (SZ, [I, I, I, I, I]),
        "modet_segdice_sums": (I, [P, P, P, P, P, SZ, I, I, I, I, I, I, P]),
        "modet_segdice_fwd_bwd": (I, [P, P, P, P, P, P, P, SZ, I, I, I, I, I, I, F, I, P]),
    }),
}
# The names a family's entry had before the registry.  Nothing in this tree uses them; they stay because the previous revision's
# test files, which every change is also run against, reach the library through them (about 95 test ids).  Views of FAMILIES:
# nothing is defined twice, and a new family gets no such name.
((LOSS_HEADER_PATH, LOSS_SIGNATURES), (MI_HEADER_PATH, MI_SIGNATURES), (SSIM_HEADER_PATH, SSIM_SIGNATURES),
 (REG_HEADER_PATH, REG_SIGNATURES), (VECINT_HEADER_PATH, VECINT_SIGNATURES)) = (FAMILIES[k] for k in ("mind", "mi", "ssim", "reg", "vecint"))

_lib = None


def header_symbols(path=None):
    """Every function name include/modet_hip.h (or the header at ``path``) declares (used by the export tests)."""
    txt = open(path or HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(modet_[a-z0-9_]+)\s*\(", txt)))


def load():
    """dlopen the library and attach signatures; raises if it is absent (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -m smilecode_amd.build` "
            "(the ModeT hot path has no CPU / eager fallback)")
    lib = C.CDLL(LIB_PATH)
    for _, table in FAMILIES.values():
        for name, (res, args) in table.items():
            if not hasattr(lib, name) and os.environ.get("MODET_HIP_LIB"):
                continue    # an older build loaded for A/B timing may predate an entry point; the product library may not
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def strerror(code: int) -> str:
    return load().modet_hip_strerror(int(code)).decode()


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what} failed: [{code}] {strerror(code)}")
