"""ctypes binding of libpnpmri.so (C ABI: include/pnp_mri.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, `lib()`
raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C pnp_admm_cnc_mri_amd/csrc`.
"""
import ctypes as C
import importlib.util
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# PNP_MRI_LIB: developer knob for A/B runs of two builds of the library; the product ships the in-tree one
LIB_PATH = os.environ.get('PNP_MRI_LIB') or os.path.join(_HERE, 'libpnpmri.so')

c_float_p = C.POINTER(C.c_float)
c_double_p = C.POINTER(C.c_double)
ctx_p = C.c_void_p
_vp = C.c_void_p

# name -> (restype, argtypes); mirrors include/pnp_mri.h one to one
SIGNATURES = {
    'pnp_abi_version': (C.c_int, []),
    'pnp_device_info': (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int, C.c_char_p, C.c_int]),
    'pnp_calibrate_stream': (C.c_int, [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double)]),
    'pnp_last_error': (C.c_char_p, []),
    'pnp_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'pnp_ctx_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ctx_p)]),
    'pnp_ctx_destroy': (C.c_int, [ctx_p]),
    'pnp_set_stream': (C.c_int, [ctx_p, _vp]),
    'pnp_sync': (C.c_int, [ctx_p]),
    'pnp_set_fast_path': (C.c_int, [ctx_p, C.c_int]),
    'pnp_set_schedule': (C.c_int, [ctx_p, C.c_int, C.c_int, C.c_int]),
    'pnp_get_schedule': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_get_plan': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_upload_problem': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_synthesize_problem': (C.c_int, [ctx_p, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_download_y': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_init_state': (C.c_int, [ctx_p]),
    'pnp_set_state': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_get_state': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_admm_l1_run': (C.c_int, [ctx_p, C.c_int, C.c_double, C.c_double]),
    'pnp_admm_cnc_run': (C.c_int, [ctx_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]),
    'pnp_download_x': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_admm_l1_run_traced': (C.c_int, [ctx_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, _vp, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_admm_cnc_run_traced': (C.c_int, [ctx_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _vp, C.c_int,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_trace_read': (C.c_int, [ctx_p, _vp, _vp, _vp]),
    'pnp_residuals': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int]),
    'pnp_residuals_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int]),
    'pnp_dc_step': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_prox_l1_dual': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_prox_cnc_dual': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    'pnp_cnc_combine': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    'pnp_add': (C.c_int, [ctx_p, _vp, _vp, _vp]),
    'pnp_dual_clamp': (C.c_int, [ctx_p, _vp, _vp, _vp]),
    'pnp_fft2_fwd': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_fft2_inv': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_A': (C.c_int, [ctx_p, _vp, _vp]),
    'pnp_AH': (C.c_int, [ctx_p, _vp, _vp]),
    'pnp_Df': (C.c_int, [ctx_p, _vp, _vp]),
    'pnp_metrics': (C.c_int, [ctx_p, _vp, _vp, C.c_int, c_double_p, c_double_p]),
    'pnp_ctx_create_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ctx_p)]),
    'pnp_ctx_create_any': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ctx_p)]),
    'pnp_ctx_create_any_f64': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(ctx_p)]),
    'pnp_upload_problem_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_set_state_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_get_state_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_download_x_f64': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_is_f64': (C.c_int, [ctx_p]),
    'pnp_synthesize_problem_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_download_y_f64': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_metrics_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int, c_double_p, c_double_p]),
    'pnp_ssim_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int, c_double_p]),
    'pnp_prepare_loops': (C.c_int, [ctx_p]),
    'pnp_conv3x3_c64_nhwc': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_c64_pack': (C.c_int, [_vp, _vp, _vp]),
    'pnp_conv3x3_c64_nhwc_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_c64_pack_f16x3': (C.c_int, [_vp, _vp, _vp]),
    'pnp_conv3x3_nhwc_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_f16x3_set_variant': (C.c_int, [C.c_int]),
    'pnp_conv3x3_nhwc_f16x3_fmt': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_pack_f16x3': (C.c_int, [_vp, _vp, _vp, C.c_int]),
    'pnp_conv3x3_tail_nchw_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_tail_add_nchw_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv2x2s2_nhwc_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_convT2x2s2_nhwc_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv2x2_pack_f16x3': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    'pnp_ffdnet_head_nhwc': (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_ffdnet_tail_f16x3': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_head_nhwc': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_tail_nchw': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    # half-precision layers (added after ABI 13, additive)
    'pnp_conv3x3_nhwc_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_pack_f16': (C.c_int, [_vp, _vp, _vp, C.c_int]),
    'pnp_conv3x3_head_nhwc_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_ffdnet_head_nhwc_f16': (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv3x3_tail_nchw_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_ffdnet_tail_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_conv2x2s2_nhwc_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_convT2x2s2_nhwc_f16': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_conv2x2_pack_f16': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    'pnp_relayout_c64': (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    # wavelet-domain sparsity (added after ABI 13, additive)
    'pnp_sparsity_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_set_sparsity': (C.c_int, [ctx_p, C.c_int, C.c_int]),
    'pnp_get_sparsity': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_dwt2_fwd': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_dwt2_inv': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_dwt2_fwd_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_dwt2_inv_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    # cycle spinning for the wavelet prox (added after ABI 13, additive)
    'pnp_spin_check': (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    'pnp_set_spin': (C.c_int, [ctx_p, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    'pnp_get_spin': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_set_spin_cursor': (C.c_int, [ctx_p, C.c_int]),
    # temporal sparsity (added after ABI 13, additive)
    'pnp_temporal_check': (C.c_int, [C.c_int, C.c_int]),
    'pnp_set_temporal': (C.c_int, [ctx_p, C.c_int, C.c_int]),
    'pnp_get_temporal': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    # locally low-rank prox (added after ABI 13, additive)
    'pnp_lowrank_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_set_lowrank': (C.c_int, [ctx_p, C.c_int, C.c_double, C.POINTER(C.c_int32), C.c_int]),
    'pnp_get_lowrank': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_set_lowrank_cursor': (C.c_int, [ctx_p, C.c_int]),
    'pnp_dwt2_shifted': (C.c_int, [ctx_p, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_dwt2_shifted_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    # multi-coil (SENSE) data consistency (added after ABI 13, additive)
    'pnp_coils_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_set_coils': (C.c_int, [ctx_p, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_set_coils_f64': (C.c_int, [ctx_p, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_set_cg': (C.c_int, [ctx_p, C.c_int]),
    'pnp_get_coils': (C.c_int, [ctx_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'pnp_upload_problem_mc': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_upload_problem_mc_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_synthesize_problem_mc': (C.c_int, [ctx_p, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_synthesize_problem_mc_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    'pnp_cg_residual': (C.c_int, [ctx_p, c_double_p]),
    # complex-valued images on a coil context (added after ABI 13, additive)
    'pnp_image_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_set_image': (C.c_int, [ctx_p, C.c_int]),
    'pnp_get_image': (C.c_int, [ctx_p, C.POINTER(C.c_int)]),
    'pnp_set_state_cx': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_set_state_cx_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_get_state_cx': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_get_state_cx_f64': (C.c_int, [ctx_p, _vp, _vp, C.c_int]),
    'pnp_download_x_cx': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_download_x_cx_f64': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_dc_step_cx': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_dc_step_cx_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_prox_l1_dual_cx': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_prox_l1_dual_cx_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double]),
    'pnp_prox_cnc_dual_cx': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    'pnp_prox_cnc_dual_cx_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    'pnp_A_cx': (C.c_int, [ctx_p, _vp, _vp]),
    # PnP denoisers on complex images (added after ABI 13, additive)
    'pnp_cx_den_in': (C.c_int, [ctx_p, _vp, _vp, _vp, C.c_int, C.c_double]),
    'pnp_cx_den_out': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, C.c_int, C.c_double]),
    'pnp_cx_den_out_dual': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double]),
    'pnp_cnc_combine_cx': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_double]),
    # coil mixing ahead of the multi-coil solve: prewhitening and coil compression (added after ABI 13, additive)
    'pnp_coilmix_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_coil_mix': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    'pnp_coil_mix_f64': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t]),
    'pnp_coil_gram': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_coil_gram_f64': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_coilmix_whiten': (C.c_int, [_vp, C.c_int, _vp]),
    'pnp_coilmix_compress': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    # coil sensitivity maps from the calibration region (added after ABI 13, additive)
    'pnp_coilmaps_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]),
    'pnp_coil_maps': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    'pnp_coil_maps_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]),
    'pnp_coil_maps_stage_times': (C.c_int, [ctx_p, C.c_int, c_float_p]),
    # ESPIRiT coil maps (added after ABI 13, additive)
    'pnp_espirit_check': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]),
    'pnp_calib_patch_gram': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_calib_patch_gram_f64': (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_espirit_kernels': (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp, C.POINTER(C.c_int), _vp]),
    'pnp_espirit_eigmaps': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_espirit_eigmaps_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    'pnp_espirit_maps': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]),
    'pnp_espirit_maps_f64': (C.c_int, [ctx_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                       C.c_double]),
    'pnp_espirit_ranks': (C.c_int, [ctx_p, _vp, C.c_int]),
    'pnp_espirit_stage_times': (C.c_int, [ctx_p, C.c_int, c_float_p]),
    'pnp_ssim': (C.c_int, [ctx_p, _vp, _vp, C.c_int, c_double_p]),
    'pnp_timer_start': (C.c_int, [ctx_p]),
    'pnp_timer_stop': (C.c_int, [ctx_p, c_float_p]),
    'pnp_kernels_per_iteration': (C.c_int, [ctx_p]),
    'pnp_path_name': (C.c_char_p, [ctx_p]),
    'pnp_ctx_path': (C.c_char_p, [ctx_p]),
    'pnp_fft_plan': (C.c_int, [ctx_p, C.c_int, C.c_char_p, C.c_int]),
}

ABI_VERSION = 13
_lib = None


class PnpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libpnpmri error %d: %s' % (code, msg))
        self.code = code


def lib():
    """Load libpnpmri.so once; raise (never fall back) if it is absent or ABI-mismatched."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s not found: build the HIP extension first (python -c "import __graft_entry__ as g; '
                          'g.build()" or make -C pnp_admm_cnc_mri_amd/csrc); there is no CPU fallback' % LIB_PATH)
    # One HIP runtime per process: libpnpmri.so and PyTorch-ROCm both need "libamdhip64.so.7" and
    # the dynamic loader keeps whichever copy arrives first.  The PnP solvers share streams and
    # device pointers with torch, so torch's bundled runtime must be that copy -- load it first.
    if 'torch' not in sys.modules and importlib.util.find_spec('torch') is not None:
        import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)           # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if L.pnp_abi_version() != ABI_VERSION:
        raise ImportError('libpnpmri.so ABI %d, binding expects %d' % (L.pnp_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise PnpError(rc, lib().pnp_last_error().decode('utf-8', 'replace'))


def device_count():
    n = C.c_int(0)
    check(lib().pnp_device_count(C.byref(n)))
    return n.value
