"""ctypes binding of libnst_hip.so (C ABI: include/nst_hip.h).

The shared library is the product: there is no CPU or eager-PyTorch fallback.  If it is missing
or does not export every symbol the header declares, importing the hot path fails loudly."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NST_LIB") or os.path.join(_HERE, "libnst_hip.so")   # NST_LIB: experiment builds
CSRC = os.path.join(_HERE, "csrc")

NST_OK = 0
NST_E_ARG = -1
NST_E_STATE = -2
NST_E_UNAVAILABLE = -5
NST_VGG19_CONVS = 13
NST_MAX_LEVELS = 8
NST_LOSS_ROW = 4
NST_MAX_STYLES = 8
NST_OPT_ADAM = 0
NST_OPT_LBFGS = 1
NST_COLOR_RGB = 0
NST_COLOR_LUMINANCE = 1
NST_POOL_MAX = 0
NST_POOL_AVG = 1
NST_MAX_LAPLACIAN = 4
NST_MAX_FLOW_SCALES = 12
NST_MAX_ANCHOR_SOURCES = 8

c_float_p = C.POINTER(C.c_float)
REDUCE_HOOK = C.CFUNCTYPE(None, C.c_void_p)
c_void = C.c_void_p


NST_CONV_F32, NST_CONV_BF16X3, NST_CONV_F16X2 = 0, 1, 2
CONV_MODES = {"f32": NST_CONV_F32, "bf16x3": NST_CONV_BF16X3, "f16x2": NST_CONV_F16X2}
NST_COMM_ID_BYTES = 128


class StepInfo(C.Structure):
    _fields_ = [("closures", C.c_int), ("total_closures", C.c_int), ("accepted", C.c_int),
                ("loss", C.c_float), ("lr", C.c_float), ("t", C.c_float), ("history", C.c_int)]


NST_GRAM_BATCH_MAX = 16


class GramBatchItem(C.Structure):
    """nst_gram_batch_item: the inputs of one map of nst_gram_batch and what the call reports back on the host."""
    _fields_ = [("f", C.c_void_p), ("C", C.c_int), ("h", C.c_int), ("w", C.c_int), ("guide", C.c_void_p), ("target", C.c_void_p),
                ("coef", C.c_float), ("gram", C.c_void_p), ("S", C.c_void_p), ("S_bf", C.c_void_p), ("mse", C.c_double),
                ("S_absmax", C.c_float), ("nsplit", C.c_int), ("pix_per_split", C.c_longlong)]


class Options(C.Structure):
    """nst_options: -1 = take the environment variable (read once at context creation), else the default."""
    _fields_ = [("struct_size", C.c_int), ("conv_mode", C.c_int), ("batched", C.c_int), ("single_stream", C.c_int),
                ("use_graph", C.c_int), ("h2_band_rows", C.c_int), ("lbfgs_gram", C.c_int), ("h2_mfma16", C.c_int),
                ("h2_wg256", C.c_int), ("h2_tile_rows", C.c_int), ("gram_overlap", C.c_int), ("h2_persist", C.c_int), ("level_split", C.c_int), ("h2_winograd", C.c_int)]


class LaunchInfo(C.Structure):
    """nst_launch_info: one timed launch of the last closure and the kernel shape the conv_h2 launcher decided for it."""
    _fields_ = [(n, C.c_int) for n in ("cls", "h", "w", "cin", "cout", "layer", "h2_rows", "h2_bn", "h2_ntw", "h2_chunk",
                                       "h2_mfma16", "h2_persist", "h2_second", "h2_unpool", "h2_bands")]


# name -> (restype, argtypes); every symbol include/nst_hip.h declares
SYMBOLS = {
    "nst_version": (C.c_int, []),
    "nst_last_error": (C.c_char_p, [c_void]),
    "nst_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "nst_ctx_create": (C.c_int, [C.c_int, C.POINTER(c_void), C.POINTER(c_void), C.POINTER(c_void)]),
    "nst_options_default": (None, [C.POINTER(Options)]),
    "nst_ctx_create_ex": (C.c_int, [C.c_int, C.POINTER(c_void), C.POINTER(c_void), C.POINTER(Options), C.POINTER(c_void)]),
    "nst_ctx_destroy": (None, [c_void]),
    "nst_job_configure": (C.c_int, [c_void, C.c_int, C.c_int, C.c_int]),
    "nst_job_set_taps": (C.c_int, [c_void, C.c_int, C.c_uint, C.c_int]),
    "nst_job_set_color": (C.c_int, [c_void, C.c_int]),
    "nst_job_color": (C.c_int, [c_void]),
    "nst_job_set_pooling": (C.c_int, [c_void, C.c_int]),
    "nst_job_pooling": (C.c_int, [c_void]),
    "nst_job_set_laplacian": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_int), c_float_p]),
    "nst_job_laplacian": (C.c_int, [c_void, C.POINTER(C.c_int), C.POINTER(C.c_int), c_float_p]),
    "nst_job_laplacian_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_laplacian_loss": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_job_set_matting": (C.c_int, [c_void, C.c_float, C.c_double]),
    "nst_job_matting": (C.c_int, [c_void, c_float_p, C.POINTER(C.c_double)]),
    "nst_job_matting_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_matting_loss": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_double, c_void, c_void, c_void]),
    "nst_level_set_anchor": (C.c_int, [c_void, C.c_int, c_void, c_void, C.c_float, c_void]),
    "nst_level_anchor": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int)]),
    "nst_job_temporal_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_anchor_loss": (C.c_int, [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_anchor_geometry": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_level_set_patches": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.c_int, c_float_p, C.c_int, C.c_double, c_void]),
    "nst_level_patches": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "nst_job_patch_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_level_patch_matches": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_patch_match": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, C.c_double, c_void,
                                  c_void, c_void]),
    "nst_patch_term": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_float,
                                 c_void, c_void, c_void]),
    "nst_level_set_patch_guidance": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, C.c_float, c_void]),
    "nst_level_patch_guidance": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_int), c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_patch_descriptors": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_void, c_void]),
    "nst_patch_match_guided": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, C.c_double,
                                         C.c_int, c_void, c_void, C.c_float, c_void, c_void, c_void]),
    "nst_level_set_histograms": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.c_int, c_float_p, C.c_int, c_void]),
    "nst_level_histograms": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int)]),
    "nst_job_histogram_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_level_histogram_tables": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nst_level_histogram_style": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_histogram_counts": (C.c_int, [c_void, c_void, C.c_longlong, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_histogram_tables": (C.c_int, [c_void, c_void, c_void, C.c_longlong, c_void, c_void, C.c_longlong, C.c_int, C.c_int, c_void, c_void]),
    "nst_histogram_term": (C.c_int, [c_void, c_void, C.c_longlong, C.c_int, C.c_int, c_void, c_void, C.c_float, c_void, c_void, c_void]),
    "nst_level_set_remd": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_double,
                                     c_void]),
    "nst_level_remd": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_job_remd_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_level_remd_matches": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nst_remd_match": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_void,
                                 c_void, c_void]),
    "nst_remd_term": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_void,
                                c_void, C.c_int, C.c_float, c_void, c_void, c_void, c_void]),
    "nst_level_set_selfsim": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_int), C.c_double, c_void]),
    "nst_level_selfsim": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "nst_job_selfsim_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_level_selfsim_decisions": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nst_selfsim_matrix": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, c_void, c_void, c_void]),
    "nst_selfsim_term": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_float, c_void, c_void,
                                   c_void, c_void]),
    "nst_level_set_xcorr": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.c_int, c_float_p, C.POINTER(C.c_int), C.c_int, c_void]),
    "nst_level_xcorr": (C.c_int, [c_void, C.c_int, c_float_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_job_xcorr_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_level_xcorr_matrices": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_xcorr": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, c_void, C.POINTER(C.c_int), c_void]),
    "nst_xcorr_term": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.POINTER(C.c_int), C.c_int, C.c_float, c_void, c_void,
                                 c_void]),
    "nst_warp_bilinear": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_flow_weights": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_anchor_fold": (C.c_int, [c_void, C.c_int, C.POINTER(c_void), C.POINTER(c_void), C.c_int, C.c_int, C.c_int, c_void, c_void,
                                  c_void, c_void]),
    "nst_flow_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "nst_flow_estimate": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, c_void, c_void,
                                    C.c_size_t, c_void]),
    "nst_flow_reduce": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_flow_prolong": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_flow_linearize": (C.c_int, [c_void, c_void, c_void, c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    "nst_flow_sweeps": (C.c_int, [c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_float, C.c_int, c_void, c_void,
                                  c_void]),
    "nst_flow_tvl1_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "nst_flow_tvl1_estimate": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                         C.c_int, c_void, c_void, C.c_size_t, c_void]),
    "nst_flow_tvl1_iterations": (C.c_int, [c_void, c_void, c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_float, C.c_float,
                                           C.c_float, C.c_int, c_void, c_void, c_void, c_void]),
    "nst_job_set_gram_shift": (C.c_int, [c_void, c_float_p, C.c_uint]),
    "nst_job_gram_shift": (C.c_int, [c_void, c_float_p, C.POINTER(C.c_uint)]),
    "nst_level_gram_offsets": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_gram_shifted": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nst_gram_batch": (C.c_int, [c_void, C.POINTER(GramBatchItem), C.c_int, C.c_int, c_void]),
    "nst_job_set_moments": (C.c_int, [c_void, c_float_p, c_float_p, C.c_float]),
    "nst_job_moments": (C.c_int, [c_void, c_float_p, c_float_p, c_float_p]),
    "nst_job_moment_losses": (C.c_int, [c_void, c_void, c_void]),
    "nst_moments": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_float, c_void, c_void, c_void]),
    "nst_job_set_style_weights": (C.c_int, [c_void, c_float_p]),
    "nst_job_style_weights": (C.c_int, [c_void, c_float_p]),
    "nst_color_stats": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), c_void]),
    "nst_color_transfer_matrix": (C.c_int, [C.POINTER(C.c_double)] * 6),
    "nst_color_affine": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), c_void, c_void]),
    "nst_luminance": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_double, C.c_double, c_void, c_void]),
    "nst_luminance_recombine": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_level_set_targets": (C.c_int, [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, c_void]),
    "nst_level_set_targets_blend": (C.c_int, [c_void, C.c_int, c_void, C.c_int, C.POINTER(c_void), C.POINTER(C.c_int),
                                              C.POINTER(C.c_int), c_float_p, c_void]),
    "nst_level_set_guidance": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_float_p, c_void]),
    "nst_level_set_targets_guided": (C.c_int, [c_void, C.c_int, c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_level_guidance": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_int), c_float_p, C.POINTER(C.c_double)]),
    "nst_level_guidance_planes": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_closure": (C.c_int, [c_void, c_void, C.c_float, C.c_float, C.c_float, c_void, c_void, c_void]),
    "nst_closure_levels": (C.c_int, [c_void, c_void, C.c_float, C.c_float, C.c_float, C.c_uint, c_void, c_void, c_void]),
    "nst_closure_forward": (C.c_int, [c_void, c_void, C.c_float, C.c_float, C.c_float, C.c_uint, c_void, c_void]),
    "nst_closure_backward": (C.c_int, [c_void, c_void, C.c_float, C.c_float, C.c_float, C.c_uint, c_void, c_void]),
    "nst_opt_shard_levels": (C.c_int, [c_void, C.c_uint, c_void, c_void, c_void, c_void]),
    "nst_opt_shard_levels_comm": (C.c_int, [c_void, C.c_uint, c_void]),
    "nst_opt_history": (C.c_int, [c_void, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_opt_set_closure_reuse": (C.c_int, [c_void, C.c_int]),
    "nst_opt_closure_stats": (C.c_int, [c_void, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "nst_opt_set_lazy_backward": (C.c_int, [c_void, C.c_int]),
    "nst_opt_backward_stats": (C.c_int, [c_void, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "nst_comm_unique_id": (C.c_int, [c_void]),
    "nst_comm_create": (C.c_int, [C.c_int, C.c_int, C.c_int, c_void, C.POINTER(c_void)]),
    "nst_comm_destroy": (None, [c_void]),
    "nst_comm_info": (C.c_int, [c_void, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_double)]),
    "nst_comm_allreduce_sum": (C.c_int, [c_void, c_void, C.c_size_t, c_void]),
    "nst_adam_step": (C.c_int, [c_void, c_void, c_void, c_void, c_void, C.c_size_t, C.c_int, C.c_double, c_void]),
    "nst_lbfgs_direction": (C.c_int, [c_void, c_void, C.POINTER(c_void), C.POINTER(c_void), C.POINTER(C.c_float), C.c_int,
                                      C.c_float, C.c_size_t, C.c_int, c_void, c_void]),
    "nst_opt_create": (C.c_int, [c_void, C.c_int, C.c_float, C.c_int, C.POINTER(c_void)]),
    "nst_opt_destroy": (None, [c_void]),
    "nst_opt_step": (C.c_int, [c_void, c_void, C.c_float, C.c_float, C.c_float, c_void, C.c_int,
                               C.POINTER(StepInfo), c_void]),
    "nst_vgg_features": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.POINTER(c_void), c_void]),
    "nst_vgg_features_backward": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.POINTER(c_void), c_void, c_void]),
    "nst_vgg_activations": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.POINTER(c_void), c_void]),
    "nst_level_activation": (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_job_map_stats": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_uint)]),
    "nst_ctx_set_keep_all_maps": (C.c_int, [c_void, C.c_int]),
    "nst_ctx_keep_all_maps": (C.c_int, [c_void]),
    "nst_ctx_set_forward_pack": (C.c_int, [c_void, C.c_int]),
    "nst_ctx_forward_pack": (C.c_int, [c_void]),
    "nst_ctx_set_gram_pack": (C.c_int, [c_void, C.c_int]),
    "nst_ctx_gram_pack": (C.c_int, [c_void]),
    "nst_ctx_set_h2_direct_weights": (C.c_int, [c_void, C.c_int]),
    "nst_ctx_h2_direct_weights": (C.c_int, [c_void]),
    "nst_ctx_h2_direct_launches": (C.c_longlong, [c_void]),
    "nst_level_image": (C.c_int, [c_void, C.c_int, c_void, c_void]),
    "nst_gram": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nst_guided_gram_backward": (C.c_int, [c_void, c_void, C.c_size_t, C.c_int, C.c_int, c_void, c_void, c_void, c_void, c_void,
                                            c_void, c_void]),
    "nst_total_variation": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    "nst_bicubic_half": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nst_bicubic_half_backward": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nst_prepare_img": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_unprepare_img": (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void, c_void]),
    "nst_resize_bicubic": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, c_void]),
    "nst_gather_rows": (C.c_int, [c_void, c_void, c_void, C.c_size_t, C.c_int, c_void, c_void]),
    "nst_gaussian_mask_accumulate": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                               C.c_double, c_void]),
    "nst_noise_blend": (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_double, c_void, c_void]),
    "nst_scale": (C.c_int, [c_void, c_void, C.c_float, C.c_size_t, c_void, c_void]),
    "nst_window_sums_count": (C.c_int, [C.POINTER(C.c_size_t)]),
    "nst_window_begin": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    "nst_window_end": (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, c_void, c_void,
                                 c_void, c_void]),
    "nst_conv_mode": (C.c_int, [c_void]),
    "nst_ctx_bytes": (C.c_int, [c_void, C.POINTER(C.c_size_t)]),
    "nst_set_timing": (C.c_int, [c_void, C.c_int]),
    "nst_last_closure_ms": (C.c_int, [c_void, C.POINTER(C.c_float)]),
    "nst_last_closure_class": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                         C.POINTER(C.c_double)]),
    "nst_last_closure_launches": (C.c_int, [c_void, C.POINTER(LaunchInfo), C.c_int, C.POINTER(C.c_int)]),
    "nst_last_closure_schedule": (C.c_int, [c_void, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "nst_dump_last_closure": (C.c_int, [c_void]),
    "nst_timing_totals": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long),
                                    C.POINTER(C.c_double), C.c_int]),
    "nst_timing_mfma_flops": (C.c_int, [c_void, C.c_int, C.POINTER(C.c_double)]),
}

_lib = None
_lock = threading.Lock()


class NstError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 into libnst_hip.so (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True)
    return LIB_PATH


def load():
    """Returns the ctypes handle; raises NstError when the native library is unavailable."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NstError(
                f"{LIB_PATH} is missing: the HIP extension is the only implementation of the style-transfer "
                f"hot path (no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"or `make -C {CSRC}`.")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise NstError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise NstError(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(ctx, code: int, what: str) -> None:
    if code != NST_OK:
        msg = load().nst_last_error(ctx)
        raise NstError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")
