"""ctypes binding of ``csrc/libneube_hip.so`` (the C ABI declared in ``include/neube_hip.h``).

There is no CPU fallback: if the library is missing or a symbol cannot be resolved this raises, and
every product-path op goes through :func:`lib`.  (The reference silently falls back to slow
``_ref`` ops when its plugin build fails, ``torch_utils/ops/bias_act.py:47-50``; this build must not.)
"""
from __future__ import annotations

import ctypes as C
import os
import threading

# torch MUST be imported before the library is dlopen'ed: the torch wheel bundles its own HIP runtime
# (torch/lib/libamdhip64.so, soname libamdhip64.so.7).  Loaded first, it satisfies this library's
# NEEDED libamdhip64.so.7, so kernels, device pointers and streams all live in ONE runtime.  Loaded
# second, /opt/rocm's copy would come in beside it and launches fail with "no ROCm-capable device".
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "csrc", "libneube_hip.so")
ABI_VERSION = 22

_lock = threading.Lock()
_lib = None

f32p = C.POINTER(C.c_float)
vp = C.c_void_p


class NbLayerDesc(C.Structure):
    """Mirror of ``struct NbLayerDesc`` (include/neube_hip.h)."""
    _fields_ = [
        ("affine_w", C.c_uint64), ("affine_b", C.c_uint64), ("wsq", C.c_uint64), ("styles", C.c_uint64),
        ("dcoefs", C.c_uint64), ("noise_const", C.c_uint64), ("noise_lin", C.c_uint64), ("noise_out", C.c_uint64),
        ("noise_strength", C.c_uint64),
        ("c_aff", C.c_int32), ("n_plain", C.c_int32), ("c_out", C.c_int32), ("w_index", C.c_int32),
        ("res", C.c_int32), ("style_scale", C.c_float), ("pad_", C.c_int32 * 2),
    ]


# name -> (restype, argtypes); must list EVERY symbol declared in include/neube_hip.h
PROTOTYPES = {
    "nb_last_error": (C.c_char_p, []),
    "nb_abi_version": (C.c_int, []),
    "nb_bias_act_f32": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_bias_act_grad_f32": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                       C.c_float, C.c_float, vp]),
    "nb_upfirdn2d_f32": (C.c_int, [vp, vp, vp] + [C.c_int] * 14 + [C.c_float, vp]),
    "nb_modconv3x3_up1_small_h3": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_up2_small_h3": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int,
                                             C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_conv2d_f32": (C.c_int, [vp, vp, vp, vp, vp] + [C.c_int] * 9 + [vp]),
    "nb_conv2d_wgrad_f32": (C.c_int, [vp, vp, vp] + [C.c_int] * 9 + [vp]),
    "nb_conv2d_wgrad_h3": (C.c_int, [vp, vp, vp, vp] + [C.c_int] * 9 + [vp]),
    "nb_conv2d_wgrad_h3_ws_bytes": (C.c_longlong, [C.c_int] * 5),
    "nb_conv2d_wgrad_h3_ws": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_longlong] + [C.c_int] * 10 + [vp]),
    "nb_modconv_bwd_dot_f32": (C.c_int, [vp, vp, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_modconv_bwd_finish_f32": (C.c_int, [vp, C.c_longlong, C.c_longlong, C.c_longlong, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_absmax_f32": (C.c_int, [vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, vp]),
    "nb_pack_h2_ranged_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_float, vp, vp, C.c_int, vp]),
    "nb_mapping_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_mapping_ws_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp]),
    "nb_styles_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_styles_fast_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_styles_noise_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "nb_demod_coefs_f32": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_noise_f32": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "nb_noise_seeded_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int, vp]),
    "nb_norm_positions_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp]),
    "nb_modconv3x3_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp, vp,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_variant": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "nb_calibrate_mfma_f16": (C.c_int, [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]),
    "nb_modconv3x3_up2_h3_variant": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "nb_pack_h2_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "nb_pack_conv_weight_h3": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "nb_pack_conv_weight_h3_dev": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "nb_conv3x3_s2_valid_h3": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int, vp] + [C.c_int] * 4 + [vp]),
    "nb_modconv3x3_up1_h3": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_up2_h3": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_up2_f32_h2": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp, vp, vp,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_torgb_triad_f32": (C.c_int, [vp, vp, C.c_int, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp,
                                     C.c_int, C.c_int, C.c_int, vp]),
    "nb_blend_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_modconv3x3_up1_h3_ex": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_up2_h3_ex": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_pack_h2f8_part_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_pack_h2f8_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "nb_pack_h2f6_part_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_pack_h2f6_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp]),
    "nb_modconv3x3_up1_h3_torgb": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_float, C.c_float, C.c_float, vp, vp]),
    "nb_modconv3x3_up1_h3_h2": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_modconv3x3_up2_h3_h2": (C.c_int, [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp]),
    "nb_pack_h2_part_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_geom_tiles_f32": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, vp]),
    "nb_canvas_replay_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int,
                                       vp, vp, vp]),
    "nb_canvas_replay_box_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int,
                                       vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_canvas_replay_pieces_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp,
                                              C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_paste_tiles_u8": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp]),
    "nb_enc_stem7x7_f32_h2": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_enc_conv3x3_h3": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_enc_conv3x3_h3_handoff": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_float, vp]),
    "nb_enc_upsample2x_h2": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_enc_stem7x7_f32_h2_ex": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_enc_conv3x3_ex": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_enc_upsample2x_h2_ex": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_enc_stem_conv3x3_f8": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp]),
    "nb_pack_conv_weight": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "nb_pack_conv_weight_dev": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
    "nb_pack_conv_weight_h3f8_dev": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    "nb_pack_conv_weight_h3_up2_dev": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    # the whole generator behind one handle (argument structs below)
    "nb_generator_param_count": (C.c_int, [vp]),
    "nb_generator_param_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "nb_generator_layer_count": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "nb_generator_layer_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int, vp]),
    "nb_generator_create": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]),
    "nb_generator_destroy": (C.c_int, [vp]),
    "nb_generator_forward": (C.c_int, [vp, vp, vp, C.c_int, vp]),
    "nb_generator_describe": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int]),
    # the geometry encoder behind the generator handle
    "nb_encoder_param_count": (C.c_int, []),
    "nb_encoder_param_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "nb_generator_encoder_check": (C.c_int, [vp, C.c_int]),
    "nb_generator_attach_encoder": (C.c_int, [vp, vp, C.c_int, vp]),
    "nb_generator_forward_geom": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    # staged passes (the generator split around the feature-canvas blend) and the canvas helpers of a C host
    "nb_generator_forward_staged": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp]),
    "nb_generator_describe_staged": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    # brush noise sets: a projected brush's noise_const replacements and their transposes (csrc/nb_brush_noise.hip)
    "nb_brush_noise_build_f32": (C.c_int, [vp, C.c_int, C.c_float, C.c_float, vp]),
    "nb_brush_noise_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "nb_brush_noise_load": (C.c_int, [vp, vp, vp, C.c_float, vp]),
    "nb_generator_bind_brush_noise": (C.c_int, [vp, vp]),
    "nb_brush_noise_destroy": (C.c_int, [vp]),
    "nb_dirty_area_alpha_f32":(C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    "nb_canvas_cells_count": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
    "nb_canvas_build_cells": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    # drawing preparation (csrc/nb_geomprep.hip): Otsu geometry into the padded buffer, tile picks, crop + on-white
    "nb_geom_prepare_u8": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "nb_tile_stroke_counts_u8": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "nb_composite_on_white_u8": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "nb_stitching_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 5),
    # vector strokes (csrc/nb_strokes.hip): splines cut into capsule segments, segments rasterised into the geometry
    "nb_raster_segments_u8": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_spline_flatten_f32": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp]),
    "nb_spline_segment_count": (C.c_longlong, [C.c_int, C.c_int, C.c_int]),
    # synthetic drawings (csrc/nb_drawings.hip): seeded spline control points, K drawings rasterised in one launch
    "nb_synth_spline_counts": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, vp]),
    "nb_synth_spline_ctrl_f32": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "nb_raster_batch_u8": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    # compositing for a paint session (csrc/nb_compose.hip): tiles over a canvas, a reduced view of a canvas window
    "nb_over_tiles_u8": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, vp]),
    "nb_canvas_view_u8": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    # masked selection (csrc/nb_select.hip): the k-th largest included value of every image
    "nb_masked_kth_largest_f32": (C.c_int, [vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    # brush scores (csrc/nb_metrics.hip): evaluation masks of the drawings, the per-image sums of the colour and transparency metrics
    "nb_eval_masks_f32": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "nb_brush_metrics_f32": (C.c_int, [vp, C.c_longlong, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp, vp, vp]),
    # inputs of the perceptual brush scores (csrc/nb_metric_patches.hip): the once-blurred guidance, masked mean colours, the patch pairs
    "nb_bg_guidance_f32": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
    "nb_bg_mean_colors_f32": (C.c_int, [vp, C.c_longlong, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "nb_metric_pairs_f32": (C.c_int, [vp, C.c_longlong, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    # inputs of the stitching scores (csrc/nb_stitch_metrics.hip): windows of full-size drawings, the composited and cropped pairs with their L1 sums
    "nb_stitch_crops_u8": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp]),
    "nb_stitch_pairs_f32": (C.c_int, [vp, C.c_longlong, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    # clarity optimisation (csrc/nb_clarity.hip): the fused loss and its gradient, the noise regulariser, the Adam + renormalise step
    "nb_clarity_scratch_floats": (C.c_longlong, [vp, C.c_int, C.c_longlong, C.c_int]),
    "nb_clarity_loss_f32": (C.c_int, [vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_int, C.c_int, C.c_int, C.c_float,
                                      C.c_float, C.c_float, vp, vp, vp, vp]),
    "nb_clarity_loss_bwd_f32": (C.c_int, [vp, C.c_longlong, vp, C.c_longlong, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                          C.c_float, vp, vp, vp]),
    "nb_noise_reg_f32": (C.c_int, [vp, C.c_longlong, C.c_longlong, C.c_int, vp, C.c_int, C.c_float, vp, C.c_longlong, vp, vp, C.c_longlong, vp]),
    "nb_clarity_step_f32": (C.c_int, [vp, vp, vp, vp, C.c_longlong, C.c_longlong, C.c_int, vp, C.c_int, C.c_float, C.c_int, vp, C.c_longlong, vp]),
    # brush projection (csrc/nb_projection.hip): the conservative masks and background colour, the fused loss and its gradient
    "nb_projection_masks_f32": (C.c_int, [vp, vp, C.c_longlong, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "nb_projection_loss_f32": (C.c_int, [vp, C.c_longlong, vp, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, vp, vp, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, C.c_float, vp, vp, vp, vp]),
    "nb_projection_loss_bwd_f32": (C.c_int, [vp, C.c_longlong, vp, vp, C.c_longlong, vp, C.c_longlong, vp, C.c_longlong, vp, vp, vp, vp, vp, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, vp, vp, vp, vp, vp]),
    # LPIPS network (csrc/nb_lpips.hip): scaling layer, bias + ReLU + tap + pool and its backward, the head and its backward
    "nb_lpips_scale_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_longlong, vp]),
    "nb_lpips_relu_pool_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_lpips_relu_pool_bwd_f32": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "nb_lpips_head_parts": (C.c_longlong, [C.c_int, C.c_int]),
    "nb_lpips_head_f32": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "nb_lpips_head_bwd_f32": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    # the per-batch layer plan (host only)
    "nb_plan_options_default": (C.c_int, [vp]),
    "nb_synthesis_plan": (C.c_int, [vp, vp, C.c_int, vp]),
}


class NbTilePiece(C.Structure):
    """``struct NbTilePiece`` of include/neube_hip.h."""
    _fields_ = [("data", C.c_uint64), ("cstride", C.c_int32), ("rstride", C.c_int32), ("cy", C.c_int32), ("cx", C.c_int32),
                ("h", C.c_int32), ("w", C.c_int32), ("ly0", C.c_int32), ("lx0", C.c_int32)]


class NbNoiseSrc(C.Structure):
    """``struct NbNoiseSrc`` of include/neube_hip.h (noise computed inside the split-f16 convolutions)."""
    _fields_ = [("noise_const_t", vp), ("noise_lin", vp), ("noise_strength", vp), ("norm_pos", vp), ("positions", vp),
                ("res", C.c_int), ("img_resolution", C.c_int)]


NB_NOISE_IN_KERNEL = -1


class NbBrushNoiseLayer(C.Structure):
    """``struct NbBrushNoiseLayer`` of include/neube_hip.h (one layer of nb_brush_noise_build_f32's host array)."""
    _fields_ = [("a", vp), ("b", vp), ("dst", vp), ("dst_t", vp), ("res", C.c_int32), ("pad", C.c_int32)]


class NbTorgbArgs(C.Structure):
    """``struct NbTorgbArgs`` of include/neube_hip.h."""
    _fields_ = [("styles", vp), ("w", vp), ("bias", vp), ("color_bias", vp), ("logits", vp), ("uvs", vp), ("img", vp),
                ("colors_out", vp), ("user_colors", vp), ("sfactor", vp), ("rgba_f32", vp), ("rgba_u8", vp),
                ("styles_stride_n", C.c_int), ("render_mode", C.c_int), ("clamp", C.c_float)]


class NbGeneratorConfig(C.Structure):
    """``struct NbGeneratorConfig`` of include/neube_hip.h (config.GeneratorConfig)."""
    _fields_ = [("z_dim", C.c_int32), ("c_dim", C.c_int32), ("w_dim", C.c_int32), ("img_resolution", C.c_int32),
                ("mapping_layers", C.c_int32), ("mapping_lr_multiplier", C.c_float), ("channel_base", C.c_int32),
                ("channel_max", C.c_int32), ("conv_clamp", C.c_float), ("num_geom", C.c_int32),
                ("geom_channels", C.c_int32 * 4), ("geom_resolutions", C.c_int32 * 4)]


class NbGeneratorLayerInfo(C.Structure):
    """``struct NbGeneratorLayerInfo`` (config.LayerSpec)."""
    _fields_ = [("block_res", C.c_int32), ("up", C.c_int32), ("in_channels", C.c_int32), ("out_channels", C.c_int32),
                ("geom_channels", C.c_int32), ("w_index", C.c_int32)]


class NbGeneratorInputs(C.Structure):
    """``struct NbGeneratorInputs``."""
    _fields_ = [("z", vp), ("ws", vp), ("truncation_psi", C.c_float), ("truncation_cutoff", C.c_int32), ("geom", vp * 4),
                ("positions", vp), ("noise_mode", C.c_int32), ("render_mode", C.c_int32), ("user_colors", vp), ("sfactor", vp),
                ("noise_seed", C.c_uint64), ("noise_offset", C.c_uint64), ("noise_state", vp)]


class NbGeneratorOutputs(C.Structure):
    """``struct NbGeneratorOutputs``."""
    _fields_ = [("rgba_u8", vp), ("rgba", vp), ("img", vp), ("uvs", vp), ("colors", vp)]


class NbGeneratorStage(C.Structure):
    """``struct NbGeneratorStage``: one half of a pass split around the feature-canvas blend."""
    _fields_ = [("stop_res", C.c_int32), ("resume_res", C.c_int32), ("features_out", vp), ("features_in", vp)]


NB_PLAN_MAX_LAYERS = 24
NB_PLAN_POS_NONE, NB_PLAN_POS_INT, NB_PLAN_POS_NORM = 0, 1, 2
NB_KERNEL_F32, NB_KERNEL_SMALL_H3, NB_KERNEL_LARGE_H3 = 0, 1, 2
NB_PACK_H3, NB_PACK_F8, NB_PACK_F6, NB_PACK_H3_UP2 = 1, 2, 4, 8


class NbPlanOptions(C.Structure):
    """``struct NbPlanOptions`` of include/neube_hip.h."""
    KNOBS = ("h3_min_pixels", "h3_min_batch", "h3_up2_w16_min_batch", "h3_up2_w8_min_batch", "small_h3", "h2_handoff",
             "early_geom_pack", "fuse_torgb", "noise_in_kernel", "positions_once", "styles_fast")
    _fields_ = [(k, C.c_int32) for k in ("conv_mode",) + KNOBS + ("noise_positions", "noise_overrides", "tap_mask", "blend_mask",
                                                                  "resume_res")]


class NbLayerPlan(C.Structure):
    """``struct NbLayerPlan``."""
    _fields_ = [("kernel", C.c_char * 64)] + [(k, C.c_int32) for k in ("kind", "in_fmt", "kernel_fmt", "out_fmt", "handoff",
                                                                       "fused_torgb", "noise_in_kernel", "packs")]


class NbGeomPlan(C.Structure):
    """``struct NbGeomPlan``."""
    _fields_ = [(k, C.c_int32) for k in ("consumer", "early_pack", "encoder_handoff", "fmt")]


class NbPassPlan(C.Structure):
    """``struct NbPassPlan``."""
    _fields_ = [(k, C.c_int32) for k in ("num_layers", "num_geom", "inkernel_from", "styles_fast", "styles_noise", "positions_once")] + [
        ("layers", NbLayerPlan * NB_PLAN_MAX_LAYERS), ("geom", NbGeomPlan * 4)]


NB_GEOM_PREP_WS_BYTES = 1040
NB_SEG_PITCH = 8
NB_SPLINE_MODES = {"uniform": 0, "cells": 1}
NB_THICK_MODES = {"fixed": 0, "range": 1, "mixture": 2}
NB_SYNTH_MAX_POINTS, NB_SYNTH_MAX_MIX, NB_SYNTH_COORD_ROUNDINGS = 64, 4, 3


class NbSplineSpec(C.Structure):
    """``struct NbSplineSpec`` of include/neube_hip.h (drawings.SplineSpec)."""
    _fields_ = [("pts_min", C.c_int32), ("pts_max", C.c_int32), ("mode", C.c_int32), ("thick_mode", C.c_int32), ("radius", C.c_float),
                ("rmin", C.c_int32), ("rmax", C.c_int32), ("n_mix", C.c_int32), ("center", C.c_float * 4), ("sigma", C.c_float * 4),
                ("cdf", C.c_float * 4)]

NB_BRUSH_METRICS_PARTS = 16
NB_BG_MEAN_PARTS = 16
NB_METRIC_PAIRS_TRANSPOSE, NB_METRIC_PAIRS_MASKED = 1, 2
NB_STITCH_PARTS = 32
NB_CLARITY_MAX_PLANES, NB_CLARITY_LOSS_PARTS, NB_CLARITY_CHUNK = 32, 8, 1024
NB_PROJECTION_PARTS = 8
NB_LPIPS_SPLIT_MAX_HW, NB_LPIPS_SPLIT_MIN_C = 1024, 64


class NbClarityPlanes(C.Structure):
    """``struct NbClarityPlanes`` of include/neube_hip.h: side and offset of every noise plane of an arena row (a host struct)."""
    _fields_ = [("n", C.c_int32), ("res", C.c_int32 * NB_CLARITY_MAX_PLANES), ("off", C.c_int32 * NB_CLARITY_MAX_PLANES)]

NB_OK, NB_EINVAL, NB_ELAUNCH, NB_EUNSUPPORTED = 0, -1, -2, -3
NB_CONV_MODES = {"f32": 0, "h3": 1, "f8": 2, "f6": 3, "f16": 4}
NB_NOISE_MODES = {"const": 0, "none": 1, "random": 2, "seeded": 3}
NB_RENDER_MODES = {"clear": 0, "full": 1}
NB_GEOM_PREPROC = {None: 0, "none": 0, "-11inverse": 1, "inverse": 2}      # encoder.HipGeometryEncoder's preproc_type strings


class NeubeHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load (once) and return the shared library; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        from . import build as _build
        override = os.environ.get("NEUBE_LIB_PATH")          # developer A/B switch: load this prebuilt library instead
        if override:
            globals()["LIB_PATH"] = override
        if not override and os.path.exists(LIB_PATH) and not os.path.exists(_build.STAMP):
            # a prebuilt library without a build stamp (packaged deployment, older checkout, built by hand with other
            # flags): its sources cannot be compared, so it is loaded as it is -- the export and ABI-version checks below
            # still apply -- and says so
            import warnings
            warnings.warn(f"{LIB_PATH} has no build stamp ({os.path.basename(_build.STAMP)}): loading it without checking that "
                          f"it was built from the kernel sources in this tree (python -m brushstroke_engine_amd.build rebuilds)")
        elif not override and _build.is_stale():
            # missing, or built from other sources than the tree holds now (kernel edits without an ABI bump would
            # otherwise run the old code silently): rebuild if a compiler is here, else fail loudly.  Multi-process
            # callers build BEFORE init_process_group (bench.py, paint_image_main, tools/bench_*.py call build.build()
            # first), so that no rank sits in a collective timeout while another compiles.
            if os.path.exists(_build.HIPCC) and os.environ.get("NEUBE_NO_AUTOBUILD") != "1":
                try:
                    _build.build(verbose=False)
                except Exception as e:                                   # noqa: BLE001
                    raise NeubeHipError(f"rebuilding the stale HIP kernel library failed: {e}") from e
            else:
                raise NeubeHipError(
                    f"HIP kernel library at {LIB_PATH} is missing or was built from different sources. Build it with "
                    f"`python -m brushstroke_engine_amd.build` (needs hipcc, gfx950). There is no CPU fallback.")
        l = C.CDLL(globals()["LIB_PATH"])
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(l, name)
            except AttributeError as e:
                raise NeubeHipError(f"{LIB_PATH} does not export {name}; rebuild the library") from e
            fn.restype = res
            fn.argtypes = args
        v = l.nb_abi_version()
        if v != ABI_VERSION:
            raise NeubeHipError(f"ABI version mismatch: library {v}, python {ABI_VERSION}; rebuild the library")
        _lib = l
        return _lib


def check(code: int, what: str) -> None:
    """Translate a negative NB_E* return code into the exception type the reference would raise
    (TORCH_CHECK failures surface as RuntimeError, bias_act.cpp:35-52)."""
    if code != 0:
        msg = lib().nb_last_error().decode("utf-8", "replace")
        raise NeubeHipError(f"{what} failed ({code}): {msg}")
