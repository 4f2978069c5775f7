"""ctypes loader for libhashmod.so (the C ABI declared in include/hashmod.h).

There is NO fallback: if the library is missing or a call fails, the product raises.
PyTorch is used only for device memory (``tensor.data_ptr()``) and streams.
"""
import ctypes as C
import os

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
# HM_LIB_PATH: kernel-experiment builds of the same ABI (profiling only)
LIB_PATH = os.environ.get("HM_LIB_PATH") or os.path.join(_PKG, "libhashmod.so")
_lib = None

_p = C.c_void_p
_i64 = C.c_int64
_int = C.c_int

# name -> (restype, argtypes); must list every symbol include/hashmod.h declares
SIGNATURES = {
    "hm_version": (_int, []),
    "hm_last_error": (C.c_char_p, []),
    "hm_device_count": (_int, []),
    "hm_grid_desc_create": (_int, [_int, _int, _p, _p, _p, C.POINTER(_p)]),
    "hm_grid_desc_destroy": (None, [_p]),
    "hm_grid_embed_dim": (_int, [_p]),
    "hm_corner_ids": (_int, [_p, _int, _p, _i64, _p, _p, _p]),
    "hm_diag_gather_calib": (_int, [_p, _i64, _i64, _int, _int, _p, _p]),
    "hm_diag_mfma_f32_stream": (_int, [_int, _int, _p, _p]),
    "hm_encode_fwd": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _int, _p]),
    "hm_encode_workspace_bytes": (_i64, [_p, _i64]),
    "hm_encode_fwd_ws": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _int, _p, _i64, _p]),
    "hm_encode_bwd_table": (_int, [_p, _p, _i64, _p, _i64, _p, _int, _p]),
    "hm_encode_bwd_workspace_bytes": (_i64, [_p, _i64]),
    "hm_encode_bwd_table_ws": (_int, [_p, _p, _i64, _p, _i64, _p, _int, _p, _i64, _p]),
    "hm_encode_rows": (_int, [_p, _p, _i64, _int, _p, _p, _p]),
    "hm_encode_bwd_table_sorted": (_int, [_p, _p, _p, _i64, _int, _p, _i64, _p, _p, _p]),
    "hm_sort_workspace_bytes": (_i64, [_i64]),
    "hm_sort_pairs_i32": (_int, [_p, _i64, _int, _p, _p, _p, _i64, _p]),
    "hm_encode_bwd_input": (_int, [_p, _p, _i64, _p, _p, _i64, _p, _p, _p]),
    "hm_encode_jvp": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _p]),
    "hm_encode_bwd_table_jvp": (_int, [_p, _p, _i64, _p, _p, _i64, _p, _p]),
    "hm_fourier_bwd_input": (_int, [_p, _i64, _p, _int, _p, _i64, _p, _p]),
    "hm_fourier_bwd_input_bwd": (_int, [_p, _i64, _p, _int, _p, _i64, _p, _p, _p, _i64, _int, _p]),
    "hm_weight_norm_multi": (_int, [_int, _int, _p, _p]),
    "hm_rownorm": (_int, [_int, _p, _p, _p, _p, _p, _i64, _int, C.c_float, _p]),
    "hm_sine": (_int, [_int, _p, _p, _p, _p, _p, _i64, C.c_float, _p]),
    "hm_posenc": (_int, [_int, _p, _int, _int, _p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p]),
    "hm_sdf_fwd": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _int, _int, _int, _p, _int, _p]),
    "hm_nffb_fwd": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _int, _p, _p]),
    "hm_sdf_fwd_emb": (_int, [_p, _p, _i64, _int, _i64, _p, _i64, _int, _int, _p, _int, _p]),
    "hm_sdf_net_fits": (_int, [_p, _int, _int]),
    "hm_diag_sdf_lds": (_int, [_p, _int, _int, _int, _p]),
    "hm_trace_workspace_bytes": (_i64, [_i64, _p]),
    "hm_trace_guard_clear": (_int, [_p, _i64, _p]),
    "hm_trace_guard_tolerances": (_int, [_p, _p]),
    "hm_trace_scan_pool_plan": (_int, [_i64, _i64, _i64, _int, _int, _i64, _int, _i64, _p, _p]),
    "hm_diag_trace_plan": (_int, [_i64, _p, _int, _int, _p]),
    "hm_trace_forward": (_int, [_p, _p, _p, _p, _int, _int, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p,
                                _i64, _p, _p]),
    "hm_trace_workspace_bytes_nffb": (_i64, [_i64, _p, _int]),
    "hm_trace_forward_nffb": (_int, [_p, _p, _p, _p, _p, _int, _int, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p,
                                     _p, _p, _i64, _p, _p]),
    "hm_pack_mlp_layer_bf16": (_int, [_p, _i64, _int, _int, _int, _p, _p]),
    "hm_sdf_fwd_bf16": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _int, _p, _i64, _p]),
    "hm_sdf_fwd_emb_bf16": (_int, [_p, _p, _i64, _int, _i64, _p, _i64, _p, _i64, _p]),
    "hm_pack_mlp_layer_split": (_int, [_p, _i64, _int, _int, _int, C.c_float, C.c_float, _int, _p, _p]),
    "hm_pack_mlp_layers_split": (_int, [_p, _int, _int, _p]),
    "hm_sdf_fwd_split": (_int, [_p, _p, _p, _i64, _p, _p, _p, _i64, _int, _p, _i64, _p]),
    "hm_sdf_fwd_emb_split": (_int, [_p, _p, _i64, _int, _i64, _p, _i64, _p, _i64, _p]),
    "hm_pack_mlp_layers": (_int, [_p, _int, _p]),
    "hm_pack_mlp_layer": (_int, [_p, _i64, _p, _int, _int, _int, _p, _p, _p, _p]),
    "hm_softplus": (_int, [_int, _p, _p, _p, _p, _p, _i64, C.c_float, C.c_float, _p]),
    "hm_sdf_head": (_int, [_int, _p, _i64, _i64, C.c_float, _p, _p, _p, _p, _p, _p]),
    "hm_colsum": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "hm_colsum_acc": (_int, [_p, _i64, _i64, _i64, _p, _p]),
    "hm_colsum_acc_multi": (_int, [_p, _int, _p]),
    "hm_copy2d_f32": (_int, [_p, _i64, _p, _i64, _i64, _i64, _p]),
    "hm_camera_rays": (_int, [_p, _p, _p, _i64, _i64, C.c_float, _p, _p, _p, _p, _p]),
    "hm_idr_loss": (_int, [_p, _p, _p, _p, _p, _i64, _p, _i64, C.c_float, C.c_float, C.c_float, _p, _p, _p, _p, _p]),
    "hm_idr_loss_dev": (_int, [_p, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _p]),
    "hm_adam_scratch_floats": (_i64, [_p, _int]),
    "hm_adam_step": (_int, [_p, _int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _p, _p]),
    "hm_adam_step_dev": (_int, [_p, _int, _p, _int, _p, _p]),
    "hm_encode_bwd_table_tracked": (_int, [_p, _p, _i64, _p, _i64, _p, _int, _p, _p, _p, _i64, _p]),
    "hm_rows_pack": (_int, [_p, _int, _p, _p, _i64, _p, _p, _p, _p]),
    "hm_rows_apply": (_int, [_p, _i64, _int, _p, _i64, _i64, _int, C.c_float, _p]),
    "hm_rows_clear": (_int, [_p, _i64, _int, _p, _i64, _i64, _int, _p, _p]),
    "hm_multi_copy_f32": (_int, [_p, _int, _p]),
    "hm_gemm_f32_group_tn": (_int, [_p, _int, _p]),
    "hm_gemm_f32_det_workspace_bytes": (_i64, [_int, _int, _i64, _i64, _i64, _i64, _i64]),
    "hm_gemm_f32_det": (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _i64, _int, _p, _i64, _p]),
    "hm_gemm_f32_group_tn_det_workspace_bytes": (_i64, [_p, _int]),
    "hm_gemm_f32_group_tn_det": (_int, [_p, _int, _p, _i64, _p]),
    "hm_gemm_f32_group_tn_add": (_int, [_p, _int, _p]),
    "hm_gemm_f32_group_tn_add_det_workspace_bytes": (_i64, [_p, _int]),
    "hm_gemm_f32_group_tn_add_det": (_int, [_p, _int, _p, _i64, _p]),
    "hm_colsum_det_workspace_bytes": (_i64, [_i64, _i64]),
    "hm_colsum_det": (_int, [_p, _i64, _i64, _i64, _p, _p, _i64, _p]),
    "hm_colsum_acc_det": (_int, [_p, _i64, _i64, _i64, _p, _p, _i64, _p]),
    "hm_colsum_acc_multi_det_workspace_bytes": (_i64, [_p, _int]),
    "hm_colsum_acc_multi_det": (_int, [_p, _int, _p, _i64, _p]),
    "hm_encode_bwd_table_sorted_tracked": (_int, [_p, _p, _p, _i64, _int, _p, _i64, _p, _p, _p, _p, _p, _i64, _p]),
    "hm_gemm_f32_ep": (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _i64, _p, _p]),
    "hm_gemm_f32": (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _i64, _int, _p]),
    "hm_diag_gemm_plan": (_int, [_int, _int, _i64, _i64, _i64, _p, _i64, _p, _i64, _int, _int, _p]),
    "hm_mc_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "hm_mc_count": (_int, [_p, _i64, _i64, _i64, _i64, _i64, _i64, C.c_float, _p, _i64, _p, _p]),
    "hm_mc_emit": (_int, [_p, _i64, _i64, _i64, _i64, _i64, _i64, C.c_float, _p, _p, _i64, _i64, _i64, _p, _p, _p,
                          _p]),
    "hm_mcs_points_bricks": (_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "hm_mcs_points_index": (_int, [_p, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p]),
    "hm_mcs_status": (_int, [_p, _i64, _p, C.c_float, _p, _p]),
    "hm_mcs_workspace_bytes": (_i64, [_i64]),
    "hm_mcs_count": (_int, [_p, _i64, _p, C.c_float, _p, _i64, _p, _p]),
    "hm_mcs_emit": (_int, [_p, _i64, _p, _p, C.c_float, _p, _p, _i64, _i64, _i64, _p, _p, _p, _p, _p, _p]),
    # eval.py's cleanup of the fine mesh: split -> hm_mesh_cc_labels, the parts' areas -> hm_mesh_cc_face_stats and
    # hm_mesh_cc_sums, components[areas.argmax()] -> hm_mesh_select_*; hm_mesh_moments is plots._surface_moments
    "hm_mesh_cc_labels": (_int, [_p, _i64, _i64, _p, _p, _p]),
    "hm_mesh_cc_face_stats": (_int, [_p, _p, _i64, _i64, _p, _p, _p, _p]),
    "hm_mesh_cc_sums_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_cc_sums": (_int, [_p, _i64, _i64, _p, _p, _p, _i64, _p, _p, _p, _i64, _p, _p]),
    "hm_mesh_moments_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_moments": (_int, [_p, _p, _i64, _i64, _p, _p, _i64, _p, _p]),
    "hm_mesh_select_mark": (_int, [_p, _i64, _i64, _p, C.c_int32, _p, _p, _p, _p]),
    "hm_mesh_select_emit": (_int, [_p, _p, _p, _i64, _i64, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p]),
    # vertex clustering (ops.mesh_simplify): keys and runs, the clusters' representatives, the face pass, the emit
    "hm_mesh_simplify_keys_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_simplify_keys": (_int, [_p, _p, _i64, _i64, _p, C.c_float, _p, _p, _p, _p, _p, _p, _i64, _p, _p]),
    "hm_mesh_simplify_clusters": (_int, [_p, _p, _i64, _p, _p, _p, _i64, _p, C.c_float, _p, _int, C.c_double, _p, _p,
                                         _p, _p]),
    "hm_mesh_simplify_face_flags": (_int, [_p, _i64, _i64, _p, _i64, _p, _p]),
    "hm_mesh_simplify_dedupe_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_simplify_dedupe": (_int, [_p, _i64, _i64, _p, _i64, _p, _p, _i64, _p, _p, _p, _p, _i64, _p]),
    "hm_mesh_simplify_emit": (_int, [_p, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _p, _p,
                                     _p]),
    # the DTU Chamfer evaluation: exact nearest neighbours on a uniform grid, triangle upsampling to a point density
    "hm_nn_workspace_bytes": (_i64, [_i64]),
    "hm_nn_build": (_int, [_p, _i64, _p, C.c_float, _p, _p, _p, _p, _i64, _p, _p]),
    "hm_nn_query": (_int, [_p, _i64, _p, _i64, _p, _p, C.c_float, _p, C.c_float, _p, _p, _p, _i64, _p, _p, _p]),
    "hm_mesh_sample_count": (_int, [_p, _p, _i64, _i64, C.c_double, _p, _p, _p, _p]),
    "hm_mesh_sample_emit": (_int, [_p, _p, _i64, _i64, C.c_double, _p, _i64, _i64, _p, _p, _p]),
    # the rest of the DTU evaluation: greedy radius down-sampling on hm_nn_build's grid, the per-point filters
    "hm_nn_radius_workspace_bytes": (_i64, [_i64]),
    "hm_nn_radius_begin": (_int, [_i64, _p, _i64, _p, _p]),
    "hm_nn_radius_rounds": (_int, [_p, _i64, _p, _p, C.c_float, _p, C.c_float, C.c_float, _i64, _i64, C.c_int32, _p,
                                   _i64, _p, _p]),
    "hm_nn_radius_finish": (_int, [_p, _i64, _p, _i64, _p, _p]),
    "hm_dtu_point_flags": (_int, [_p, _i64, _p, _p, _p, _p, _p]),
    # eval.py's per-view image scores: masked squared error (PSNR) and SSIM
    "hm_image_sqerr_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "hm_image_sqerr": (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _p, _p, _p]),
    "hm_image_ssim_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "hm_image_ssim": (_int, [_p, _p, _i64, _i64, _i64, _i64, _i64, _p, C.c_double, C.c_double, _p, _p, _p, _p]),
    # culling by camera masks and visibility: per-vertex view votes, depth maps of the mesh, the keep flags
    "hm_mesh_mask_votes": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _int, _p, _p, _p]),
    "hm_mesh_depth_workspace_bytes": (_i64, [_i64, _i64]),
    "hm_mesh_depth_maps": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _p, _p, _i64, _p, _p]),
    "hm_mesh_visible_votes": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, C.c_float, _int, _p, _p]),
    "hm_mesh_keep_mark": (_int, [_p, _i64, _i64, _p, _p, _p, _p, _p]),
    "hm_mesh_vertex_colors": (_int, [_p, _p, _i64, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, C.c_float, _i64,
                                     C.c_double, _int, _int, _int, _p, _p, _p]),
    # the mesh through a camera: the visibility buffer (nearest face per pixel) resolved with vertex attributes
    "hm_mesh_render_workspace_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "hm_mesh_render": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _p, _p, _p, _p, _p, _p,
                              _i64, _p, _p]),
    # point-to-mesh distance: the triangle grid and the exact closest point
    "hm_mesh_dist_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_dist_count": (_int, [_p, _p, _i64, _i64, _p, C.c_float, _p, _i64, _p, _p, _p, _p]),
    "hm_mesh_dist_build": (_int, [_p, _p, _i64, _i64, _p, C.c_float, _p, _p, _p, _p, _i64, _p, _i64, _p, _p, _p, _i64,
                                  _p]),
    "hm_mesh_dist_query": (_int, [_p, _i64, _p, _i64, _i64, _p, _p, C.c_float, _p, C.c_float, _p, _p, _p, _p, _p, _i64,
                                  _p, _p, _p]),
    # rays against the mesh: the index with a pad, the first hit of a ray
    "hm_mesh_index_count": (_int, [_p, _p, _i64, _i64, _p, C.c_float, _p, C.c_float, _i64, _p, _p, _p, _p]),
    "hm_mesh_index_build": (_int, [_p, _p, _i64, _i64, _p, C.c_float, _p, C.c_float, _p, _p, _p, _i64, _p, _i64, _p, _p,
                                   _p, _i64, _p]),
    "hm_mesh_ray_cast": (_int, [_p, _p, _p, _p, _i64, _p, _i64, _i64, _p, _p, C.c_float, _p, C.c_float, _p, _p, _p, _p,
                                _p, _p, _p]),
    # signed distance to the mesh: the pseudo-normal tables and the sign of a closest-point result
    "hm_mesh_topology_workspace_bytes": (_i64, [_i64]),
    "hm_mesh_topology_build": (_int, [_p, _p, _i64, _i64, _p, _p, _p, _p, _i64, _p, _p]),
    "hm_mesh_sign": (_int, [_p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    # a per-face texture atlas: the texels' points on the faces, and the sampler from (face, weights) back to texels
    "hm_mesh_texture_points": (_int, [_p, _p, _i64, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    "hm_mesh_texture_sample": (_int, [_p, _i64, _i64, _p, _p, _i64, _p, _p, _p, _p]),
}


class MlpLayer(C.Structure):
    _fields_ = [("w_packed", C.c_void_p), ("bias", C.c_void_p), ("out_dim", C.c_int32), ("n_tiles", C.c_int32),
                ("seg_octets", C.c_int32 * 2), ("seg_src", C.c_int32 * 2), ("activation", C.c_int32),
                ("post_div_sqrt2", C.c_int32), ("w_packed_m16", C.c_void_p), ("seg_blocks16", C.c_int32 * 2),
                ("w_packed_bf16", C.c_void_p), ("w_packed_split", C.c_void_p)]


class GemmEpilogue(C.Structure):
    _fields_ = [("mode", C.c_int32), ("nz", C.c_int32), ("scale", C.c_float), ("beta", C.c_float),
                ("threshold", C.c_float), ("z", C.c_void_p), ("ldz", C.c_int64), ("g", C.c_void_p), ("ldg", C.c_int64),
                ("out1", C.c_void_p), ("ld1", C.c_int64), ("out2", C.c_void_p), ("ld2", C.c_int64),
                ("out3", C.c_void_p), ("ld3", C.c_int64)]


class GemmPlanInfo(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("k_tail", C.c_int32), ("vec_a", C.c_int32), ("vec_b", C.c_int32),
                ("part", C.c_int32), ("pad_", C.c_int32), ("split", C.c_int64), ("k_chunk", C.c_int64)]


class AdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("step", C.c_void_p), ("numel", C.c_int64)]


class GemmGroupItem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("M", C.c_int64), ("N", C.c_int64),
                ("K", C.c_int64), ("lda", C.c_int64), ("ldb", C.c_int64), ("ldc", C.c_int64)]


class GemmGroupAddItem(C.Structure):
    _fields_ = GemmGroupItem._fields_ + [("A2", C.c_void_p), ("B2", C.c_void_p), ("lda2", C.c_int64), ("ldb2", C.c_int64),
                                         ("a_k0", C.c_int64), ("a_k1", C.c_int64), ("b_k0", C.c_int64), ("b_k1", C.c_int64)]


class ColsumItem(C.Structure):
    _fields_ = [("x", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int64), ("N", C.c_int64), ("ld", C.c_int64)]


class PackItem(C.Structure):
    _fields_ = [("W", C.c_void_p), ("bias", C.c_void_p), ("w_packed", C.c_void_p), ("w_packed_m16", C.c_void_p),
                ("bias_padded", C.c_void_p), ("ldw", C.c_int64), ("out_dim", C.c_int32), ("seg_width0", C.c_int32),
                ("seg_width1", C.c_int32), ("pad_", C.c_int32)]


class PackSplitItem(C.Structure):
    _fields_ = [("W", C.c_void_p), ("w_packed_split", C.c_void_p), ("ldw", C.c_int64), ("out_dim", C.c_int32),
                ("seg_width0", C.c_int32), ("seg_width1", C.c_int32), ("seg_scale0", C.c_float), ("seg_scale1", C.c_float),
                ("pad_", C.c_int32)]


class CopyItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("numel", C.c_int64)]


class TraceCfg(C.Structure):
    _fields_ = [("object_bounding_sphere", C.c_float), ("sdf_threshold", C.c_float), ("line_search_step", C.c_double),
                ("line_step_iters", C.c_int32), ("sphere_tracing_iters", C.c_int32), ("n_steps", C.c_int32),
                ("n_secant_steps", C.c_int32), ("training", C.c_int32), ("coarse_bf16", C.c_int32),
                ("sampler_head", C.c_int32)]


class TracePlanInfo(C.Structure):
    _fields_ = [("sequence", C.c_int32), ("sel_own", C.c_int32), ("head", C.c_int32), ("per_ray", C.c_int32),
                ("c_first", C.c_int32), ("k_tail", C.c_int32), ("c_ref2", C.c_int32), ("march_tail", C.c_int32),
                ("march_launched", C.c_int32), ("march_rounds", C.c_int32), ("secant", C.c_int32),
                ("scan_rule", C.c_int32), ("noise_nan", C.c_int32), ("noise_amp", C.c_float),
                ("chain_tiles", C.c_int64), ("guard_min", C.c_int64)]


class WnLayer(C.Structure):
    _fields_ = [("v", C.c_void_p), ("g", C.c_void_p), ("w", C.c_void_p), ("norm", C.c_void_p), ("grad_w", C.c_void_p),
                ("grad_v", C.c_void_p), ("grad_g", C.c_void_p), ("rows", C.c_int32), ("cols", C.c_int32)]


class NffbDesc(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("bound", C.c_float), ("w0", C.c_float), ("style_eps", C.c_float),
                ("trunk_w", C.c_void_p * 32), ("trunk_b", C.c_void_p * 32), ("out_w", C.c_void_p), ("out_b", C.c_void_p),
                ("style_w", C.c_void_p), ("style_b", C.c_void_p)]


class MlpDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("beta", C.c_float), ("layer", MlpLayer * 16), ("split_kind", C.c_int32)]


class McsLattice(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64), ("n_slots", C.c_int64),
                ("map", C.c_void_p), ("pool", C.c_void_p)]


class HashmodError(RuntimeError):
    pass


class HashmodArgumentError(HashmodError, ValueError):
    """An argument the library rejected (HM_ERR_INVALID): a HashmodError like every other failure of the library, and
    still the ValueError that the reference raises for it."""


# Parameters written through raw pointers (hm_adam_step, graph replays) do not bump torch's tensor._version, so
# every cache derived from parameter VALUES (ImplicitNetwork.packed_weights) also keys on this counter; every
# writer that bypasses ATen calls bump_param_epoch().
_param_epoch = [0]


def param_epoch():
    return _param_epoch[0]


def bump_param_epoch():
    _param_epoch[0] += 1


class PinnedRing:
    """Host staging of asynchronous host->device copies: two slots of pinned tensors of the given shapes, each guarded by
    an event.  slot() returns (*tensors, event) after the copies that last read that slot have completed; the caller
    fills the tensors, enqueues its copies (non_blocking) and records the event.  A copy engine that reads a source
    after the host has rewritten it copies the wrong values, and one whose source has been freed faults."""

    def __init__(self, *shapes):
        self._slots = [([torch.empty(s).pin_memory() for s in shapes], torch.cuda.Event()) for _ in range(2)]
        self._next = 0

    def slot(self):
        bufs, ev = self._slots[self._next]
        self._next ^= 1
        ev.synchronize()
        return (*bufs, ev)


class Workspace:
    """Grow-on-demand scratch memory of one purpose (`what`, for the error message), one uint8 buffer per device.
    A captured graph holds the buffer's address by value, so an outgrown buffer stays allocated for as long as the
    process lives (growth is geometric: the held memory is bounded by the final size) and nothing grows during a
    stream capture.  A copied or pickled Workspace starts empty."""

    def __init__(self, what):
        self.what = what
        self._live = {}     # device -> the buffer get() hands out
        self._held = []     # outgrown buffers

    def get(self, device, need):
        """a uint8 tensor of at least `need` bytes on `device` (None for need <= 0)"""
        if need <= 0:
            return None
        ws = self._live.get(device)
        if ws is None or ws.numel() < need:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"hashmod {self.what}: a {need}-byte workspace is needed during graph capture; "
                                   "run the captured work once eagerly first (warm-up) so that it is sized beforehand")
            if ws is not None:
                self._held.append(ws)
                need = max(need, 2 * ws.numel())
            ws = self._live[device] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def buffers(self, device):
        """the live buffer of `device` (if any) followed by its held ones, oldest first"""
        live = self._live.get(device)
        return ([] if live is None else [live]) + [t for t in self._held if t.device == device]

    def __reduce__(self):
        return (Workspace, (self.what,))


def lib():
    """Load libhashmod.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HashmodError(
                f"{LIB_PATH} is missing - build it with `python -m hashmodnffbanks_idr_amd.build` "
                "(hipcc --offload-arch=gfx950); there is no CPU / PyTorch fallback for the hot path")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc < 0:
        msg = lib().hm_last_error()
        msg = msg.decode() if msg else "unknown error"
        if rc == -1:
            raise HashmodArgumentError(f"hashmod: {msg}")
        raise HashmodError(f"hashmod: {msg} (code {rc}) {what}")
    return rc


def stream_ptr(t):
    """hipStream_t of torch's CURRENT stream on t's device (never the legacy default stream)."""
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HashmodError("hashmod: the hot path runs only on HIP (cuda) tensors; got a CPU tensor. "
                               "There is deliberately no CPU fallback (see oracle/ for the CPU checker).")
