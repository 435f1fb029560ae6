"""ctypes loader for libgoi_raster.so (the C ABI of include/goi_raster.h).

The library is hand-written HIP for gfx950 and is the ONLY compute path of this package: there is
no CPU or PyTorch fallback.  Loading fails loudly when the shared object is missing; calling a
compute entry point without a GPU fails inside HIP with a clear error.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libgoi_raster.so")

ABI_VERSION = 9

STAGES = ("preprocess", "depth_sort", "scan", "emit", "tile_sort", "ranges", "blend_fwd", "blend_bwd",
          "preprocess_bwd")


class GoiRasterScene(C.Structure):
    """Mirror of `struct GoiRasterScene` (include/goi_raster.h)."""
    _fields_ = [
        ("P", C.c_int), ("D", C.c_int), ("M", C.c_int), ("S", C.c_int), ("W", C.c_int), ("H", C.c_int),
        ("bg", C.c_void_p), ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("semantics", C.c_void_p), ("opacities", C.c_void_p), ("scales", C.c_void_p),
        ("scale_modifier", C.c_float), ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
        ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("prefiltered", C.c_int), ("debug", C.c_int),
    ]


ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)

# name -> (restype, argtypes): the rasterizer's frame and the families that once lived in csrc/api.hip beside it
BASE_SYMBOLS = {
    "goi_raster_abi_version": (C.c_int, []),
    "goi_raster_last_error": (C.c_char_p, []),
    "goi_raster_geom_bytes": (C.c_size_t, [C.c_int]),
    "goi_raster_image_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "goi_raster_binning_bytes": (C.c_size_t, [C.c_int]),
    "goi_raster_backward_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "goi_raster_forward": (C.c_int, [C.POINTER(GoiRasterScene), C.c_void_p, C.c_void_p, ALLOC_FN, C.c_void_p]
                           + [C.c_void_p] * 5 + [C.c_void_p, C.c_int, C.c_void_p]),
    "goi_raster_forward_async": (C.c_int, [C.POINTER(GoiRasterScene), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
                                 + [C.c_void_p] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "goi_raster_ticket_result": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint)]),
    "goi_raster_forward_redo": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
                                + [C.c_void_p] * 5 + [C.c_void_p]),
    "goi_raster_forward_reblend": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int] + [C.c_void_p] * 9),
    "goi_raster_backward": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_void_p] * 6
                            + [C.c_void_p] * 11 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_raster_debug_backward_contrib_offset": (C.c_size_t, [C.c_int, C.c_int]),
    "goi_raster_backward_semantics": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int] + [C.c_void_p] * 9),
    "goi_raster_trace": (C.c_int, [C.POINTER(GoiRasterScene), C.c_void_p, C.c_void_p, C.c_void_p, ALLOC_FN,
                                   C.c_void_p] + [C.c_void_p] * 4 + [C.c_void_p]),
    "goi_raster_mark_visible": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_void_p]),
    "goi_codebook_loss_partial_rows": (C.c_int, []),
    "goi_codebook_loss_rows": (C.c_int, [C.c_void_p] * 5 + [C.c_longlong, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4),
    "goi_codebook_sim_workspace_bytes": (C.c_size_t, []),
    "goi_codebook_sim": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "goi_codebook_dlut_partial_blocks": (C.c_int, []),
    "goi_codebook_dlut": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "goi_codebook_fused_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "goi_codebook_fused_partial_rows": (C.c_int, []),
    "goi_codebook_fused": (C.c_int, [C.c_void_p] * 5 + [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 5),
    "goi_adam_step": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "goi_adam_step_guarded": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "goi_raster_truncated_flag": (C.c_void_p, [C.c_void_p, C.c_int]),
    "goi_knn_workspace_bytes": (C.c_size_t, [C.c_int]),
    "goi_knn_dist2": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_raster_sh_grad_from_views": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "goi_raster_profile_enable": (None, [C.c_int]),
    "goi_raster_profile_stages": (None, [C.c_uint]),
    "goi_raster_profile_collect": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "goi_semantic_decode": (C.c_int, [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                      C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_semantic_osh_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]),
    "goi_semantic_osh_fit": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_int, C.c_double] + [C.c_void_p] * 6),
    "goi_semantic_dbscan_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "goi_semantic_dbscan": (C.c_int, [C.c_longlong, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "goi_semantic_mask_pack": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_semantic_mask_dilate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "goi_semantic_mask_unpack": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3),
    "goi_semantic_mask_confusion": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "goi_semantic_frame_workspace_bytes": (C.c_size_t, [C.c_int]),
    "goi_semantic_frame_compose": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_void_p]),
    "goi_semantic_pca_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "goi_semantic_pca_accumulate": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "goi_semantic_pca_solve": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_semantic_pca_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int, C.c_double,
                                         C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "goi_codebook_unique_rows_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "goi_codebook_unique_rows": (C.c_int, [C.c_void_p] + [C.c_int] * 4 + [C.POINTER(C.c_longlong), C.POINTER(C.c_uint), ALLOC_FN,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_codebook_kmeans_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_int]),
    "goi_codebook_kmeans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong] + [C.c_int] * 3
                            + [C.c_void_p] * 5),
    "goi_raster_photometric_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_uint]),
    "goi_raster_photometric_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                          C.c_uint] + [C.c_void_p] * 4),
    "goi_raster_photometric_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.c_uint] + [C.c_void_p] * 5),
    "goi_raster_densify_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "goi_raster_densify_stats": (C.c_int, [C.c_longlong, C.c_void_p, C.c_longlong] + [C.c_void_p] * 4),
    "goi_raster_densify_plan": (C.c_int, [C.c_longlong] + [C.c_void_p] * 4 + [C.c_double] * 3 + [C.c_int, C.c_double, C.c_double]
                                + [C.c_void_p] * 3),
    "goi_raster_densify_prune_plan": (C.c_int, [C.c_longlong] + [C.c_void_p] * 4),
    "goi_raster_densify_apply": (C.c_int, [C.c_longlong, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_longlong, C.c_longlong]
                                 + [C.c_void_p] * 2),
    "goi_raster_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "goi_raster_blend_stats": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 5),
    "goi_raster_contrib_frame": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 7),
    "goi_raster_contrib_votes": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2),
    "goi_raster_debug_views": (C.c_int, [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_void_p] * 8 + [C.c_void_p]),
    "goi_raster_debug_sort_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int]),
    "goi_raster_debug_sort_pairs": (C.c_int, [C.c_void_p] * 4 + [C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
                                    + [C.c_void_p] * 3),
    "goi_raster_debug_scan_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "goi_raster_debug_exclusive_scan": (C.c_int, [C.c_void_p] * 3 + [C.c_longlong] + [C.c_void_p] * 4),
    "goi_raster_debug_reduce_row_floats": (C.c_int, [C.c_int, C.c_int]),
    "goi_raster_debug_reduce_workspace_bytes": (C.c_size_t, [C.c_longlong]),
    "goi_raster_debug_reduce_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 14),
    "goi_raster_debug_preprocess_backward": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int, C.c_int, C.c_int, C.c_longlong]
                                             + [C.c_void_p] * 22),
    "goi_raster_debug_pair_eval": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_void_p] * 4),
    "goi_raster_debug_backward_blend": (C.c_int, [C.POINTER(GoiRasterScene), C.c_int, C.c_int] + [C.c_void_p] * 24),
}

_LL, _P, _I = C.c_longlong, C.c_void_p, C.c_int
# the goi_field_* family (csrc/field.hip: density grid and iso-surface)
FIELD_SYMBOLS = {
    "goi_field_density_workspace_bytes": (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_double]),
    "goi_field_density": (C.c_int, [C.c_longlong] + [C.c_void_p] * 5 + [C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_double] + [C.c_void_p] * 9),
    "goi_field_iso_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "goi_field_iso_count": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "goi_field_iso_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 4
                           + [C.c_longlong, C.c_longlong] + [C.c_void_p] * 4),
}
# the goi_mesh_* family (csrc/mesh.hip: components, clean-up, vertex clustering, normals)
MESH_SYMBOLS = {
    "goi_mesh_components_workspace_bytes": (C.c_size_t, [_LL, _LL]),
    "goi_mesh_components": (C.c_int, [_LL, _LL] + [_P] * 6),
    "goi_mesh_clean_workspace_bytes": (C.c_size_t, [_LL, _LL]),
    "goi_mesh_clean_plan": (C.c_int, [_LL, _LL, _P, _P, _LL, C.c_double, _P, _P, _P]),
    "goi_mesh_clean_emit": (C.c_int, [_LL, _LL] + [_P] * 4 + [_LL, _LL] + [_P] * 6),
    "goi_mesh_decimate_workspace_bytes": (C.c_size_t, [_LL, _LL]),
    "goi_mesh_decimate_members": (C.c_int, [_LL, _LL] + [_P] * 4),
    "goi_mesh_decimate_probe": (C.c_int, [_LL, _LL, _P, _P, C.c_int, _P, _P, _P]),
    "goi_mesh_decimate_plan": (C.c_int, [_LL, _LL, _P, _P, C.c_int, _P, _P, _P]),
    "goi_mesh_decimate_emit": (C.c_int, [_LL, _LL, _P, _P, C.c_int, C.c_int, _P, _LL, _LL] + [_P] * 5),
    "goi_mesh_normals_workspace_bytes": (C.c_size_t, [_LL, _LL]),
    "goi_mesh_normals": (C.c_int, [_LL, _LL] + [_P] * 6),
}
# the goi_texture_* family (csrc/texture.hip: rasterize, resolve, grid put, accumulate, fill)
TEXTURE_SYMBOLS = {
    "goi_texture_rasterize_workspace_bytes": (C.c_size_t, [_LL, _I, _I]),
    "goi_texture_rasterize": (C.c_int, [_LL, _LL, _P, _P, _I, _I] + [_P] * 6),
    "goi_texture_resolve": (C.c_int, [_LL, _LL, _LL, _I, _I] + [_P] * 13),
    "goi_texture_grid_put_workspace_bytes": (C.c_size_t, [_LL, _I, _I, _I]),
    "goi_texture_grid_put": (C.c_int, [_LL, _I, _I, _I, _I] + [_P] * 12),
    "goi_texture_accumulate": (C.c_int, [_LL, _I] + [_P] * 5),
    "goi_texture_normalize": (C.c_int, [_LL, _I] + [_P] * 5),
    "goi_texture_fill_workspace_bytes": (C.c_size_t, [_I, _I]),
    "goi_texture_fill": (C.c_int, [_I, _I, _I, _I] + [_P] * 6),
}
# the goi_edit_* family (csrc/edit.hip: bounds of a selection, rigid transform in place)
EDIT_SYMBOLS = {
    "goi_edit_bounds_workspace_bytes": (C.c_size_t, [_LL]),
    "goi_edit_bounds": (C.c_int, [_LL, _P, _P, _I, _P, _P, _P, _P]),
    "goi_edit_transform": (C.c_int, [_LL, _I, _P, _I, _P] + [_P] * 9),
}
# the k-NN graph (csrc/knn.hip: goi_knn_graph, goi_knn_majority), written in its own unit from the start
KNN_GRAPH_SYMBOLS = {
    "goi_knn_graph_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "goi_knn_graph": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "goi_knn_majority": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int] + [C.c_void_p] * 4),
}
# the goi_pose_* family (csrc/pose.hip: the pose gradient of a selection from one backward's gradients)
POSE_SYMBOLS = {
    "goi_pose_gradient_workspace_bytes": (C.c_size_t, [_LL]),
    "goi_pose_gradient": (C.c_int, [_LL, _I, _P, _I] + [_P] * 14),
}
# the neighbour-consistency loss and feature diffusion on a k-NN graph (csrc/smooth.hip)
SMOOTH_SYMBOLS = {
    "goi_knn_transpose_workspace_bytes": (C.c_size_t, [_I, _I]),
    "goi_knn_transpose": (C.c_int, [_I, _I] + [_P] * 5),
    "goi_knn_smooth_loss_workspace_bytes": (C.c_size_t, [_I]),
    "goi_knn_smooth_loss": (C.c_int, [_I, _I, _I] + [_P] * 11),
    "goi_knn_diffuse": (C.c_int, [_I, _I, _I] + [_P] * 4 + [C.c_float, _P, _P]),
}
# the edge gate and the connected components of a k-NN graph (csrc/segment.hip)
SEGMENT_SYMBOLS = {
    "goi_knn_segment_edges": (C.c_int, [_I, _I, _I, _P, _P, C.c_float, _P, C.c_float, _I, _P, _P, _P, _P]),
    "goi_knn_segment_components_workspace_bytes": (C.c_size_t, [_I, _I]),
    "goi_knn_segment_components": (C.c_int, [_I, _I, _P, _P, _P, _I] + [_P] * 7),
}
# the partition as member lists and the per-instance statistics (csrc/instance.hip); like the goi_pose_* family
# these names carry a prefix of their own, so they are bound through LATER_TABLES and are not part of SYMBOLS below
INSTANCE_SYMBOLS = {
    "goi_instance_members_workspace_bytes": (C.c_size_t, [_I, _I]),
    "goi_instance_members": (C.c_int, [_I, _I] + [_P] * 5),
    "goi_instance_stats_workspace_bytes": (C.c_size_t, [_I, _I]),
    "goi_instance_stats": (C.c_int, [_I, _I, _I] + [_P] * 16),
}
# the mask-contrast loss of a rendered feature map against one view's 2D instance masks (csrc/grouping.hip); a prefix
# of its own again: bound through LATER_TABLES, not part of SYMBOLS below
GROUPING_SYMBOLS = {
    "goi_mask_contrast_workspace_bytes": (C.c_size_t, [_I] * 4),
    "goi_mask_contrast": (C.c_int, [_I] * 4 + [_P, _P, C.c_float, C.c_float, C.c_float, _I, C.c_float] + [_P] * 10),
}
# the fixed-budget densification (csrc/mcmc.hip); a prefix of its own: bound through LATER_TABLES
MCMC_SYMBOLS = {
    "goi_mcmc_relocate_workspace_bytes": (C.c_size_t, [_LL]),
    "goi_mcmc_relocate": (C.c_int, [_LL, _P, _P, _LL, _P, C.c_double, _LL, _LL, _LL, _I, _P, _I] + [_P] * 5),
    "goi_mcmc_noise": (C.c_int, [_LL] + [_P] * 6 + [C.c_double] * 3 + [_P]),
    "goi_mcmc_debug_relocation_sum": (C.c_int, [_I] + [_P] * 4),
}
# the as-rigid-as-possible deformation of a selection (csrc/deform.hip); a prefix of its own: bound through LATER_TABLES
DEFORM_SYMBOLS = {
    "goi_deform_solve_workspace_bytes": (C.c_size_t, [_I]),
    "goi_deform_solve": (C.c_int, [_I, _I] + [_P] * 7 + [_I, _I, C.c_float] + [_P] * 4),
    "goi_deform_energy_workspace_bytes": (C.c_size_t, [_I]),
    "goi_deform_energy": (C.c_int, [_I, _I] + [_P] * 8),
    "goi_deform_apply": (C.c_int, [_LL, _I, _I, _I, _P, _I, _P, _P, C.c_float] + [_P] * 10 + [_I, _P]),
}
# every symbol include/goi_raster.h declares under the goi_raster / semantic / knn / adam / codebook prefixes
SYMBOLS = {**BASE_SYMBOLS, **KNN_GRAPH_SYMBOLS, **SMOOTH_SYMBOLS, **SEGMENT_SYMBOLS}
# The entries that were MOVED out of csrc/api.hip into their families' units, with the frame's own: the set whose refusals
# tests/test_entry_refusals_cpu.py records as they were before the move.  Entries added since are in LATER_TABLES and bring
# their refusals in their own test files (tests/test_knn_graph_cpu.py, tests/test_pose_cpu.py, tests/test_smooth_entry_refusals_cpu.py,
# tests/test_segment_entry_refusals_cpu.py, tests/test_instance_entry_refusals_cpu.py, tests/test_grouping_entry_refusals_cpu.py,
# tests/test_mcmc_entry_refusals_cpu.py, tests/test_deform_entry_refusals_cpu.py).
# load() binds both.
SYMBOL_TABLES = (BASE_SYMBOLS, FIELD_SYMBOLS, MESH_SYMBOLS, TEXTURE_SYMBOLS, EDIT_SYMBOLS)
LATER_TABLES = (KNN_GRAPH_SYMBOLS, POSE_SYMBOLS, SMOOTH_SYMBOLS, SEGMENT_SYMBOLS, INSTANCE_SYMBOLS, GROUPING_SYMBOLS,
                MCMC_SYMBOLS, DEFORM_SYMBOLS)

_lib = None


def load():
    """Returns the loaded library; raises if it has not been built (python -m goi_hyperplane_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
                "`python -m goi_hyperplane_amd.build` (needs hipcc; cross-compiles for gfx950 without a GPU). "
                "There is deliberately no CPU fallback.")
        # The tensors this library is handed live in the HIP runtime PyTorch loaded: that copy of libamdhip64 must
        # be the one in the process before ours resolves its dependency (loaded first, libgoi_raster.so would pull in
        # the system copy and the two runtimes would not see each other's devices and allocations).
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for table in SYMBOL_TABLES + LATER_TABLES:
            for name, (res, args) in table.items():
                fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
                fn.restype = res
                fn.argtypes = args
        got = lib.goi_raster_abi_version()
        if got != ABI_VERSION:
            raise ImportError(f"libgoi_raster.so ABI {got} != expected {ABI_VERSION}; rebuild")
        _lib = lib
        # experiment switches, e.g. GOI_OPTIONS="sort_variant=1,bwd_variant=1"
        for item in filter(None, os.environ.get("GOI_OPTIONS", "").split(",")):
            name, _, value = item.partition("=")
            if lib.goi_raster_set_option(name.strip().encode(), int(value)) < 0:
                raise RuntimeError(lib.goi_raster_last_error().decode())
            OPTIONS[name.strip()] = int(value)
    return _lib


def last_error() -> str:
    return load().goi_raster_last_error().decode("utf-8", "replace")


# ---- what every module's calls into the library share --------------------------------------------------------------------
def check(r, exc=RuntimeError):
    """The return value of a library call: raises `exc` with the library's message when it is negative."""
    if r < 0:
        raise exc(last_error())
    return r


def ptr(t):
    """Device pointer of a tensor (an empty one included: the C entries go by counts), None for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(dev):
    import torch
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def workspace(nbytes, dev):
    import torch
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


class TensorAlloc:
    """An allocation callback to hand to the library (`.cb`): `make(nbytes)` returns the tensor, which is kept in `.tensor`;
    an exception it raises is kept in `.error` for the caller to re-raise, because none may cross the C boundary."""

    def __init__(self, make, tensor=None):
        self.make, self.tensor, self.error = make, tensor, None
        self.cb = ALLOC_FN(self._alloc)

    def _alloc(self, _user, nbytes):
        try:
            self.tensor = self.make(int(nbytes))
            return self.tensor.data_ptr()
        except Exception as ex:  # noqa: BLE001
            self.error = ex
            return None


class GoiAdamGroup(C.Structure):
    """include/goi_raster.h: GoiAdamGroup"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_longlong), ("row_len", C.c_int), ("step_size", C.c_float), ("bc2_sqrt", C.c_float)]


ADAM_MAX_GROUPS = 8


class GoiDensifyRows(C.Structure):
    """include/goi_raster.h: GoiDensifyRows"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("rows", C.c_longlong), ("row_len", C.c_int), ("mode", C.c_int)]


DENSIFY_MAX_GROUPS = 24


class GoiMcmcRows(C.Structure):
    """include/goi_raster.h: GoiMcmcRows"""
    _fields_ = [("data", C.c_void_p), ("row_len", C.c_int), ("mode", C.c_int)]


MCMC_MAX_GROUPS = 24
MCMC_PARAM, MCMC_OPACITY, MCMC_SCALING, MCMC_MOMENT = 0, 1, 2, 3  # GOI_MCMC_* of include/goi_raster.h


class GoiDeformSH(C.Structure):
    """include/goi_raster.h: GoiDeformSH"""
    _fields_ = [("dirs1", C.c_float * 9), ("dirs2", C.c_float * 15), ("dirs3", C.c_float * 21), ("inv1", C.c_float * 9),
                ("inv2", C.c_float * 25), ("inv3", C.c_float * 49)]


class GoiEditTransform(C.Structure):
    """include/goi_raster.h: GoiEditTransform"""
    _fields_ = [("R", C.c_float * 9), ("q", C.c_float * 4), ("t", C.c_float * 3), ("pivot", C.c_float * 3), ("s", C.c_float),
                ("log_s", C.c_float), ("flags", C.c_int), ("D1", C.c_float * 9), ("D2", C.c_float * 25), ("D3", C.c_float * 49)]


EDIT_ROTATE, EDIT_SCALE = 1, 2  # GOI_EDIT_* of include/goi_raster.h


OPTIONS = {}  # the switches set through set_option / GOI_OPTIONS in this process (name -> value)


def set_option(name: str, value: int) -> None:
    check(load().goi_raster_set_option(name.encode(), int(value)))
    OPTIONS[name] = int(value)


def profile_enable(on: bool) -> None:
    load().goi_raster_profile_enable(1 if on else 0)


def profile_stages(names) -> None:
    """Record events only around the named stages (cheaper than profile_enable inside a timed region)."""
    load().goi_raster_profile_stages(sum(1 << STAGES.index(n) for n in names))


def profile_collect() -> dict:
    """{stage: (milliseconds, launches)} accumulated since the previous collect."""
    n = len(STAGES)
    ms = (C.c_double * n)()
    calls = (C.c_int * n)()
    check(load().goi_raster_profile_collect(ms, calls))
    return {STAGES[i]: (ms[i], calls[i]) for i in range(n)}
