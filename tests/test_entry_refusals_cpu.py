"""What the C entries of the stand-alone families refuse before they touch the device, without a GPU: each family's unit
(csrc/mesh.hip, csrc/pca.hip, ...) defines its own extern "C" entries, and every refusal ends in the one thread_local message of
csrc/api.hip that goi_raster_last_error returns.  Per entry: the message of its first refusal; where it takes a workspace, the
messages for a NULL and for a misaligned one; per size function, the 0 it returns for an argument out of range.  The strings
were recorded from the library as it was when every one of these entries still lived in csrc/api.hip.

The same for the rasterizer's direct-test and diagnostic entries that live beside their kernels (the RASTER tables below): for
those, every refusal and every return of 0 that comes before the entry's first HIP call.

And for the entries of the rasterizer's frame in csrc/api.hip (the FRAME table): forward, asynchronous forward and its ticket,
redo, reblend, backward, semantics-only backward, trace, truncated flag.  Recorded from the library of ABI 8 through the widest
entry of each operation, before ABI 9 folded the narrower ones into it.
"""
import ctypes as C
import threading

import pytest

F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 4)  # 4-byte aligned, not 256
N = None
WS = object()  # where a workspace case puts the workspace under test

_COUNTS = (C.c_longlong * 1)()
_FLAGS = C.c_uint(0)
_MAPS = (C.c_void_p * 1)(F.value)
_ALLOC = _NO_ALLOC = None  # made with the library's callback type in the fixture: a callback, and the NULL one


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    global _ALLOC, _NO_ALLOC
    _ALLOC = _lib.ALLOC_FN(lambda user, nbytes: None)
    _NO_ALLOC = _lib.ALLOC_FN()
    return _lib.load()


def _call(lib, fn, args, ws=None):
    args = tuple(ws if a is WS else _ALLOC if a == "alloc" else _NO_ALLOC if a == "no alloc" else a for a in args)
    return getattr(lib, fn)(*args)


def _err(lib):
    return lib.goi_raster_last_error().decode()


_UNIQ = (_MAPS, 1, 4, 8, 8, _COUNTS, C.byref(_FLAGS), "alloc", N)

# entry, arguments, the message of its first refusal
FIRST = [
    ("goi_semantic_decode", (N, 16, 64, F, F, 300, N, 0.0, F, F, F, N), "goi_semantic_decode: NULL input"),
    ("goi_semantic_osh_counts", (F, F, -1, 300, F, N), "goi_semantic_osh_counts: bad HW"),
    ("goi_semantic_osh_fit", (F, 0, 256, F, 64, 1, F, F, 0.1, 10, 0.9, F, F, F, F, N, N),
     "goi_semantic_osh_fit: need 1 <= n_codes <= 1000"),
    ("goi_semantic_dbscan", (-1, F, 0.1, 1, F, F, F, F, N), "goi_semantic_dbscan: need 0 <= n < 2^30"),
    ("goi_semantic_mask_pack", (F, 0, 1, 0, 8, 0, F, F, N), "goi_semantic_mask_pack: need H >= 1 and W >= 1"),
    ("goi_semantic_mask_dilate", (F, F, 1, 0, 8, 1, N), "goi_semantic_mask_dilate: need H >= 1 and W >= 1"),
    ("goi_semantic_mask_unpack", (F, 1, 0, 8, 1, N, F, N), "goi_semantic_mask_unpack: need H >= 1 and W >= 1"),
    ("goi_semantic_mask_confusion", (F, F, 1, 0, 8, F, N), "goi_semantic_mask_confusion: need H >= 1 and W >= 1"),
    ("goi_semantic_frame_compose", (F, 3, F, F, 1, 0, 8, 0, 0, 0.5, 0.5, F, 16, F, 0, F, N),
     "goi_semantic_frame_compose: need H >= 1 and W >= 1"),
    ("goi_semantic_frame_compose", (F, 3, F, F, 1, 8, 8, 3, 0, 0.5, 0.5, F, 16, F, 0, N, N),
     "goi_semantic_frame_compose: NULL workspace"),
    ("goi_semantic_pca_accumulate", (F, 0, 2, 10, N, 1, F, N), "goi_semantic_pca_accumulate: need 3 <= S <= 32"),
    ("goi_semantic_pca_solve", (2, F, F, N), "goi_semantic_pca_solve: need 3 <= S <= 32"),
    ("goi_semantic_pca_apply", (F, 0, 2, 10, 1, F, 0, 2.0, F, 0, F, N), "goi_semantic_pca_apply: need 3 <= S <= 32"),
    ("goi_semantic_pca_apply", (F, 0, 3, 10, 1, F, 2, 2.0, F, 0, N, N),
     "goi_semantic_pca_apply: GOI_PCA_MINMAX needs a 4-byte aligned workspace"),
    ("goi_semantic_pca_apply", (F, 0, 3, 10, 1, F, 2, 2.0, F, 0, C.c_void_p((1 << 20) + 2), N),
     "goi_semantic_pca_apply: GOI_PCA_MINMAX needs a 4-byte aligned workspace"),
    ("goi_field_density", (-1, F, F, F, F, N, 0, 0.1, N, N, 64, 8, 1.0, F, F, F, F, N, F, F, F, N),
     "goi_field_density: need 0 <= P < 2^30"),
    ("goi_field_density", (10, F, F, F, F, N, 0, 0.1, N, N, 64, 2, 1.0, F, F, F, F, N, F, F, F, N),
     "goi_field_density: need resolution <= 256, resolution % num_blocks == 0, 4 <= resolution / num_blocks <= 16 "
     "and 0 <= relax_ratio <= 4"),
    ("goi_field_iso_count", (F, 0, 4, 4, 0.5, F, F, N), "goi_field_iso_count: need X, Y, Z >= 1 and X Y Z <= 2^26"),
    ("goi_field_iso_emit", (F, N, 0, 4, 4, 0.5, F, F, F, F, 1, 1, F, F, N, N),
     "goi_field_iso_emit: need X, Y, Z >= 1 and X Y Z <= 2^26"),
    ("goi_mesh_components", (-1, 4, F, F, F, F, F, N), "goi_mesh_components: need 0 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_clean_plan", (0, 4, F, F, 1, 0.0, F, F, N), "goi_mesh_clean_plan: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_clean_emit", (0, 4, F, F, N, F, 1, 1, F, F, N, F, F, N), "goi_mesh_clean_emit: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_decimate_members", (0, 4, F, F, F, N), "goi_mesh_decimate_members: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_decimate_probe", (0, 4, F, F, 8, F, F, N), "goi_mesh_decimate_probe: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_decimate_probe", (4, 4, F, F, 0, F, F, N), "goi_mesh_decimate_probe: need 1 <= divisions <= 1024"),
    ("goi_mesh_decimate_plan", (0, 4, F, F, 8, F, F, N), "goi_mesh_decimate_plan: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_decimate_emit", (0, 4, F, N, 8, 0, F, 1, 1, F, F, N, F, N),
     "goi_mesh_decimate_emit: need 1 <= V, F and V, 3 F < 2^30"),
    ("goi_mesh_normals", (-1, 4, F, F, F, F, F, N), "goi_mesh_normals: need 0 <= V, F and V, 3 F < 2^30"),
    ("goi_texture_rasterize", (-1, 4, F, F, 8, 8, F, F, F, F, F, N), "goi_texture_rasterize: need 0 <= V, F and V, 3 F < 2^30"),
    ("goi_texture_rasterize", (4, 4, F, F, 0, 8, F, F, F, F, F, N), "goi_texture_rasterize: need 1 <= H, W <= 16384"),
    ("goi_texture_resolve", (-1, 4, 4, 8, 8) + (F,) * 12 + (N,), "goi_texture_resolve: need 0 <= V, F and V, 3 F < 2^30"),
    ("goi_texture_grid_put", (-1, 3, 8, 8, 1, F, F, N, F, F, N, N, N, N, F, F, N),
     "goi_texture_grid_put: need 0 <= N < 2^28, 1 <= C <= 4 and 1 <= H, W <= 16384"),
    ("goi_texture_accumulate", (-1, 3, F, F, F, F, N), "goi_texture_accumulate: need 0 <= T <= 16384^2 and 1 <= C <= 4"),
    ("goi_texture_normalize", (-1, 3, F, F, F, F, N), "goi_texture_normalize: need 0 <= T <= 16384^2 and 1 <= C <= 4"),
    ("goi_texture_fill", (0, 8, 3, 1, F, F, F, F, F, N), "goi_texture_fill: need 1 <= H, W <= 16384"),
    ("goi_edit_bounds", (-1, F, N, 0, F, F, F, N), "goi_edit_bounds: need 0 <= P < 2^31"),
    ("goi_edit_transform", (-1, 1, N, 0, F, F, F, F, N, N, N, N, N, N), "goi_edit_transform: need 0 <= P < 2^31"),
    ("goi_codebook_unique_rows", (_MAPS, -1, 4, 8, 8, _COUNTS, C.byref(_FLAGS), "alloc", N, F, N),
     "goi_codebook_unique_rows: need n_views >= 0 and D, H, W >= 1"),
    ("goi_codebook_kmeans", (F, F, -1, 4, 4, 8, 2, 1, F, F, F, F, N), "goi_codebook_kmeans: need 0 <= n_problems <= 65535"),
    ("goi_raster_photometric_forward", (F, F, 1, 3, 8, 8, 7, 0.2, 0, F, N, F, N),
     "goi_raster_photometric_forward: window_size 7 is not supported (only 11)"),
    ("goi_raster_photometric_backward", (F, F, 1, 3, 8, 8, 7, 0.2, 1, F, F, F, N, N),
     "goi_raster_photometric_backward: window_size 7 is not supported (only 11)"),
    ("goi_raster_densify_stats", (-1, F, 2, F, F, F, N), "goi_raster_densify_stats: need 0 <= P < 2^31"),
    ("goi_raster_densify_plan", (-1, F, F, F, F, 0.1, 0.1, 0.1, 0, 1.0, 1.0, F, F, N),
     "goi_raster_densify_plan: need 0 <= P < 2^30"),
    ("goi_raster_densify_prune_plan", (-1, F, F, F, N), "goi_raster_densify_prune_plan: need 0 <= P < 2^30"),
    ("goi_raster_densify_apply", (-1, N, 0, N, N, N, 0, 0, F, N), "goi_raster_densify_apply: need 0 <= P < 2^30"),
    ("goi_codebook_loss_rows", (F, F, F, F, N, -1, 300, 16, 1.0, F, F, F, N), "goi_codebook_loss_rows: bad HW"),
    ("goi_codebook_loss_rows", (F, F, F, F, N, 64, 300, 17, 1.0, F, F, F, N),
     "goi_codebook_loss_rows: supported sizes are 1 <= S <= 16, 1 <= C <= 512"),
    ("goi_codebook_sim", (N, F, 64, 300, 256, F, F, F, N), "goi_codebook_sim: a required pointer is NULL"),
    ("goi_codebook_sim", (F, F, 64, 300, 256, F, F, N, N), "goi_codebook_sim: a required pointer is NULL"),  # (its workspace)
    ("goi_codebook_dlut", (N, F, 64, 300, 256, F, N), "goi_codebook_dlut: bad arguments"),
    ("goi_codebook_fused", (N, F, F, F, N, 64, 300, 256, 16, 1.0, F, F, F, F, N), "goi_codebook_fused: a required pointer is NULL"),
    ("goi_adam_step", (N, -1, 0.9, 0.999, 1e-15, N, N), "goi_adam_step: n_groups must be 0..8"),
    ("goi_adam_step_guarded", (N, 9, 0.9, 0.999, 1e-15, N, N, N), "goi_adam_step: n_groups must be 0..8"),
    ("goi_knn_dist2", (-1, F, F, F, N), "goi_knn_dist2: bad P"),
    ("goi_knn_dist2", (1 << 30, F, F, F, N), "goi_knn_dist2: need P < 2^30"),
]

# entry, arguments around its workspace, the messages for a NULL and for a misaligned workspace.  (goi_semantic_dbscan clears
# `result` on the stream before it looks at its workspace, goi_semantic_frame_compose and goi_semantic_pca_apply have a
# workspace rule of their own and goi_codebook_sim only a NULL check: FIRST above.)
WORKSPACE = [
    ("goi_semantic_pca_accumulate", (F, 0, 3, 10, N, 1, WS, N),
     "goi_semantic_pca_accumulate: NULL workspace", "goi_semantic_pca_accumulate: workspace must be 256-byte aligned"),
    ("goi_semantic_pca_solve", (3, WS, F, N),
     "goi_semantic_pca_solve: NULL workspace", "goi_semantic_pca_solve: workspace must be 256-byte aligned"),
    ("goi_field_density", (10, F, F, F, F, N, 0, 0.1, N, N, 64, 8, 1.0, F, F, F, F, N, F, F, WS, N),
     "goi_field_density: NULL workspace", "goi_field_density: workspace must be 256-byte aligned"),
    ("goi_field_iso_count", (F, 4, 4, 4, 0.5, WS, F, N),
     "goi_field_iso_count: NULL workspace", "goi_field_iso_count: workspace must be 256-byte aligned"),
    ("goi_field_iso_emit", (F, N, 4, 4, 4, 0.5, F, F, F, WS, 1, 1, F, F, N, N),
     "goi_field_iso_emit: NULL workspace", "goi_field_iso_emit: workspace must be 256-byte aligned"),
    ("goi_mesh_components", (4, 4, F, F, F, F, WS, N),
     "goi_mesh_components: NULL workspace", "goi_mesh_components: workspace must be 256-byte aligned"),
    ("goi_mesh_clean_plan", (4, 4, F, F, 1, 0.0, WS, F, N),
     "goi_mesh_clean_plan: NULL workspace", "goi_mesh_clean_plan: workspace must be 256-byte aligned"),
    ("goi_mesh_clean_emit", (4, 4, F, F, N, WS, 1, 1, F, F, N, F, F, N),
     "goi_mesh_clean_emit: NULL workspace", "goi_mesh_clean_emit: workspace must be 256-byte aligned"),
    ("goi_mesh_decimate_members", (4, 4, F, F, WS, N),
     "goi_mesh_decimate_members: NULL workspace", "goi_mesh_decimate_members: workspace must be 256-byte aligned"),
    ("goi_mesh_decimate_probe", (4, 4, F, F, 8, WS, F, N),
     "goi_mesh_decimate_probe: NULL workspace", "goi_mesh_decimate_probe: workspace must be 256-byte aligned"),
    ("goi_mesh_decimate_plan", (4, 4, F, F, 8, WS, F, N),
     "goi_mesh_decimate_plan: NULL workspace", "goi_mesh_decimate_plan: workspace must be 256-byte aligned"),
    ("goi_mesh_decimate_emit", (4, 4, F, N, 8, 0, WS, 1, 1, F, F, N, F, N),
     "goi_mesh_decimate_emit: NULL workspace", "goi_mesh_decimate_emit: workspace must be 256-byte aligned"),
    ("goi_mesh_normals", (4, 4, F, F, F, F, WS, N),
     "goi_mesh_normals: NULL workspace", "goi_mesh_normals: workspace must be 256-byte aligned"),
    ("goi_texture_rasterize", (4, 4, F, F, 8, 8, F, F, F, F, WS, N),
     "goi_texture_rasterize: NULL workspace", "goi_texture_rasterize: workspace must be 256-byte aligned"),
    ("goi_texture_grid_put", (4, 3, 8, 8, 1, F, F, N, F, F, N, N, N, N, F, WS, N),
     "goi_texture_grid_put: NULL workspace", "goi_texture_grid_put: workspace must be 256-byte aligned"),
    ("goi_texture_fill", (8, 8, 3, 1, F, F, F, F, WS, N),
     "goi_texture_fill: NULL workspace", "goi_texture_fill: workspace must be 256-byte aligned"),
    ("goi_edit_bounds", (4, F, N, 0, F, F, WS, N),
     "goi_edit_bounds: NULL workspace", "goi_edit_bounds: workspace must be 256-byte aligned"),
    ("goi_codebook_unique_rows", _UNIQ + (WS, N),
     "goi_codebook_unique_rows: NULL workspace", "goi_codebook_unique_rows: workspace must be 256-byte aligned"),
    ("goi_codebook_kmeans", (F, F, 1, 4, 4, 8, 2, 1, F, F, F, WS, N),
     "goi_codebook_kmeans: NULL workspace", "goi_codebook_kmeans: workspace must be 256-byte aligned"),
    ("goi_raster_photometric_forward", (F, F, 1, 3, 8, 8, 11, 0.2, 0, F, N, WS, N),
     "goi_raster_photometric_forward: NULL workspace", "goi_raster_photometric_forward: workspace must be 256-byte aligned"),
    ("goi_raster_photometric_backward", (F, F, 1, 3, 8, 8, 11, 0.2, 1, F, WS, F, N, N),
     "goi_raster_photometric_backward: NULL workspace", "goi_raster_photometric_backward: workspace must be 256-byte aligned"),
    ("goi_raster_densify_plan", (4, F, F, F, F, 0.1, 0.1, 0.1, 0, 1.0, 1.0, F, WS, N),
     "goi_raster_densify_plan: NULL workspace", "goi_raster_densify_plan: workspace must be 256-byte aligned"),
    ("goi_raster_densify_prune_plan", (4, F, F, WS, N),
     "goi_raster_densify_prune_plan: NULL workspace", "goi_raster_densify_prune_plan: workspace must be 256-byte aligned"),
    ("goi_raster_densify_apply", (4, N, 0, N, N, N, 0, 0, WS, N),
     "goi_raster_densify_apply: NULL workspace", "goi_raster_densify_apply: workspace must be 256-byte aligned"),
    ("goi_codebook_fused", (F, F, F, F, N, 64, 300, 256, 16, 1.0, F, F, F, WS, N),
     "goi_codebook_fused: NULL workspace", "goi_codebook_fused: workspace must be 256-byte aligned"),
    ("goi_knn_dist2", (4, F, F, WS, N), "goi_knn_dist2: NULL workspace", "goi_knn_dist2: workspace must be 256-byte aligned"),
]

# size function, one argument list out of its range: every one of them answers 0
SIZES = [
    ("goi_semantic_dbscan_workspace_bytes", (0,)), ("goi_semantic_dbscan_workspace_bytes", (1 << 30,)),
    ("goi_semantic_frame_workspace_bytes", (0,)), ("goi_semantic_pca_workspace_bytes", (2, 1)),
    ("goi_semantic_pca_workspace_bytes", (3, 65536)), ("goi_field_density_workspace_bytes", (0, 64, 8, 1.0)),
    ("goi_field_density_workspace_bytes", (10, 64, 2, 1.0)), ("goi_field_iso_workspace_bytes", (0, 4, 4)),
    ("goi_mesh_components_workspace_bytes", (-1, 0)), ("goi_mesh_clean_workspace_bytes", (0, 1)),
    ("goi_mesh_decimate_workspace_bytes", (1, 0)), ("goi_mesh_normals_workspace_bytes", (0, 1 << 29)),
    ("goi_texture_rasterize_workspace_bytes", (-1, 8, 8)), ("goi_texture_grid_put_workspace_bytes", (1 << 28, 3, 8, 8)),
    ("goi_texture_fill_workspace_bytes", (0, 8)), ("goi_edit_bounds_workspace_bytes", (-1,)),
    ("goi_codebook_unique_rows_workspace_bytes", (0, 4, 8, 8)), ("goi_codebook_kmeans_workspace_bytes", (-1, 1, 1, 1)),
    ("goi_raster_photometric_workspace_bytes", (0, 3, 8, 8, 0)), ("goi_raster_densify_workspace_bytes", (1 << 30,)),
    ("goi_codebook_fused_workspace_bytes", (-1,)), ("goi_knn_workspace_bytes", (0,)), ("goi_knn_workspace_bytes", (1 << 30,)),
]


# ---- the rasterizer's direct-test and diagnostic entries, which live beside the kernels they drive (csrc/scan_sort.hip,
# reduce_rows.hip, preprocess_fwd.hip, preprocess_bwd.hip, blend_stats.hip, contrib.hip).  Per entry EVERY refusal it can reach
# before its first HIP call, in the order of its checks -- each row passes all earlier checks and fails exactly this one -- and
# every return of 0 that comes before a HIP call.  Recorded from the library as it was when these entries lived in csrc/api.hip.
A16 = C.c_void_p((1 << 20) + 4)  # 4-byte aligned, not 8 or 16
A2 = C.c_void_p((1 << 20) + 2)  # 2-byte aligned, not 4
_NAN = float("nan")

_SCENE = dict(P=4, D=3, M=16, S=16, W=16, H=16, bg=F, means3D=F, shs=F, colors_precomp=N, semantics=F, opacities=F, scales=F,
              scale_modifier=1.0, rotations=F, cov3D_precomp=N, viewmatrix=F, projmatrix=F, campos=F, tan_fovx=1.0, tan_fovy=1.0,
              prefiltered=0, debug=0)
# goi_raster_debug_preprocess_backward's arguments behind the scene, a call that passes every check (source 1: the records)
_PBWD = dict(source=1, flags=0, max_blocks=0, n_cap=8, frame=F, radii=F, clamped=F, cov3D=F, prev_radii=N, aux=F, tiles_touched=F,
             rows=F, row_flags=F, dL_dmean2D=F, dL_dconic=F, dL_dopacity=F, dL_dcolor=F, dL_dsemantic=F, dL_ddepth=F, dL_dmean3D=F,
             dL_dcov3D=F, dL_dsh=F, dL_dscale=F, dL_drot=F, workspace=F, stream=N)


def _pbwd(scene=None, **over):
    """The argument list of goi_raster_debug_preprocess_backward: the passing call with scene fields (`scene`: a dict, or "null")
    and arguments replaced."""
    from goi_hyperplane_amd import _lib
    assert set(over) <= set(_PBWD) and (scene == "null" or set(scene or {}) <= set(_SCENE))
    sc = N
    if scene != "null":
        fields = dict(_SCENE, **(scene or {}))
        sc = C.byref(_lib.GoiRasterScene(**{k: (v.value if isinstance(v, C.c_void_p) else v) for k, v in fields.items()}))
    return (sc,) + tuple(dict(_PBWD, **over).values())


_PB = "goi_raster_debug_preprocess_backward"
_NOSH = dict(shs=N, colors_precomp=F)
_SORT, _SCAN, _RED, _PAIR = ("goi_raster_debug_sort_pairs", "goi_raster_debug_exclusive_scan", "goi_raster_debug_reduce_rows",
                             "goi_raster_debug_pair_eval")
_RED_MSG = "goi_raster_debug_reduce_rows: "
_SH = "goi_raster_sh_grad_from_views"
_SH_MSG = "goi_raster_sh_grad_from_views: need 0 <= D <= 3 and (D+1)^2 <= M <= 16"

# entry, arguments (a tuple, or a function that makes one once the library is there), return value, message (None: no refusal)
RASTER = [
    (_SORT, (F, F, F, F, -1, 0, 32, N, N, 0, N, F, N), -1, _SORT + ": need 0 <= n < 2^30"),
    (_SORT, (F, F, F, F, 1 << 30, 0, 32, N, N, 0, N, F, N), -1, _SORT + ": need 0 <= n < 2^30"),
    (_SORT, (F, F, F, F, 8, -1, 32, N, N, 0, N, F, N), -1, _SORT + ": need 0 <= lo < hi <= 32"),
    (_SORT, (F, F, F, F, 8, 0, 33, N, N, 0, N, F, N), -1, _SORT + ": need 0 <= lo < hi <= 32"),
    (_SORT, (F, F, F, F, 8, 8, 8, N, N, 0, N, F, N), -1, _SORT + ": need 0 <= lo < hi <= 32"),
    (_SORT, (F, F, F, F, 8, 0, 32, N, N, 2, N, F, N), -1, _SORT + ": unknown flags"),
    (_SORT, (N, N, N, N, 0, 0, 32, F, F, 1, N, N, N), 0, None),  # n == 0: nothing to sort, nothing looked at
    (_SORT, (F, N, F, F, 8, 0, 32, N, N, 0, N, F, N), -1, _SORT + ": a required pointer is NULL"),
    (_SORT, (F, F, F, N, 8, 0, 32, N, N, 0, N, F, N), -1, _SORT + ": a required pointer is NULL"),
    (_SCAN, (F, N, F, -1, N, N, F, N), -1, _SCAN + ": need 0 <= n < 2^32"),
    (_SCAN, (F, N, F, 1 << 32, N, N, F, N), -1, _SCAN + ": need 0 <= n < 2^32"),
    (_SCAN, (F, F, F, 8, N, N, F, N), -1, _SCAN + ": out == in with a gather is a data race"),
    (_SCAN, (N, N, F, 8, N, N, F, N), -1, _SCAN + ": a required pointer is NULL"),
    (_SCAN, (F, N, N, 8, N, N, F, N), -1, _SCAN + ": a required pointer is NULL"),
    (_SCAN, (F, N, A16, 8, N, N, N, N), -1, _SCAN + ": a required pointer is NULL"),  # (its workspace: a NULL check only)
    ("goi_raster_debug_reduce_row_floats", (-1, 16), -1, _RED_MSG + "unknown mode"),
    ("goi_raster_debug_reduce_row_floats", (4, 16), -1, _RED_MSG + "unknown mode"),
    ("goi_raster_debug_reduce_row_floats", (0, 0), -1, _RED_MSG + "need 1 <= S <= 32"),
    ("goi_raster_debug_reduce_row_floats", (3, 33), -1, _RED_MSG + "need 1 <= S <= 32"),
    ("goi_raster_debug_reduce_row_floats", (2, 4), -1, _RED_MSG + "mode 2 sums 128-byte rows only (S = 5 .. 20)"),
    ("goi_raster_debug_reduce_row_floats", (2, 21), -1, _RED_MSG + "mode 2 sums 128-byte rows only (S = 5 .. 20)"),
    ("goi_raster_debug_reduce_row_floats", (0, 4), 16, None),
    ("goi_raster_debug_reduce_row_floats", (1, 16), 32, None),
    ("goi_raster_debug_reduce_row_floats", (2, 20), 32, None),
    ("goi_raster_debug_reduce_row_floats", (0, 32), 48, None),
    ("goi_raster_debug_reduce_row_floats", (3, 16), 16, None),
    ("goi_raster_debug_reduce_row_floats", (3, 17), 32, None),
    (_RED, (4, 4, 16, 8) + (F,) * 13 + (N,), -1, _RED_MSG + "unknown mode"),
    (_RED, (0, 4, 0, 8) + (F,) * 13 + (N,), -1, _RED_MSG + "need 1 <= S <= 32"),
    (_RED, (2, 4, 4, 8) + (F,) * 13 + (N,), -1, _RED_MSG + "mode 2 sums 128-byte rows only (S = 5 .. 20)"),
    (_RED, (0, -1, 16, 8) + (F,) * 13 + (N,), -1, _RED_MSG + "need P >= 0 and 0 <= n_cap < 2^31"),
    (_RED, (0, 4, 16, -1) + (F,) * 13 + (N,), -1, _RED_MSG + "need P >= 0 and 0 <= n_cap < 2^31"),
    (_RED, (0, 4, 16, 1 << 31) + (F,) * 13 + (N,), -1, _RED_MSG + "need P >= 0 and 0 <= n_cap < 2^31"),
    (_RED, (1, 0, 16, 8) + (N,) * 14, 0, None),  # P == 0: nothing to sum, nothing looked at
    (_RED, (1, 4, 16, 8, N) + (F,) * 12 + (N,), -1, _RED_MSG + "a required pointer is NULL"),  # frame
    (_RED, (1, 4, 16, 8, F, F, F, N, F, N, N, N, N, N, N, N, F, N), -1, _RED_MSG + "a required pointer is NULL"),  # flags
    (_RED, (0, 4, 16, 8, F, F, F, N) + (F,) * 9 + (N,), -1, _RED_MSG + "a required pointer is NULL"),  # mode 0: tiles_touched
    (_RED, (0, 4, 16, 8, F, F, F, F, F, F, N) + (F,) * 6 + (N,), -1, _RED_MSG + "a required pointer is NULL"),  # mode 0: dL_dmean2D
    (_RED, (0, 4, 16, 8, F, F, F, F, F, F, F, F, F, F, F, N, F, N), -1, _RED_MSG + "a required pointer is NULL"),  # mode 0: dL_ddepth
    (_RED, (3, 4, 16, 8, F, F, F, F, F, F, N, N, N, N, N, N, F, N), -1, _RED_MSG + "a required pointer is NULL"),  # mode 3: dL_dsemantic
    (_PB, lambda: _pbwd("null"), -1, _PB + ": scene is NULL"),
    (_PB, lambda: _pbwd(dict(P=-1)), -1, _PB + ": bad P/W/H"),
    (_PB, lambda: _pbwd(dict(W=0)), -1, _PB + ": bad P/W/H"),
    (_PB, lambda: _pbwd(dict(H=0)), -1, _PB + ": bad P/W/H"),
    (_PB, lambda: _pbwd(dict(S=0)), -1, _PB + ": need 1 <= S <= 32"),
    (_PB, lambda: _pbwd(dict(S=33)), -1, _PB + ": need 1 <= S <= 32"),
    (_PB, lambda: _pbwd(source=-1), -1, _PB + ": unknown source (0 per-id arrays, 1 records, 2 rows summed in the kernel)"),
    (_PB, lambda: _pbwd(source=3), -1, _PB + ": unknown source (0 per-id arrays, 1 records, 2 rows summed in the kernel)"),
    (_PB, lambda: _pbwd(flags=2), -1, _PB + ": unknown flag bits"),
    (_PB, lambda: _pbwd(max_blocks=-1), -1, _PB + ": max_blocks must be >= 0 (0: the product's grid)"),
    (_PB, lambda: _pbwd(n_cap=-1), -1, _PB + ": need 0 <= n_cap < 2^31"),
    (_PB, lambda: _pbwd(n_cap=1 << 31), -1, _PB + ": need 0 <= n_cap < 2^31"),
    (_PB, lambda: _pbwd(dict(S=4), source=2), -1, _PB + ": source 2 sums 128-byte rows only (S = 5 .. 20)"),
    (_PB, lambda: _pbwd(dict(S=21), source=2), -1, _PB + ": source 2 sums 128-byte rows only (S = 5 .. 20)"),
    # P == 0: nothing to do, whatever else the scene and the arguments hold
    (_PB, lambda: _pbwd(dict(P=0, tan_fovx=0.0, means3D=N), frame=N, workspace=N), 0, None),
    (_PB, lambda: _pbwd(dict(tan_fovx=0.0)), -1, _PB + ": tan_fovx / tan_fovy must be positive"),
    (_PB, lambda: _pbwd(dict(tan_fovy=-1.0)), -1, _PB + ": tan_fovx / tan_fovy must be positive"),
    (_PB, lambda: _pbwd(dict(tan_fovx=_NAN)), -1, _PB + ": tan_fovx / tan_fovy must be positive"),
    (_PB, lambda: _pbwd(dict(means3D=N)), -1, _PB + ": a required scene pointer is NULL"),
    (_PB, lambda: _pbwd(dict(viewmatrix=N)), -1, _PB + ": a required scene pointer is NULL"),
    (_PB, lambda: _pbwd(dict(projmatrix=N)), -1, _PB + ": a required scene pointer is NULL"),
    (_PB, lambda: _pbwd(dict(campos=N)), -1, _PB + ": a required scene pointer is NULL"),
    (_PB, lambda: _pbwd(dict(colors_precomp=F)), -1, _PB + ": shs and colors_precomp are both given"),
    (_PB, lambda: _pbwd(dict(D=-1)), -1, _PB + ": SH degree must be 0..3 and (D+1)^2 <= M <= 16"),
    (_PB, lambda: _pbwd(dict(D=4, M=25)), -1, _PB + ": SH degree must be 0..3 and (D+1)^2 <= M <= 16"),
    (_PB, lambda: _pbwd(dict(D=3, M=15)), -1, _PB + ": SH degree must be 0..3 and (D+1)^2 <= M <= 16"),
    (_PB, lambda: _pbwd(dict(D=0, M=17)), -1, _PB + ": SH degree must be 0..3 and (D+1)^2 <= M <= 16"),
    (_PB, lambda: _pbwd(dict(shs=A16)), -1, _PB + ": shs must be 16-byte aligned when 3 M is a multiple of 4"),
    (_PB, lambda: _pbwd(_NOSH), -1, _PB + ": dL_dsh without shs"),
    (_PB, lambda: _pbwd(dict(rotations=N)), -1, _PB + ": scales and rotations go together"),
    (_PB, lambda: _pbwd(dict(scales=N)), -1, _PB + ": scales and rotations go together"),
    (_PB, lambda: _pbwd(dict(cov3D_precomp=F)), -1, _PB + ": exactly one of the scale/rotation pair and cov3D_precomp"),
    (_PB, lambda: _pbwd(dict(scales=N, rotations=N)), -1, _PB + ": exactly one of the scale/rotation pair and cov3D_precomp"),
    (_PB, lambda: _pbwd(cov3D=N), -1, _PB + ": cov3D (what the forward computed from scale/rotation) is NULL"),
    (_PB, lambda: _pbwd(dict(rotations=A16)), -1, _PB + ": rotations must be 16-byte aligned"),
    (_PB, lambda: _pbwd(flags=1, source=0), -1, _PB + ": accumulate needs source 1 (the records)"),
    (_PB, lambda: _pbwd(flags=1, source=2), -1, _PB + ": accumulate needs source 1 (the records)"),
    (_PB, lambda: _pbwd(flags=1, prev_radii=F), -1, _PB + ": accumulate with prev_radii"),
    (_PB, lambda: _pbwd(flags=1, dL_dsh=N), -1, _PB + ": accumulate with factored SH (dL_dsh NULL)"),
    (_PB, lambda: _pbwd(frame=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(radii=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_dmean2D=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_dcolor=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_dmean3D=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_dcov3D=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_dscale=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(dL_drot=N), -1, _PB + ": a required pointer is NULL"),
    (_PB, lambda: _pbwd(clamped=N), -1, _PB + ": a required pointer is NULL"),  # (SH colours: the clamp bits)
    (_PB, lambda: _pbwd(source=0, dL_dconic=N), -1, _PB + ": source 0 reads dL_dconic and dL_ddepth"),
    (_PB, lambda: _pbwd(source=0, dL_ddepth=N), -1, _PB + ": source 0 reads dL_dconic and dL_ddepth"),
    (_PB, lambda: _pbwd(aux=N), -1, _PB + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic"),
    (_PB, lambda: _pbwd(tiles_touched=N), -1, _PB + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic"),
    (_PB, lambda: _pbwd(source=2, rows=N), -1, _PB + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic"),
    (_PB, lambda: _pbwd(dL_dopacity=N), -1, _PB + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic"),
    (_PB, lambda: _pbwd(source=2, dL_dsemantic=N), -1,
     _PB + ": sources 1 and 2 need aux, tiles_touched, rows, dL_dopacity and dL_dsemantic"),
    (_PB, lambda: _pbwd(source=2, row_flags=N), -1, _PB + ": source 2 needs the validity bytes"),
    # (what a source does not read may be NULL: the call gets as far as its workspace)
    (_PB, lambda: _pbwd(_NOSH, source=0, clamped=N, aux=N, tiles_touched=N, rows=N, row_flags=N, dL_dopacity=N, dL_dsemantic=N,
                        dL_dsh=N, workspace=N), -1, _PB + ": NULL workspace"),
    (_PB, lambda: _pbwd(dict(scales=N, rotations=N, cov3D_precomp=F), cov3D=N, row_flags=N, dL_dconic=N, dL_ddepth=N,
                        workspace=MIS), -1, _PB + ": workspace must be 256-byte aligned"),
    (_PB, lambda: _pbwd(dL_drot=A16), -1,
     _PB + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned"),
    (_PB, lambda: _pbwd(aux=A16), -1,
     _PB + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned"),
    (_PB, lambda: _pbwd(rows=A16), -1,
     _PB + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned"),
    (_PB, lambda: _pbwd(source=2, row_flags=A2), -1,
     _PB + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned"),
    (_PB, lambda: _pbwd(dL_dsemantic=A16), -1,
     _PB + ": dL_drot, aux, rows and dL_dsemantic must be 16-byte aligned, the validity bytes 4-byte aligned"),
    (_SH, (0, 3, 16, 2, N, N, N, N, N), 0, None),  # P <= 0 or V <= 0: nothing to add, nothing looked at
    (_SH, (-1, 9, 0, 2, N, N, N, N, N), 0, None),
    (_SH, (4, 3, 16, 0, N, N, N, N, N), 0, None),
    (_SH, (4, -1, 16, 2, F, F, F, F, N), -1, _SH_MSG),
    (_SH, (4, 4, 25, 2, F, F, F, F, N), -1, _SH_MSG),
    (_SH, (4, 2, 8, 2, F, F, F, F, N), -1, _SH_MSG),
    (_SH, (4, 0, 17, 2, F, F, F, F, N), -1, _SH_MSG),
    (_SH, (4, 3, 16, 2, N, F, F, F, N), -1, _SH + ": NULL pointer"),
    (_SH, (4, 3, 16, 2, F, N, F, F, N), -1, _SH + ": NULL pointer"),
    (_SH, (4, 3, 16, 2, F, F, N, F, N), -1, _SH + ": NULL pointer"),
    (_SH, (4, 3, 16, 2, F, F, F, N, N), -1, _SH + ": NULL pointer"),
    ("goi_raster_mark_visible", (-1, F, F, F, F, N), -1, "bad P"),
    ("goi_raster_mark_visible", (0, N, N, N, N, N), 0, None),  # P == 0
    ("goi_raster_mark_visible", (4, N, F, N, F, N), -1, "NULL pointer"),
    ("goi_raster_mark_visible", (4, F, N, N, F, N), -1, "NULL pointer"),
    ("goi_raster_mark_visible", (4, F, F, N, N, N), -1, "NULL pointer"),
    (_PAIR, (0, 16, 16, F, F, 8, F, F, F, N), -1, _PAIR + ": bad P/W/H"),
    (_PAIR, (4, 0, 16, F, F, 8, F, F, F, N), -1, _PAIR + ": bad P/W/H"),
    (_PAIR, (4, 16, -1, F, F, 8, F, F, F, N), -1, _PAIR + ": bad P/W/H"),
    (_PAIR, (4, 16, 16, F, F, -1, F, F, F, N), -1, _PAIR + ": need 0 <= n_requests <= 2^31"),
    (_PAIR, (4, 16, 16, F, F, (1 << 31) + 1, F, F, F, N), -1, _PAIR + ": need 0 <= n_requests <= 2^31"),
    (_PAIR, (4, 16, 16, N, N, 0, N, N, N, N), 0, None),  # no requests: nothing looked at
    (_PAIR, (4, 16, 16, F, N, 8, F, F, F, N), -1, _PAIR + ": a required pointer is NULL"),
    (_PAIR, (4, 16, 16, F, F, 8, N, F, F, N), -1, _PAIR + ": a required pointer is NULL"),
    (_PAIR, (4, 16, 16, F, F, 8, F, N, F, N), -1, _PAIR + ": a required pointer is NULL"),
    (_PAIR, (4, 16, 16, F, F, 8, F, F, N, N), -1, _PAIR + ": a required pointer is NULL"),
    (_PAIR, (4, 16, 16, F, A16, 8, F, F, F, N), -1, _PAIR + ": requests must be 8-byte aligned"),
    (_PAIR, (4, 16, 16, F, F, 8, A2, F, F, N), -1, _PAIR + ": E and alpha must be 4-byte aligned"),
    (_PAIR, (4, 16, 16, F, F, 8, F, A2, F, N), -1, _PAIR + ": E and alpha must be 4-byte aligned"),
    ("goi_raster_blend_stats", (0, 16, 16, 8, F, F, F, F, N), -1, "goi_raster_blend_stats: bad P/W/H/R"),
    ("goi_raster_blend_stats", (4, 0, 16, 8, F, F, F, F, N), -1, "goi_raster_blend_stats: bad P/W/H/R"),
    ("goi_raster_blend_stats", (4, 16, 0, 8, F, F, F, F, N), -1, "goi_raster_blend_stats: bad P/W/H/R"),
    ("goi_raster_blend_stats", (4, 16, 16, -1, F, F, F, F, N), -1, "goi_raster_blend_stats: bad P/W/H/R"),
    ("goi_raster_blend_stats", (4, 16, 16, 8, N, F, F, F, N), -1, "workspace pointer is NULL"),
    ("goi_raster_blend_stats", (4, 16, 16, 8, F, N, F, F, N), -1, "workspace pointer is NULL"),
    ("goi_raster_blend_stats", (4, 16, 16, 0, F, N, N, F, N), -1, "workspace pointer is NULL"),
    ("goi_raster_blend_stats", (4, 16, 16, 8, F, F, F, N, N), -1, "workspace pointer is NULL"),  # (the counters)
    ("goi_raster_contrib_frame", (0, 16, 16, 8, F, F, F, F, F, F, N), -1, "goi_raster_contrib_frame: bad P/W/H/R"),
    ("goi_raster_contrib_frame", (4, 16, 16, -1, F, F, F, F, F, F, N), -1, "goi_raster_contrib_frame: bad P/W/H/R"),
    ("goi_raster_contrib_frame", (4, 16, 16, 8, N, F, F, F, F, F, N), -1, "goi_raster_contrib_frame: workspace pointer is NULL"),
    ("goi_raster_contrib_frame", (4, 16, 16, 8, F, N, F, F, F, F, N), -1, "goi_raster_contrib_frame: workspace pointer is NULL"),
    ("goi_raster_contrib_frame", (4, 16, 16, 0, F, N, N, F, F, F, N), -1, "goi_raster_contrib_frame: workspace pointer is NULL"),
    ("goi_raster_contrib_frame", (4, 16, 16, 8, F, F, F, N, N, N, N), -1,
     "goi_raster_contrib_frame: peak, top_id and top_w are all NULL"),
]

# the same entries' workspaces, through check_workspace (goi_raster_debug_preprocess_backward: RASTER, between its pointer checks)
WORKSPACE += [
    (_SORT, (F, F, F, F, 8, 0, 32, N, N, 0, N, WS, N), _SORT + ": NULL workspace", _SORT + ": workspace must be 256-byte aligned"),
    (_RED, (1, 4, 16, 8, F, F, F, N, F, F, N, N, N, N, N, N, WS, N),
     _RED_MSG + "NULL workspace", _RED_MSG + "workspace must be 256-byte aligned"),
    (_PAIR, (4, 16, 16, WS, F, 8, F, F, F, N), _PAIR + ": NULL geom_buffer", _PAIR + ": geom_buffer must be 256-byte aligned"),
]

# their size functions: 0 for an argument out of range
RASTER_SIZES = [
    ("goi_raster_debug_sort_workspace_bytes", (-1, 0, 32)), ("goi_raster_debug_sort_workspace_bytes", (1 << 30, 0, 32)),
    ("goi_raster_debug_sort_workspace_bytes", (8, -1, 32)), ("goi_raster_debug_sort_workspace_bytes", (8, 0, 33)),
    ("goi_raster_debug_sort_workspace_bytes", (8, 8, 8)), ("goi_raster_debug_scan_workspace_bytes", (-1,)),
    ("goi_raster_debug_scan_workspace_bytes", (1 << 32,)), ("goi_raster_debug_reduce_workspace_bytes", (-1,)),
    ("goi_raster_debug_reduce_workspace_bytes", (1 << 31,)),
]


# ---- the entries of the rasterizer's frame (csrc/api.hip).  Per entry every path that returns before its first HIP call, in the
# order of its checks: each row passes all earlier checks and fails exactly this one.  (A forward or a trace over P == 0 Gaussians
# clears its outputs on the stream: not such a path.)  Each entry's arguments are a passing call with fields replaced.
_FWD = dict(geom=F, image=F, alloc="alloc", user=N, color=F, sem=F, depth=F, alpha=F, radii=F, keep=N, invert=0, stream=N)
_ASYNC = dict(geom=F, image=F, binning=F, capacity=64, color=F, sem=F, depth=F, alpha=F, radii=F, zcut_in=N, zcut_out=N, keep=N,
              invert=0, stream=N)
_REDO = dict(num_rendered=8, geom=F, image=F, binning=F, color=F, sem=F, depth=F, alpha=F, radii=F, stream=N)
_REBLEND = dict(R=8, geom=F, binning=F, cached_image=F, image=F, color=F, sem=F, depth=F, alpha=F, stream=N)
_TRACE = dict(img_sem=F, geom=F, image=F, alloc="alloc", user=N, color=F, gau_sem=F, num_gsem=F, radii=F, stream=N)
_BWD = dict(R=8, scratch_instances=0, flags=0, geom=F, binning=F, image=F, radii=F, out_alpha=F, dL_dout_color=F, dL_dout_semantic=F,
            dL_dout_depth=F, dL_dout_alpha=F, dL_dmean2D=F, dL_dconic=F, dL_dopacity=F, dL_dcolor=F, dL_dsemantic=F, dL_ddepth=F,
            dL_dmean3D=F, dL_dcov3D=F, dL_dsh=F, dL_dscale=F, dL_drot=F, scratch=F, prev_radii=N, prev_mask=N, row_mask=N, stream=N)
_BSEM = dict(R=8, geom=F, binning=F, image=F, radii=F, out_alpha=F, dL_dout_semantic=F, dL_dsemantic=F, scratch=F, stream=N)
_FRAME_ARGS = {"goi_raster_forward": _FWD, "goi_raster_forward_async": _ASYNC, "goi_raster_forward_redo": _REDO,
               "goi_raster_forward_reblend": _REBLEND, "goi_raster_trace": _TRACE, "goi_raster_backward": _BWD,
               "goi_raster_backward_semantics": _BSEM}


def _frame(fn, message, scene=None, rc=-1, **over):
    """A FRAME row: entry `fn` called with its passing arguments, scene fields (`scene`: a dict, or "null") and arguments replaced."""
    base = _FRAME_ARGS[fn]
    assert set(over) <= set(base) and (scene == "null" or set(scene or {}) <= set(_SCENE))

    def args():
        from goi_hyperplane_amd import _lib
        sc = N
        if scene != "null":
            fields = dict(_SCENE, **(scene or {}))
            sc = C.byref(_lib.GoiRasterScene(**{k: (v.value if isinstance(v, C.c_void_p) else v) for k, v in fields.items()}))
        return (sc,) + tuple(dict(base, **over).values())
    return (fn, args, rc, message)


_SH_MSG2 = "Please provide excatly one of either SHs or precomputed colors!"
_COV_MSG = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
_DEG_MSG = "SH degree must be 0..3 and (D+1)^2 <= M <= 16"


def _validate_rows(fn, need_sem=True, need_opacity=True):
    """The refusals of validate() (csrc/api.hip), which every entry that takes a whole scene starts with, through `fn`."""
    rows = [_frame(fn, "scene is NULL", "null")]
    rows += [_frame(fn, "bad P/W/H", dict([f])) for f in (("P", -1), ("W", 0), ("H", 0), ("W", -1))]
    rows += [_frame(fn, "semantic channels S must be in 1..32", dict(S=v)) for v in (0, 33)]
    if need_opacity:
        rows += [_frame(fn, "opacities is NULL", dict(opacities=N))]
    rows += [_frame(fn, "a required input pointer is NULL", {f: N}) for f in ("means3D", "viewmatrix", "projmatrix", "campos", "bg")]
    if need_sem:
        rows += [_frame(fn, "semantics is required (the reference dereferences it unconditionally)", dict(semantics=N))]
    rows += [_frame(fn, "semantics must be 16-byte aligned when S is a multiple of 4 (its rows are moved as 16-byte words)",
                    dict(semantics=A16, S=v)) for v in (16, 4)]
    rows += [_frame(fn, _SH_MSG2, dict(colors_precomp=F)), _frame(fn, _SH_MSG2, dict(shs=N))]
    rows += [_frame(fn, "shs must be 16-byte aligned when 3 M is a multiple of 4 (its rows are moved as 16-byte words)",
                    dict(shs=A16, **m)) for m in (dict(M=16), dict(D=1, M=4))]
    rows += [_frame(fn, _COV_MSG, sc) for sc in (dict(scales=N), dict(rotations=N), dict(scales=N, rotations=N), dict(cov3D_precomp=F),
                                                 dict(scales=N, cov3D_precomp=F))]
    rows += [_frame(fn, _DEG_MSG, sc) for sc in (dict(D=-1), dict(D=4, M=25), dict(D=3, M=15), dict(D=0, M=17))]
    return rows


_FA, _RD, _RB = "goi_raster_forward_async", "goi_raster_forward_redo", "goi_raster_forward_reblend"
_BW, _BS = "goi_raster_backward", "goi_raster_backward_semantics"
_ACC_MSG = ("GOI_BACKWARD_ACCUMULATE needs the default backward (scratch given, bwd_variant 0 / 2, bwd_records 1), dL_dsh when "
            "the colours are SH, prev_radii NULL and debug off")
_P0 = dict(P=0, means3D=N, opacities=N, shs=N, scales=N)  # (P == 0: nothing else of the scene is looked at)

# entry, arguments (a function that makes them once the library is there), return value, message (None: no refusal)
FRAME = (
    _validate_rows("goi_raster_forward")
    + [_frame("goi_raster_forward", "workspace pointer / allocator is NULL", **kw)
       for kw in (dict(geom=N), dict(image=N), dict(alloc="no alloc"))]
    + _validate_rows(_FA)
    + [_frame(_FA, _FA + ": P == 0 has nothing to speculate on; use goi_raster_forward", _P0),
       _frame(_FA, _FA + ": debug mode synchronises after every stage; use goi_raster_forward", dict(debug=1)),
       _frame(_FA, _FA + ": capacity must be positive", capacity=0),
       _frame(_FA, _FA + ": capacity must be positive", capacity=-1)]
    + [_frame(_FA, "workspace pointer is NULL", **{k: N}) for k in ("geom", "image", "binning")]
    + [_frame(_FA, _FA + ": a selection (keep) cannot be combined with a depth cut", keep=F, **z)
       for z in (dict(zcut_in=F), dict(zcut_out=F), dict(zcut_in=F, zcut_out=F))]
    + [("goi_raster_ticket_result", (t, w, N, N), -1, "invalid or already resolved ticket")
       for t, w in ((-1, 0), (-1, 1), (0, 0), (4095, 1), (1 << 20, 0))]  # (no ticket was ever issued in this process)
    + [_frame(_RD, "scene is NULL", "null")]
    + [_frame(_RD, _RD + ": bad P/W/H/S", dict([f])) for f in (("P", 0), ("P", -1), ("W", 0), ("H", 0), ("S", 0), ("S", 33))]
    + [_frame(_RD, _RD + ": semantics, bg and radii are required", dict(semantics=N)),
       _frame(_RD, _RD + ": semantics, bg and radii are required", dict(bg=N)),
       _frame(_RD, _RD + ": semantics, bg and radii are required", radii=N),
       _frame(_RD, _RD + ": nothing to redo", num_rendered=-1),
       _frame(_RD, "workspace pointer is NULL", geom=N),
       _frame(_RD, "workspace pointer is NULL", image=N),
       _frame(_RD, "workspace pointer is NULL", binning=N),
       _frame(_RD, "workspace pointer is NULL", num_rendered=0, binning=N, image=N)]
    + [_frame(_RB, "scene is NULL", "null")]
    + [_frame(_RB, _RB + ": bad P/W/H/S", dict([f])) for f in (("P", 0), ("P", -1), ("W", 0), ("H", 0), ("S", 0), ("S", 33))]
    + [_frame(_RB, _RB + ": semantics and bg are required", dict(semantics=N)),
       _frame(_RB, _RB + ": semantics and bg are required", dict(bg=N)),
       _frame(_RB, _RB + ": bad R", R=-1)]
    + [_frame(_RB, "workspace pointer is NULL", **{k: N}) for k in ("geom", "cached_image", "image", "binning")]
    + [_frame(_RB, "workspace pointer is NULL", R=0, binning=N, geom=N)]
    + [_frame(_RB, "output pointer is NULL", **{k: N}) for k in ("color", "sem", "depth", "alpha")]
    + [_frame(_RB, "output pointer is NULL", R=0, binning=N, alpha=N)]  # (R == 0 needs no binning workspace)
    + _validate_rows(_BW, need_opacity=False)
    + [_frame(_BW, None, _P0, rc=0, geom=N, image=N, binning=N, scratch=N),  # P == 0: nothing to do, nothing looked at
       # (the forward's records hold the opacities: a scene without them gets as far as the workspaces)
       _frame(_BW, "workspace pointer is NULL", dict(opacities=N), geom=N),
       _frame(_BW, "workspace pointer is NULL", image=N),
       _frame(_BW, "workspace pointer is NULL", binning=N),
       _frame(_BW, "workspace pointer is NULL", R=0, binning=N, image=N),
       _frame(_BW, "scratch_instances must be in 0..R (0: the scratch is laid out for R)", scratch_instances=-1),
       _frame(_BW, "scratch_instances must be in 0..R (0: the scratch is laid out for R)", scratch_instances=9),
       _frame(_BW, "scratch_instances must be in 0..R (0: the scratch is laid out for R)", R=0, binning=N, scratch_instances=1),
       _frame(_BW, _ACC_MSG, flags=1, scratch=N),
       _frame(_BW, _ACC_MSG, flags=1, prev_radii=F),
       _frame(_BW, _ACC_MSG, flags=1, dL_dsh=N),
       _frame(_BW, _ACC_MSG, dict(debug=1), flags=1),
       _frame(_BW, "GOI_BACKWARD_ACCUMULATE: prev_mask and row_mask must be NULL", flags=1, prev_mask=F),
       _frame(_BW, "GOI_BACKWARD_ACCUMULATE: prev_mask and row_mask must be NULL", flags=1, row_mask=F),
       _frame(_BW, "GOI_BACKWARD_ACCUMULATE: prev_mask and row_mask must be NULL", flags=1, scratch_instances=8, prev_mask=F,
              row_mask=F)]
    + _validate_rows(_BS, need_opacity=False)
    + [_frame(_BS, None, _P0, rc=0, geom=N, image=N, binning=N, scratch=N),
       _frame(_BS, "workspace pointer is NULL", dict(opacities=N), geom=N),
       _frame(_BS, "workspace pointer is NULL", image=N),
       _frame(_BS, "workspace pointer is NULL", binning=N),
       _frame(_BS, _BS + " needs the scratch of goi_raster_backward_scratch_bytes", scratch=N),
       _frame(_BS, _BS + " needs the scratch of goi_raster_backward_scratch_bytes", R=0, binning=N, scratch=N)]
    + [_frame(_BS, "a required pointer is NULL", **{k: N}) for k in ("dL_dout_semantic", "dL_dsemantic", "out_alpha", "radii")]
    + _validate_rows("goi_raster_trace", need_sem=False)
    + [("goi_raster_truncated_flag", a, None, None) for a in ((N, 4), (F, 0), (F, -1), (N, 0))]
)


def _ids(table):
    seen = {}
    out = []
    for row in table:
        seen[row[0]] = seen.get(row[0], 0) + 1
        out.append(row[0] if seen[row[0]] == 1 else f"{row[0]}-{seen[row[0]]}")
    return out


@pytest.mark.parametrize("fn,args,message", FIRST, ids=_ids(FIRST))
def test_first_refusal(lib, fn, args, message):
    assert _call(lib, fn, args) < 0
    assert _err(lib) == message


@pytest.mark.parametrize("fn,args,null_message,misaligned_message", WORKSPACE, ids=_ids(WORKSPACE))
def test_workspace_refusals(lib, fn, args, null_message, misaligned_message):
    assert _call(lib, fn, args, ws=None) < 0
    assert _err(lib) == null_message
    assert _call(lib, fn, args, ws=MIS) < 0
    assert _err(lib) == misaligned_message


@pytest.mark.parametrize("fn,args", SIZES, ids=_ids(SIZES))
def test_size_out_of_range_is_zero(lib, fn, args):
    assert getattr(lib, fn)(*args) == 0


@pytest.mark.parametrize("fn,args,rc,message", RASTER, ids=_ids(RASTER))
def test_raster_entry_refusals_and_early_returns(lib, fn, args, rc, message):
    assert lib.goi_knn_dist2(-1, F, F, F, N) < 0  # (a message of another unit's: a return of 0 must leave it alone)
    assert _call(lib, fn, args() if callable(args) else args) == rc
    assert _err(lib) == (message if message is not None else "goi_knn_dist2: bad P")


@pytest.mark.parametrize("fn,args", RASTER_SIZES, ids=_ids(RASTER_SIZES))
def test_raster_size_out_of_range_is_zero(lib, fn, args):
    assert getattr(lib, fn)(*args) == 0


@pytest.mark.parametrize("fn,args,rc,message", FRAME, ids=_ids(FRAME))
def test_frame_entry_refusals_and_early_returns(lib, fn, args, rc, message):
    assert lib.goi_knn_dist2(-1, F, F, F, N) < 0  # (a message of another unit's: a return without a refusal must leave it alone)
    assert _call(lib, fn, args() if callable(args) else args) == rc
    assert _err(lib) == (message if message is not None else "goi_knn_dist2: bad P")


def test_async_forward_refuses_without_the_onesweep_sort(lib):
    """The speculative forward takes its counts on the device, which only the onesweep sort does: with sort_variant 0 it is
    refused, behind the debug check and before it looks at the capacity or the workspaces."""
    fn, args, _rc, _message = _frame(_FA, None, capacity=0, geom=N)
    assert lib.goi_raster_set_option(b"sort_variant", 0) == 0
    try:
        assert _call(lib, fn, args()) == -1
        assert _err(lib) == "goi_raster_forward_async needs the onesweep sort (sort_variant 1)"
    finally:
        assert lib.goi_raster_set_option(b"sort_variant", 1) == 0
    assert _call(lib, fn, args()) == -1
    assert _err(lib) == _FA + ": capacity must be positive"


def test_sort_entry_refuses_device_counts_without_the_onesweep_sort(lib):
    """n_dev and ghist belong to the onesweep sort: with sort_variant 0 the entry refuses them, behind its flags check and
    before it looks at n, the pointers or the workspace."""
    message = _SORT + ": n_dev and ghist need the onesweep sort (sort_variant 1)"
    assert lib.goi_raster_set_option(b"sort_variant", 0) == 0
    try:
        for n_dev, ghist in ((F, N), (N, F)):
            assert lib.goi_raster_debug_sort_pairs(N, N, N, N, 0, 0, 32, n_dev, ghist, 0, N, N, N) < 0
            assert _err(lib) == message
        assert lib.goi_raster_debug_sort_pairs(N, N, N, N, 0, 0, 32, N, N, 0, N, N, N) == 0
    finally:
        assert lib.goi_raster_set_option(b"sort_variant", 1) == 0


def test_every_raster_test_entry_is_covered():
    from goi_hyperplane_amd import _lib
    beside_kernels = {n for n in _lib.SYMBOLS if n.startswith(("goi_raster_debug_sort_", "goi_raster_debug_scan_",
                                                                "goi_raster_debug_exclusive_scan", "goi_raster_debug_reduce_",
                                                                "goi_raster_debug_preprocess_", "goi_raster_debug_pair_"))}
    beside_kernels |= {"goi_raster_blend_stats", "goi_raster_contrib_frame", "goi_raster_mark_visible",
                       "goi_raster_sh_grad_from_views"}
    assert len(beside_kernels) == 13
    assert beside_kernels == {row[0] for row in RASTER + RASTER_SIZES}
    assert {n for n in beside_kernels if n.endswith("_bytes")} == {row[0] for row in RASTER_SIZES}


def test_every_frame_entry_is_covered():
    from goi_hyperplane_amd import _lib
    frame = {n for n in _lib.SYMBOLS if n.startswith(("goi_raster_forward", "goi_raster_backward", "goi_raster_ticket_",
                                                       "goi_raster_trace", "goi_raster_truncated_"))}
    frame -= {"goi_raster_backward_scratch_bytes"}  # (a size function: any int has an answer)
    assert len(frame) == 9
    assert frame == {row[0] for row in FRAME}


def test_every_moved_entry_is_covered():
    from goi_hyperplane_amd import _lib
    families = ("goi_semantic_", "goi_field_", "goi_mesh_", "goi_texture_", "goi_edit_", "goi_codebook_", "goi_adam_",
                "goi_knn_", "goi_raster_photometric_", "goi_raster_densify_")
    moved = {n for table in _lib.SYMBOL_TABLES for n in table if n.startswith(families)}
    # (no arguments, nothing to refuse)
    moved -= {"goi_codebook_loss_partial_rows", "goi_codebook_sim_workspace_bytes", "goi_codebook_dlut_partial_blocks",
              "goi_codebook_fused_partial_rows"}
    assert moved == {row[0] for row in FIRST + SIZES}
    assert {n for n in moved if n.endswith("_bytes")} == {row[0] for row in SIZES}


def test_effects_before_a_refusal_keep_their_place(lib):
    """goi_codebook_unique_rows writes *flags = 0 once its sizes and pointers are accepted, before it looks at the workspace;
    a refusal of the sizes leaves *flags alone."""
    _FLAGS.value = 7
    assert _call(lib, "goi_codebook_unique_rows", (_MAPS, -1, 4, 8, 8, _COUNTS, C.byref(_FLAGS), "alloc", N, F, N)) < 0
    assert _FLAGS.value == 7
    assert _call(lib, "goi_codebook_unique_rows", _UNIQ + (N, N)) < 0
    assert _FLAGS.value == 0


def test_last_error_is_per_thread(lib):
    """Entries of two different units refuse on two threads: each thread reads its own message, and the second thread's refusal
    does not change what the first one reads."""
    assert lib.goi_knn_dist2(-1, F, F, F, N) < 0
    assert _err(lib) == "goi_knn_dist2: bad P"
    seen = {}

    def other():
        seen["before"] = _err(lib)
        seen["rc"] = lib.goi_mesh_normals(-1, 4, F, F, F, F, F, N)
        seen["after"] = _err(lib)

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"before": "", "rc": -1, "after": "goi_mesh_normals: need 0 <= V, F and V, 3 F < 2^30"}
    assert _err(lib) == "goi_knn_dist2: bad P"
