"""What the C entries of the stand-alone families refuse before they touch the device, without a GPU: each family's unit
(csrc/mesh.hip, csrc/pca.hip, ...) defines its own extern "C" entries, and every refusal ends in the one thread_local message of
csrc/api.hip that goi_raster_last_error returns.  Per entry: the message of its first refusal; where it takes a workspace, the
messages for a NULL and for a misaligned one; per size function, the 0 it returns for an argument out of range.  The strings
were recorded from the library as it was when every one of these entries still lived in csrc/api.hip.
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
_ALLOC = None  # made with the library's callback type in the fixture


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    global _ALLOC
    _ALLOC = _lib.ALLOC_FN(lambda user, nbytes: None)
    return _lib.load()


def _call(lib, fn, args, ws=None):
    args = tuple(ws if a is WS else _ALLOC if a == "alloc" else a for a in args)
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
