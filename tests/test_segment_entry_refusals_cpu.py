"""What the C entries of csrc/segment.hip (goi_knn_segment_edges, goi_knn_segment_components) declare, export and refuse before any
device call: beside tests/test_entry_refusals_cpu.py, which records the entries that were there before."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 4)  # 4-byte aligned only
ODD = C.c_void_p((1 << 20) + 2)
N = None
NAN, INF = float("nan"), float("inf")
NAMES = ("goi_knn_segment_edges", "goi_knn_segment_components_workspace_bytes", "goi_knn_segment_components")
MUTUAL, MAX_DIST2 = 1, 2


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_listed_as_later_additions(lib):
    from goi_hyperplane_amd import _lib, segment
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    assert set(_lib.SEGMENT_SYMBOLS) == set(NAMES)
    assert _lib.SEGMENT_SYMBOLS in _lib.LATER_TABLES and _lib.SEGMENT_SYMBOLS not in _lib.SYMBOL_TABLES
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in hdr.split("#define GOI_RASTER_ABI_VERSION")[0], f"{name} is not in the list of later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    for macro, value in (("GOI_SEGMENT_MUTUAL", segment.MUTUAL), ("GOI_SEGMENT_MAX_DIST2", segment.MAX_DIST2),
                         ("GOI_SEGMENT_STATUS_UNION", segment.STATUS_UNION)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value
    assert os.path.exists(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "segment.hip"))
    assert build_flags() == ["-ffp-contract=off"]


def build_flags():
    from goi_hyperplane_amd import build
    return build.UNITS["segment.hip"]


def test_workspace_size_is_monotone_in_P_and_a_multiple_of_256(lib):
    size = lib.goi_knn_segment_components_workspace_bytes
    for bad in ((-1, 3), (10, 0), (10, -1), (2 ** 30, 1), (2 ** 26, 16), (2 ** 29, 2)):
        assert size(*bad) == 0
    grid = [0, 1, 63, 64, 65, 255, 256, 257, 5000, 100_000, 1_000_000, 3_000_000]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(a, 8) <= size(b, 8)
    for P in grid:
        assert size(P, 8) % 256 == 0 and size(P, 1) == size(P, 16)  # the partition's workspace is per row, not per edge
    assert size(2 ** 30 - 1, 1) > 0
    assert size(1_000_000, 8) < 1_000_000 * 20  # parents, sizes, ranks and the scan's scratch: below 20 bytes per row


#         P  S  k  idx f  tau dist2 max_dist2 flags labels rows join stream
EDGES = [
    ((-1, 4, 3, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: bad P"),
    ((10, 4, 0, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need k >= 1"),
    ((10, 4, -2, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need k >= 1"),
    ((2 ** 30, 4, 1, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need P * k < 2^30"),
    ((2 ** 26, 4, 16, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need P * k < 2^30"),
    ((10, 0, 3, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need 1 <= S <= 32"),
    ((10, 33, 3, F, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: need 1 <= S <= 32"),
    ((10, 4, 3, F, F, NAN, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: tau is NaN"),
    ((10, 4, 3, F, N, NAN, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: tau is NaN"),
    ((10, 4, 3, F, F, 1.0, N, 0.0, 4, N, N, F, N), "goi_knn_segment_edges: unknown flags"),
    ((10, 4, 3, F, F, 1.0, N, 1.0, MAX_DIST2, N, N, F, N), "goi_knn_segment_edges: max_dist2 needs dist2"),
    ((10, 4, 3, F, F, 1.0, N, 1.0, MAX_DIST2 | MUTUAL, N, N, F, N), "goi_knn_segment_edges: max_dist2 needs dist2"),
    ((10, 4, 3, F, F, 1.0, F, NAN, MAX_DIST2, N, N, F, N), "goi_knn_segment_edges: max_dist2 is NaN"),
    ((10, 4, 3, N, F, 1.0, N, 0.0, 0, N, N, F, N), "goi_knn_segment_edges: a required pointer is NULL"),
    ((10, 4, 3, F, F, 1.0, N, 0.0, 0, N, N, N, N), "goi_knn_segment_edges: a required pointer is NULL"),
    ((10, 4, 3, ODD, F, 1.0, N, 0.0, 0, N, N, F, N),
     "goi_knn_segment_edges: idx, features and dist2 must be 4-byte aligned, labels 8-byte aligned"),
    ((10, 4, 3, F, ODD, 1.0, N, 0.0, 0, N, N, F, N),
     "goi_knn_segment_edges: idx, features and dist2 must be 4-byte aligned, labels 8-byte aligned"),
    ((10, 4, 3, F, F, 1.0, ODD, 0.0, 0, N, N, F, N),
     "goi_knn_segment_edges: idx, features and dist2 must be 4-byte aligned, labels 8-byte aligned"),
    ((10, 4, 3, F, F, 1.0, N, 0.0, 0, MIS, N, F, N),
     "goi_knn_segment_edges: idx, features and dist2 must be 4-byte aligned, labels 8-byte aligned"),
]
#              P  k  idx join rows min_size root size label count status ws stream
COMPONENTS = [
    ((-1, 3, F, N, N, 1, F, F, F, F, F, F, N), "goi_knn_segment_components: bad P"),
    ((10, 0, F, N, N, 1, F, F, F, F, F, F, N), "goi_knn_segment_components: need k >= 1"),
    ((2 ** 29, 2, F, N, N, 1, F, F, F, F, F, F, N), "goi_knn_segment_components: need P * k < 2^30"),
    ((10, 3, F, N, N, 0, F, F, F, F, F, F, N), "goi_knn_segment_components: need min_size >= 1"),
    ((10, 3, F, N, N, -5, F, F, F, F, F, F, N), "goi_knn_segment_components: need min_size >= 1"),
    ((10, 3, N, N, N, 1, F, F, F, F, F, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, N, F, F, F, F, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, F, N, F, F, F, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, F, F, N, F, F, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, F, F, F, N, F, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, F, F, F, F, N, F, N), "goi_knn_segment_components: a required pointer is NULL"),
    ((10, 3, F, N, N, 1, F, ODD, F, F, F, F, N),
     "goi_knn_segment_components: idx, root, size, label, count and status must be 4-byte aligned"),
    ((10, 3, F, N, N, 1, F, F, F, F, F, N, N), "goi_knn_segment_components: NULL workspace"),
    ((10, 3, F, N, N, 1, F, F, F, F, F, MIS, N), "goi_knn_segment_components: workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("entry,args,message", [("goi_knn_segment_edges", a, m) for a, m in EDGES]
                         + [("goi_knn_segment_components", a, m) for a, m in COMPONENTS])
def test_refusals_before_any_device_call(lib, entry, args, message):
    assert getattr(lib, entry)(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_an_empty_graph_returns_0_and_touches_nothing(lib):
    assert lib.goi_knn_segment_edges(0, 4, 3, N, N, INF, N, 0.0, 0, N, N, N, N) == 0
    assert lib.goi_knn_segment_edges(0, 4, 3, N, N, 1.0, N, 2.0, MUTUAL, N, N, N, N) == 0
    assert lib.goi_knn_segment_components(0, 3, N, N, N, 1, N, N, N, N, N, N, N) == 0
