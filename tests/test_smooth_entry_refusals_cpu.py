"""What the C entries of csrc/smooth.hip (goi_knn_transpose, goi_knn_smooth_loss, goi_knn_diffuse) declare, export and refuse
before any device call: beside tests/test_entry_refusals_cpu.py, which records the entries that were there before."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
G = C.c_void_p(2 << 20)
MIS = C.c_void_p((1 << 20) + 4)
N = None
NAMES = ("goi_knn_transpose_workspace_bytes", "goi_knn_transpose", "goi_knn_smooth_loss_workspace_bytes", "goi_knn_smooth_loss",
         "goi_knn_diffuse")


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_listed_as_later_additions(lib):
    from goi_hyperplane_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    assert set(_lib.SMOOTH_SYMBOLS) == set(NAMES)
    assert _lib.SMOOTH_SYMBOLS in _lib.LATER_TABLES and _lib.SMOOTH_SYMBOLS not in _lib.SYMBOL_TABLES
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert name in hdr.split("#define GOI_RASTER_ABI_VERSION")[0], f"{name} is not in the list of later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION


def test_workspace_sizes(lib):
    size = lib.goi_knn_transpose_workspace_bytes
    for bad in ((-1, 3), (10, 0), (10, -1), (2 ** 30, 1), (2 ** 26, 16), (2 ** 29, 2)):
        assert size(*bad) == 0
    grid = [0, 1, 255, 256, 257, 5000, 100_000, 3_000_000]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(a, 8) <= size(b, 8)
        assert size(a, 3) <= size(a, 16)
    assert size(2 ** 30 - 1, 1) > 0 and size(1000, 8) % 256 == 0
    assert size(1_000_000, 8) < 1_000_000 * 8 * 40  # below 40 bytes per entry
    loss = lib.goi_knn_smooth_loss_workspace_bytes
    assert loss(-1) == 0 and 0 < loss(0) == loss(1) == loss(10 ** 6) and loss(5) % 256 == 0


TRANSPOSE = [
    ((-1, 3, F, F, F, F, N), "goi_knn_transpose: bad P"),
    ((10, 0, F, F, F, F, N), "goi_knn_transpose: need k >= 1"),
    ((10, -2, F, F, F, F, N), "goi_knn_transpose: need k >= 1"),
    ((2 ** 30, 1, F, F, F, F, N), "goi_knn_transpose: need P * k < 2^30"),
    ((2 ** 26, 16, F, F, F, F, N), "goi_knn_transpose: need P * k < 2^30"),
    ((10, 3, N, F, F, F, N), "goi_knn_transpose: a required pointer is NULL"),
    ((10, 3, F, N, F, F, N), "goi_knn_transpose: a required pointer is NULL"),
    ((10, 3, F, F, N, F, N), "goi_knn_transpose: a required pointer is NULL"),
    ((0, 3, N, N, N, N, N), "goi_knn_transpose: a required pointer is NULL"),  # even an empty graph has in_ptr[0]
    ((10, 3, F, F, F, N, N), "goi_knn_transpose: NULL workspace"),
    ((10, 3, F, F, F, MIS, N), "goi_knn_transpose: workspace must be 256-byte aligned"),
]
#            P  S  k  f  idx w  rows in_ptr in_edge loss n_edges grad ws stream
LOSS = [
    ((-1, 4, 3, F, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: bad P"),
    ((10, 0, 3, F, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: need 1 <= S <= 32"),
    ((10, 33, 3, F, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: need 1 <= S <= 32"),
    ((10, 4, 0, F, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: need k >= 1"),
    ((2 ** 28, 4, 4, F, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: need P * k < 2^30"),
    ((10, 4, 3, N, F, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((10, 4, 3, F, N, N, N, F, F, F, F, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, F, F, N, F, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, F, F, F, N, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((0, 4, 3, N, N, N, N, N, N, N, F, N, N, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, N, F, F, F, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),  # a gradient needs the transpose
    ((10, 4, 3, F, F, N, N, F, N, F, F, F, F, N), "goi_knn_smooth_loss: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, N, N, F, F, N, N, N), "goi_knn_smooth_loss: NULL workspace"),              # (no gradient: none needed)
    ((10, 4, 3, F, F, N, N, F, F, F, F, F, MIS, N), "goi_knn_smooth_loss: workspace must be 256-byte aligned"),
]
#            P  S  k  f  idx w  fixed lam out stream
DIFFUSE = [
    ((-1, 4, 3, F, F, N, N, 1.0, G, N), "goi_knn_diffuse: bad P"),
    ((10, 0, 3, F, F, N, N, 1.0, G, N), "goi_knn_diffuse: need 1 <= S <= 32"),
    ((10, 33, 3, F, F, N, N, 1.0, G, N), "goi_knn_diffuse: need 1 <= S <= 32"),
    ((10, 4, 0, F, F, N, N, 1.0, G, N), "goi_knn_diffuse: need k >= 1"),
    ((2 ** 29, 4, 2, F, F, N, N, 1.0, G, N), "goi_knn_diffuse: need P * k < 2^30"),
    ((10, 4, 3, F, F, N, N, float("nan"), G, N), "goi_knn_diffuse: lam is NaN"),
    ((10, 4, 3, N, F, N, N, 1.0, G, N), "goi_knn_diffuse: a required pointer is NULL"),
    ((10, 4, 3, F, N, N, N, 1.0, G, N), "goi_knn_diffuse: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, 1.0, N, N), "goi_knn_diffuse: a required pointer is NULL"),
    ((10, 4, 3, F, F, N, N, 1.0, F, N), "goi_knn_diffuse: out must not be f (a Jacobi step reads the old values of every row)"),
]


@pytest.mark.parametrize("entry,args,message", [("goi_knn_transpose", a, m) for a, m in TRANSPOSE]
                         + [("goi_knn_smooth_loss", a, m) for a, m in LOSS] + [("goi_knn_diffuse", a, m) for a, m in DIFFUSE])
def test_refusals_before_any_device_call(lib, entry, args, message):
    assert getattr(lib, entry)(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_an_empty_diffusion_touches_nothing(lib):
    assert lib.goi_knn_diffuse(0, 4, 3, N, N, N, N, 1.0, N, N) == 0
