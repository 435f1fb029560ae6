"""What the C entries of csrc/grouping.hip (goi_mask_contrast_workspace_bytes, goi_mask_contrast) declare, export and refuse
before any device call: beside tests/test_instance_entry_refusals_cpu.py, in its pattern."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 8)  # 8-byte aligned only
ODD = C.c_void_p((1 << 20) + 2)
FOUR = C.c_void_p((1 << 20) + 4)
N = None
NAMES = ("goi_mask_contrast_workspace_bytes", "goi_mask_contrast")
FN = "goi_mask_contrast: "


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_listed_as_later_additions(lib):
    from goi_hyperplane_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    assert set(_lib.GROUPING_SYMBOLS) == set(NAMES)
    assert _lib.GROUPING_SYMBOLS in _lib.LATER_TABLES and _lib.GROUPING_SYMBOLS not in _lib.SYMBOL_TABLES
    assert not set(_lib.GROUPING_SYMBOLS) & set(_lib.SYMBOLS)
    later = hdr.split("#define GOI_RASTER_ABI_VERSION")[0].split(" * 8:")[0]
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name)
        assert name in later, f"{name} belongs under ABI 9's later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    assert os.path.exists(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "grouping.hip"))
    assert build.UNITS["grouping.hip"] == ["-ffp-contract=off"]
    # the shared helpers stay where they are: the unit uses them and defines none of them
    src = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "grouping.hip")).read()
    for helper in ("Carver c(", "check_workspace(", "wave_sum(", "wave_butterfly(", '#include "entry.h"', '#include "workspace.h"',
                   '#include "wave_util.h"'):
        assert helper in src, helper
    for restated in ("struct Carver", "int check_workspace", "T wave_butterfly", "round_up_256("):
        assert restated not in src, restated
    assert len(_lib.GROUPING_SYMBOLS["goi_mask_contrast"][1]) == 21 and len(_lib.GROUPING_SYMBOLS[NAMES[0]][1]) == 4


def test_workspace_size_is_monotone_a_multiple_of_256_and_0_for_refused_shapes(lib):
    size = lib.goi_mask_contrast_workspace_bytes
    for bad in ((0, 8, 8, 3), (33, 8, 8, 3), (4, 0, 8, 3), (4, 8, 0, 3), (4, 2049, 2048, 3), (4, 8, 8, -1), (4, 8, 8, 65537), (-1, -1, -1, -1),
                (4, 2 ** 31 - 1, 2 ** 31 - 1, 3)):
        assert size(*bad) == 0, bad
    grid = [0, 1, 2, 63, 64, 65, 300, 4096, 65536]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(16, 64, 64, a) <= size(16, 64, 64, b)  # monotone in K
    for a, b in zip(range(1, 32), range(2, 33)):
        assert size(a, 64, 64, 300) <= size(b, 64, 64, 300)  # in S
    for a, b in ((1, 2), (2, 64), (64, 1056), (1056, 2048)):
        assert size(16, a, 7, 300) <= size(16, b, 7, 300) and size(16, 7, a, 300) <= size(16, 7, b, 300)  # in H and W
    for K in grid:
        for S in (1, 16, 17, 32):
            assert size(S, 37, 53, K) % 256 == 0
    assert size(32, 2048, 2048, 65536) > 0 and size(1, 1, 1, 0) > 0
    assert size(16, 1056, 1600, 300) < 1 << 17  # tables by mask, nothing by pixel


def args(S=4, H=8, W=8, K=3, feat=F, labels=F, margin=1.0, w_intra=1.0, w_inter=1.0, balance=0, max_abs=-1.0, loss=F, intra=F, inter=F,
         grad=F, count=F, qsum=F, qexp=F, status=F, ws=F):
    return (S, H, W, K, feat, labels, margin, w_intra, w_inter, balance, max_abs, loss, intra, inter, grad, count, qsum, qexp, status, ws, N)


NULL = FN + "a required pointer is NULL"
ALIGN4 = FN + "feat, labels, loss, intra, inter, grad, qexp and status must be 4-byte aligned"
ALIGN8 = FN + "count and qsum must be 8-byte aligned"
NUMBERS = FN + "need a finite margin >= 0 and finite weights"
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (args(S=0), FN + "need 1 <= S <= 32"), (args(S=33), FN + "need 1 <= S <= 32"), (args(S=-1, H=0), FN + "need 1 <= S <= 32"),
    (args(H=0), FN + "need H >= 1 and W >= 1"), (args(W=0), FN + "need H >= 1 and W >= 1"), (args(H=-3, K=-1), FN + "need H >= 1 and W >= 1"),
    (args(H=2049, W=2048), FN + "need H * W <= 2^22"), (args(H=2 ** 31 - 1, W=2 ** 31 - 1), FN + "need H * W <= 2^22"),
    (args(K=-1), FN + "need 0 <= K <= 65536"), (args(K=65537), FN + "need 0 <= K <= 65536"),
    (args(balance=2), FN + "balance must be 0 (pixel) or 1 (mask)"), (args(balance=-1), FN + "balance must be 0 (pixel) or 1 (mask)"),
    (args(margin=-1.0), NUMBERS), (args(margin=NAN), NUMBERS), (args(margin=INF), NUMBERS), (args(w_intra=NAN), NUMBERS),
    (args(w_inter=INF), NUMBERS), (args(w_intra=-INF), NUMBERS),
    (args(max_abs=NAN), FN + "max_abs must be finite (negative: not given)"),
    (args(max_abs=INF), FN + "max_abs must be finite (negative: not given)"),
    (args(feat=N), NULL), (args(labels=N), NULL), (args(loss=N), NULL), (args(intra=N), NULL), (args(inter=N), NULL),
    (args(count=N), NULL), (args(qsum=N), NULL), (args(qexp=N), NULL), (args(status=N), NULL), (args(K=0, qexp=N), NULL),
    (args(feat=ODD), ALIGN4), (args(labels=ODD), ALIGN4), (args(loss=ODD), ALIGN4), (args(intra=ODD), ALIGN4), (args(inter=ODD), ALIGN4),
    (args(grad=ODD), ALIGN4), (args(qexp=ODD), ALIGN4), (args(status=ODD), ALIGN4),
    (args(count=FOUR), ALIGN8), (args(qsum=FOUR), ALIGN8), (args(count=ODD), ALIGN8),
    (args(ws=N), FN + "NULL workspace"), (args(ws=MIS), FN + "workspace must be 256-byte aligned"),
    (args(K=0, ws=N), FN + "NULL workspace"),
]


@pytest.mark.parametrize("a,message", REFUSALS)
def test_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_mask_contrast(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_the_order_of_the_refusals(lib):
    """sizes before numbers before pointers before the workspace: a call that is wrong in several ways names the first"""
    assert lib.goi_mask_contrast(*args(S=0, margin=NAN, feat=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == FN + "need 1 <= S <= 32"
    assert lib.goi_mask_contrast(*args(margin=NAN, feat=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == NUMBERS
    assert lib.goi_mask_contrast(*args(feat=N, count=FOUR, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == NULL
