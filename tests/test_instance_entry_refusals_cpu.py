"""What the C entries of csrc/instance.hip (goi_instance_members, goi_instance_stats) declare, export and refuse before any device
call: beside tests/test_segment_entry_refusals_cpu.py, in its pattern."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first
MIS = C.c_void_p((1 << 20) + 4)  # 4-byte aligned only
ODD = C.c_void_p((1 << 20) + 2)
N = None
NAMES = ("goi_instance_members_workspace_bytes", "goi_instance_members", "goi_instance_stats_workspace_bytes", "goi_instance_stats")
BIG = 2 ** 30


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_listed_as_later_additions(lib):
    from goi_hyperplane_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    assert set(_lib.INSTANCE_SYMBOLS) == set(NAMES)
    # bound by load() through LATER_TABLES only: not one of the tables of entries that moved out of api.hip, and -- like the
    # goi_pose_* family, whose prefix tests/test_abi_cpu.py's header scan does not cover either -- not part of SYMBOLS
    assert _lib.INSTANCE_SYMBOLS in _lib.LATER_TABLES and _lib.INSTANCE_SYMBOLS not in _lib.SYMBOL_TABLES
    assert not set(_lib.INSTANCE_SYMBOLS) & set(_lib.SYMBOLS)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name)
        assert name in hdr.split("#define GOI_RASTER_ABI_VERSION")[0], f"{name} is not in the list of later additions"
    later = hdr.split("#define GOI_RASTER_ABI_VERSION")[0].split(" * 8:")[0]
    assert all(name in later for name in NAMES), "the names belong under ABI 9's later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    assert os.path.exists(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "instance.hip"))
    assert build.UNITS["instance.hip"] == ["-ffp-contract=off"]
    # the shared helpers stay where they are: the unit calls them and defines none of them
    src = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "instance.hip")).read()
    for helper in ("exclusive_scan_u32(", "radix_sort_pairs(", "carve_sort(", "tile_key_bits(", "Carver c("):
        assert helper in src, helper
    atomics = re.findall(r"\batomic\w+\(([^,]+),", src)
    assert atomics and all(target.startswith("cnt") for target in atomics), "only the integer counts are atomic"
    args_members, args_stats = _lib.INSTANCE_SYMBOLS["goi_instance_members"][1], _lib.INSTANCE_SYMBOLS["goi_instance_stats"][1]
    assert len(args_members) == 7 and len(args_stats) == 19


@pytest.mark.parametrize("which", ["goi_instance_members_workspace_bytes", "goi_instance_stats_workspace_bytes"])
def test_workspace_size_is_monotone_a_multiple_of_256_and_0_for_refused_shapes(lib, which):
    size = getattr(lib, which)
    for bad in ((-1, 3), (10, -1), (BIG, 1), (10, BIG), (2 ** 31 - 1, 2 ** 31 - 1), (-5, -5)):
        assert size(*bad) == 0
    grid = [0, 1, 63, 64, 65, 255, 256, 257, 5000, 100_000, 1_000_000, 3_000_000]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(a, 1000) <= size(b, 1000)  # monotone in P
        assert 0 < size(100_000, a) <= size(100_000, b)  # and in K
    for v in grid:
        assert size(v, 1000) % 256 == 0 and size(100_000, v) % 256 == 0 and size(v, v) % 256 == 0
    assert size(BIG - 1, BIG - 1) > 0 and size(0, 0) > 0
    per_row = 4 if which.endswith("stats_workspace_bytes") else 24  # slots: 400 bytes per 128 rows; the sort's four arrays and scratch
    assert size(1_000_000, 50_000) < 1_000_000 * per_row + 50_000 * 12 + (1 << 16)


#          P  K  label ptr member ws stream
MEMBERS = [
    ((-1, 3, F, F, F, F, N), "goi_instance_members: bad P"),
    ((10, -1, F, F, F, F, N), "goi_instance_members: bad K"),
    ((-1, -1, F, F, F, F, N), "goi_instance_members: bad P"),
    ((BIG, 3, F, F, F, F, N), "goi_instance_members: need P < 2^30 and K < 2^30"),
    ((10, BIG, F, F, F, F, N), "goi_instance_members: need P < 2^30 and K < 2^30"),
    ((10, 3, N, F, F, F, N), "goi_instance_members: a required pointer is NULL"),
    ((10, 3, F, N, F, F, N), "goi_instance_members: a required pointer is NULL"),
    ((10, 3, F, F, N, F, N), "goi_instance_members: a required pointer is NULL"),
    ((0, 3, N, N, N, N, N), "goi_instance_members: a required pointer is NULL"),  # member_ptr [K+1] is written even for P = 0
    ((10, 3, ODD, F, F, F, N), "goi_instance_members: label, member_ptr and member must be 4-byte aligned"),
    ((10, 3, F, ODD, F, F, N), "goi_instance_members: label, member_ptr and member must be 4-byte aligned"),
    ((10, 3, F, F, ODD, F, N), "goi_instance_members: label, member_ptr and member must be 4-byte aligned"),
    ((10, 3, F, F, F, N, N), "goi_instance_members: NULL workspace"),
    ((10, 3, F, F, F, MIS, N), "goi_instance_members: workspace must be 256-byte aligned"),
    ((10, 0, F, F, F, MIS, N), "goi_instance_members: workspace must be 256-byte aligned"),
]
ALIGN = "goi_instance_stats: every pointer but hit must be 4-byte aligned"
NULL = "goi_instance_stats: a required pointer is NULL"


def stats_args(P=10, K=3, S=4, ptr=F, member=F, xyz=F, f=F, w=N, hit=N, n=F, hits=F, wsum=F, centroid=F, lo=F, hi=F, cov=F, feature=F,
               ws=F):
    return (P, K, S, ptr, member, xyz, f, w, hit, n, hits, wsum, centroid, lo, hi, cov, feature, ws, N)


STATS = [
    (stats_args(P=-1), "goi_instance_stats: bad P"),
    (stats_args(K=-1), "goi_instance_stats: bad K"),
    (stats_args(P=BIG), "goi_instance_stats: need P < 2^30 and K < 2^30"),
    (stats_args(K=BIG), "goi_instance_stats: need P < 2^30 and K < 2^30"),
    (stats_args(S=0), "goi_instance_stats: need 1 <= S <= 32"),
    (stats_args(S=33), "goi_instance_stats: need 1 <= S <= 32"),
    (stats_args(S=-4, K=0), "goi_instance_stats: need 1 <= S <= 32"),
    (stats_args(ptr=N), NULL), (stats_args(member=N), NULL), (stats_args(n=N), NULL), (stats_args(hits=N), NULL),
    (stats_args(wsum=N), NULL), (stats_args(centroid=N), NULL), (stats_args(lo=N), NULL), (stats_args(hi=N), NULL),
    (stats_args(cov=N), NULL), (stats_args(feature=N), NULL),
    (stats_args(P=0, n=N), NULL),  # P = 0 with K > 0 still writes every instance's empty values
    (stats_args(ptr=ODD), ALIGN), (stats_args(member=ODD), ALIGN), (stats_args(xyz=ODD), ALIGN), (stats_args(f=ODD), ALIGN),
    (stats_args(w=ODD), ALIGN), (stats_args(n=ODD), ALIGN), (stats_args(hits=ODD), ALIGN), (stats_args(wsum=ODD), ALIGN),
    (stats_args(centroid=ODD), ALIGN), (stats_args(lo=ODD), ALIGN), (stats_args(hi=ODD), ALIGN), (stats_args(cov=ODD), ALIGN),
    (stats_args(feature=ODD), ALIGN),
    (stats_args(ws=N), "goi_instance_stats: NULL workspace"),
    (stats_args(ws=MIS), "goi_instance_stats: workspace must be 256-byte aligned"),
    (stats_args(P=0, ws=N), "goi_instance_stats: NULL workspace"),
]


@pytest.mark.parametrize("entry,args,message", [("goi_instance_members", a, m) for a, m in MEMBERS]
                         + [("goi_instance_stats", a, m) for a, m in STATS])
def test_refusals_before_any_device_call(lib, entry, args, message):
    assert getattr(lib, entry)(*args) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_what_is_not_refused(lib):
    """S is not looked at without features; a hit pointer may be odd (bytes); K = 0 of stats returns 0 and touches nothing,
    whatever else is NULL."""
    assert lib.goi_instance_stats(*stats_args(K=0, ptr=N, member=N, xyz=N, f=N, n=N, hits=N, wsum=N, centroid=N, lo=N, hi=N, cov=N,
                                              feature=N, ws=N)) == 0
    assert lib.goi_instance_stats(*stats_args(P=0, K=0, S=99, f=N, ptr=N, n=N, ws=N)) == 0
    assert lib.goi_instance_stats(*stats_args(K=0, hit=C.c_void_p((1 << 20) + 1))) == 0
