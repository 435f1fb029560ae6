"""What the C entries of csrc/mcmc.hip (goi_mcmc_relocate_workspace_bytes, goi_mcmc_relocate, goi_mcmc_noise,
goi_mcmc_debug_relocation_sum) declare, export and refuse before any device call: beside
tests/test_grouping_entry_refusals_cpu.py, in its pattern."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first (or has P = 0)
MIS = C.c_void_p((1 << 20) + 8)
ODD = C.c_void_p((1 << 20) + 2)
FOUR = C.c_void_p((1 << 20) + 4)
N = None
NAMES = ("goi_mcmc_relocate_workspace_bytes", "goi_mcmc_relocate", "goi_mcmc_noise", "goi_mcmc_debug_relocation_sum")
FN = "goi_mcmc_relocate: "
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def test_entries_are_declared_exported_and_listed_as_later_additions(lib):
    from goi_hyperplane_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "goi_raster.h")).read()
    assert set(_lib.MCMC_SYMBOLS) == set(NAMES)
    assert _lib.MCMC_SYMBOLS in _lib.LATER_TABLES and _lib.MCMC_SYMBOLS not in _lib.SYMBOL_TABLES
    assert not set(_lib.MCMC_SYMBOLS) & set(_lib.SYMBOLS)
    later = hdr.split("#define GOI_RASTER_ABI_VERSION")[0].split(" * 8:")[0]
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name)
        assert name in later, f"{name} belongs under ABI 9's later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    assert build.UNITS["mcmc.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "mcmc.hip")).read()
    for helper in ("Carver c(", "check_workspace(", '#include "entry.h"', '#include "workspace.h"'):
        assert helper in src, helper
    for restated in ("struct Carver", "int check_workspace", "round_up_256("):
        assert restated not in src, restated
    assert "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src  # integer atomics only
    assert len(_lib.MCMC_SYMBOLS["goi_mcmc_relocate"][1]) == 17 and len(_lib.MCMC_SYMBOLS["goi_mcmc_noise"][1]) == 11
    for name, value in (("GOI_MCMC_MAX_GROUPS", _lib.MCMC_MAX_GROUPS), ("GOI_MCMC_PARAM", _lib.MCMC_PARAM), ("GOI_MCMC_OPACITY", _lib.MCMC_OPACITY),
                        ("GOI_MCMC_SCALING", _lib.MCMC_SCALING), ("GOI_MCMC_MOMENT", _lib.MCMC_MOMENT)):
        assert int(re.search(r"#define " + name + r" (\d+)", hdr).group(1)) == value, name


def test_rows_struct_layout_matches_c(tmp_path):
    import subprocess
    from goi_hyperplane_amd._lib import GoiMcmcRows
    fields = [f[0] for f in GoiMcmcRows._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goi_raster.h"\nint main(void){\n'
                   + "".join(f'printf("{f} %zu\\n", offsetof(GoiMcmcRows, {f}));\n' for f in fields)
                   + 'printf("sizeof %zu\\n", sizeof(GoiMcmcRows));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for f in fields:
        assert getattr(GoiMcmcRows, f).offset == int(out[f]), f
    assert C.sizeof(GoiMcmcRows) == int(out["sizeof"])


def test_workspace_size(lib):
    size = lib.goi_mcmc_relocate_workspace_bytes
    for bad in (-1, 1 << 30, 1 << 40):
        assert size(bad) == 0, bad
    grid = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 5000, 1_000_000, (1 << 30) - 1]
    for a, b in zip(grid, grid[1:]):
        assert 0 < size(a) <= size(b)
    assert all(size(P) % 256 == 0 for P in grid)
    # C 8 + dead ids 4 + hits 4 + sources 4 + staged opacity 4 + staged log-scales 12 = 36 B per Gaussian, block sums 16 B per 1024
    assert 36 * 1_000_000 <= size(1_000_000) < 37 * 1_000_000


def rows(*groups):
    from goi_hyperplane_amd._lib import GoiMcmcRows
    return (GoiMcmcRows * max(len(groups), 1))(*[GoiMcmcRows(p.value if p is not None else None, rl, mode) for p, rl, mode in groups])


def args(P=8, opacity=F, draws=F, n_draws=8, selection=N, min_opacity=0.005, max_moves=8, num=1, den=1, n_max=51, groups=((F, 3, 0),),
         n_groups=None, hits=N, counts=F, status=F, ws=F):
    arr = rows(*groups) if groups is not None else None
    return (P, opacity, draws, n_draws, selection, min_opacity, max_moves, num, den, n_max, arr,
            (len(groups) if groups is not None else 1) if n_groups is None else n_groups, hits, counts, status, ws, N)


NULL = FN + "a required pointer is NULL"
FRAC = FN + "need 0 <= frac_num <= 2^32 and 1 <= frac_den <= 2^32"
REFUSALS = [
    (args(P=-1), FN + "need 0 <= P < 2^30"), (args(P=1 << 30), FN + "need 0 <= P < 2^30"),
    (args(n_draws=-1), FN + "need 0 <= n_draws < 2^30"), (args(n_draws=1 << 30), FN + "need 0 <= n_draws < 2^30"),
    (args(max_moves=-1), FN + "need max_moves >= 0"),
    (args(num=-1), FRAC), (args(num=(1 << 32) + 1), FRAC), (args(den=0), FRAC), (args(den=(1 << 32) + 1), FRAC),
    (args(n_max=0), FN + "need 1 <= n_max <= 51"), (args(n_max=52), FN + "need 1 <= n_max <= 51"),
    (args(min_opacity=-0.1), FN + "need 0 <= min_opacity < 1"), (args(min_opacity=1.0), FN + "need 0 <= min_opacity < 1"),
    (args(min_opacity=NAN), FN + "need 0 <= min_opacity < 1"),
    (args(n_groups=25), FN + "n_groups must be 0..24"), (args(n_groups=-1), FN + "n_groups must be 0..24"),
    (args(groups=None), FN + "groups is NULL"),
    (args(groups=((F, 0, 0),)), FN + "bad group"), (args(groups=((F, (1 << 20) + 1, 0),)), FN + "bad group"),
    (args(groups=((F, 3, 4),)), FN + "bad group"), (args(groups=((F, 3, -1),)), FN + "bad group"),
    (args(groups=((N, 3, 0),)), FN + "a group pointer is NULL"),
    (args(groups=((ODD, 3, 0),)), FN + "a group pointer is not 4-byte aligned"),
    (args(groups=((F, 3, 1),)), FN + "need at most one opacity group, of row length 1"),
    (args(groups=((F, 1, 1), (F, 1, 1))), FN + "need at most one opacity group, of row length 1"),
    (args(groups=((F, 1, 2),)), FN + "need at most one log-scale group, of row length 3"),
    (args(groups=((F, 3, 2), (F, 3, 2))), FN + "need at most one log-scale group, of row length 3"),
    (args(opacity=N), NULL), (args(draws=N), NULL), (args(counts=N), NULL), (args(status=N), NULL),
    (args(opacity=ODD), FN + "opacity, hits, counts and status must be 4-byte aligned"),
    (args(hits=ODD), FN + "opacity, hits, counts and status must be 4-byte aligned"),
    (args(counts=ODD), FN + "opacity, hits, counts and status must be 4-byte aligned"),
    (args(status=ODD), FN + "opacity, hits, counts and status must be 4-byte aligned"),
    (args(draws=FOUR), FN + "draws must be 8-byte aligned"),
    (args(ws=N), FN + "NULL workspace"), (args(ws=MIS), FN + "workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("a,message", REFUSALS)
def test_relocate_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_mcmc_relocate(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_the_order_of_the_refusals(lib):
    """sizes before numbers before groups before pointers before the workspace"""
    assert lib.goi_mcmc_relocate(*args(P=-1, n_max=0, opacity=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == FN + "need 0 <= P < 2^30"
    assert lib.goi_mcmc_relocate(*args(n_max=0, groups=((F, 0, 0),), opacity=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == FN + "need 1 <= n_max <= 51"
    assert lib.goi_mcmc_relocate(*args(groups=((F, 0, 0),), opacity=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == FN + "bad group"
    assert lib.goi_mcmc_relocate(*args(opacity=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == NULL


def test_p_zero_returns_zero_and_touches_nothing(lib):
    """P = 0: no pointer is looked at (none of these could be dereferenced), no device call is made (this machine has no device)"""
    assert lib.goi_mcmc_relocate(*args(P=0, opacity=N, draws=N, n_draws=0, counts=N, status=N, ws=N, groups=((N, 3, 0),))) == 0
    assert lib.goi_mcmc_relocate(*args(P=0, n_groups=0)) == 0
    assert lib.goi_mcmc_noise(0, N, N, N, N, N, N, 100.0, 0.995, 80.0, N) == 0
    assert lib.goi_mcmc_debug_relocation_sum(0, N, N, N, N) == 0
    assert lib.goi_mcmc_relocate(*args(P=0, n_max=0)) < 0  # the numbers are still checked


NOISE = "goi_mcmc_noise: "


def noise_args(P=8, xyz=F, rot=F, scal=F, op=F, z=F, sel=N, k=100.0, x0=0.995, step=80.0):
    return (P, xyz, rot, scal, op, z, sel, k, x0, step, N)


@pytest.mark.parametrize("a,message", [
    (noise_args(P=-1), NOISE + "need 0 <= P < 2^30"), (noise_args(P=1 << 30), NOISE + "need 0 <= P < 2^30"),
    (noise_args(k=NAN), NOISE + "k, x0 and step must be finite"), (noise_args(x0=INF), NOISE + "k, x0 and step must be finite"),
    (noise_args(step=-INF), NOISE + "k, x0 and step must be finite"),
    (noise_args(xyz=N), NOISE + "a required pointer is NULL"), (noise_args(rot=N), NOISE + "a required pointer is NULL"),
    (noise_args(scal=N), NOISE + "a required pointer is NULL"), (noise_args(op=N), NOISE + "a required pointer is NULL"),
    (noise_args(z=N), NOISE + "a required pointer is NULL"),
    (noise_args(xyz=ODD), NOISE + "xyz, rotation, scaling, opacity and z must be 4-byte aligned"),
    (noise_args(z=ODD), NOISE + "xyz, rotation, scaling, opacity and z must be 4-byte aligned"),
])
def test_noise_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_mcmc_noise(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_debug_sum_refusals(lib):
    fn = "goi_mcmc_debug_relocation_sum: "
    for a, message in (((-1, F, F, F, N), "need 0 <= n <= 2^24"), (((1 << 24) + 1, F, F, F, N), "need 0 <= n <= 2^24"),
                       ((4, N, F, F, N), "a required pointer is NULL"), ((4, F, N, F, N), "a required pointer is NULL"),
                       ((4, F, F, N, N), "a required pointer is NULL"), ((4, FOUR, F, F, N), "o_new and D must be 8-byte aligned"),
                       ((4, F, F, FOUR, N), "o_new and D must be 8-byte aligned"), ((4, F, ODD, F, N), "N must be 4-byte aligned")):
        assert lib.goi_mcmc_debug_relocation_sum(*a) < 0
        assert lib.goi_raster_last_error().decode() == fn + message
