"""What the C entries of csrc/deform.hip (goi_deform_solve_workspace_bytes, goi_deform_solve, goi_deform_energy_workspace_bytes,
goi_deform_energy, goi_deform_apply) declare, export and refuse before any device call: beside
tests/test_mcmc_entry_refusals_cpu.py, in its pattern."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = C.c_void_p(1 << 20)  # never dereferenced: every call below is refused first (or has nothing to do)
MIS = C.c_void_p((1 << 20) + 8)
ODD = C.c_void_p((1 << 20) + 2)
FOUR = C.c_void_p((1 << 20) + 4)
N = None
NAMES = ("goi_deform_solve_workspace_bytes", "goi_deform_solve", "goi_deform_energy_workspace_bytes", "goi_deform_energy",
         "goi_deform_apply")
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
    assert set(_lib.DEFORM_SYMBOLS) == set(NAMES)
    assert _lib.DEFORM_SYMBOLS in _lib.LATER_TABLES and _lib.DEFORM_SYMBOLS not in _lib.SYMBOL_TABLES
    assert not set(_lib.DEFORM_SYMBOLS) & set(_lib.SYMBOLS)
    later = hdr.split("#define GOI_RASTER_ABI_VERSION")[0].split(" * 8:")[0]
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name)
        assert name in later, f"{name} belongs under ABI 9's later additions"
    assert lib.goi_raster_abi_version() == _lib.ABI_VERSION == 9
    assert build.UNITS["deform.hip"] == ["-ffp-contract=off"]
    src = open(os.path.join(ROOT, "goi_hyperplane_amd", "csrc", "deform.hip")).read()
    for helper in ("Carver c(", "check_workspace(", '#include "entry.h"', '#include "workspace.h"', '#include "rest_row.h"'):
        assert helper in src, helper
    for restated in ("struct Carver", "int check_workspace", "round_up_256(", "edit_selected(const"):
        assert restated not in src, restated
    assert "atomic" not in src.split("namespace goi {")[1]  # no atomics at all: every sum has one order
    assert "hipDeviceSynchronize" not in src and "hipStreamSynchronize" not in src and "hipLaunchCooperativeKernel" not in src
    assert len(_lib.DEFORM_SYMBOLS["goi_deform_solve"][1]) == 16 and len(_lib.DEFORM_SYMBOLS["goi_deform_apply"][1]) == 21


def test_sh_struct_layout_matches_c(tmp_path):
    import subprocess
    from goi_hyperplane_amd._lib import GoiDeformSH
    fields = [f[0] for f in GoiDeformSH._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "goi_raster.h"\nint main(void){\n'
                   + "".join(f'printf("{f} %zu\\n", offsetof(GoiDeformSH, {f}));\n' for f in fields)
                   + 'printf("sizeof %zu\\n", sizeof(GoiDeformSH));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for f in fields:
        assert getattr(GoiDeformSH, f).offset == int(out[f]), f
    assert C.sizeof(GoiDeformSH) == int(out["sizeof"]) == 4 * (9 + 15 + 21 + 9 + 25 + 49)


def test_workspace_sizes(lib):
    for size in (lib.goi_deform_solve_workspace_bytes, lib.goi_deform_energy_workspace_bytes):
        for bad in (-1, 1 << 30):
            assert size(bad) == 0, bad
        grid = [0, 1, 2, 63, 64, 65, 300, 4000, 1_000_000, (1 << 30) - 1]
        for a, b in zip(grid, grid[1:]):
            assert 0 < size(a) <= size(b)
        assert all(size(M) % 256 == 0 for M in grid)
    assert 12 * 4000 <= lib.goi_deform_solve_workspace_bytes(4000) < 12 * 4000 + 256  # the second y buffer
    assert lib.goi_deform_energy_workspace_bytes(4000) == 8 * 1024                    # the per-workgroup partials


S = "goi_deform_solve: "


def solve_args(M=8, k=2, x=F, idx=F, weight=N, in_ptr=F, in_edge=F, con=N, target=N, iterations=1, polar=4, relax=0.8, y=F, q=F, ws=F):
    return (M, k, x, idx, weight, in_ptr, in_edge, con, target, iterations, polar, relax, y, q, ws, N)


ALIGN_S = S + "x, idx, weight, in_ptr, in_edge, target, y and q must be 4-byte aligned"
SOLVE_REFUSALS = [
    (solve_args(M=-1), S + "need M >= 0"), (solve_args(k=0), S + "need k >= 1"),
    (solve_args(M=1 << 28, k=4), S + "need M * k < 2^30"),
    (solve_args(iterations=-1), S + "need iterations >= 0"), (solve_args(polar=-1), S + "need polar_iters >= 0"),
    (solve_args(relax=0.0), S + "need 0 < relax <= 1"), (solve_args(relax=1.5), S + "need 0 < relax <= 1"),
    (solve_args(relax=NAN), S + "need 0 < relax <= 1"), (solve_args(relax=-INF), S + "need 0 < relax <= 1"),
    (solve_args(x=N), S + "a required pointer is NULL"), (solve_args(idx=N), S + "a required pointer is NULL"),
    (solve_args(in_ptr=N), S + "a required pointer is NULL"), (solve_args(in_edge=N), S + "a required pointer is NULL"),
    (solve_args(y=N), S + "a required pointer is NULL"), (solve_args(q=N), S + "a required pointer is NULL"),
    (solve_args(con=F, target=N), S + "a required pointer is NULL"),
    (solve_args(x=ODD), ALIGN_S), (solve_args(weight=ODD), ALIGN_S), (solve_args(in_edge=ODD), ALIGN_S),
    (solve_args(con=F, target=ODD), ALIGN_S), (solve_args(y=ODD), ALIGN_S), (solve_args(q=ODD), ALIGN_S),
    (solve_args(ws=N), S + "NULL workspace"), (solve_args(ws=MIS), S + "workspace must be 256-byte aligned"),
]


@pytest.mark.parametrize("a,message", SOLVE_REFUSALS)
def test_solve_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_deform_solve(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_the_order_of_the_solve_refusals_and_the_calls_with_nothing_to_do(lib):
    """sizes before numbers before pointers before the workspace; M = 0 and iterations = 0 look at no pointer"""
    assert lib.goi_deform_solve(*solve_args(M=-1, relax=0.0, x=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == S + "need M >= 0"
    assert lib.goi_deform_solve(*solve_args(relax=0.0, x=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == S + "need 0 < relax <= 1"
    assert lib.goi_deform_solve(*solve_args(x=N, ws=N)) < 0
    assert lib.goi_raster_last_error().decode() == S + "a required pointer is NULL"
    assert lib.goi_deform_solve(*solve_args(M=0, x=N, idx=N, in_ptr=N, in_edge=N, y=N, q=N, ws=N)) == 0
    assert lib.goi_deform_solve(*solve_args(iterations=0, x=N, idx=N, in_ptr=N, in_edge=N, y=N, q=N, ws=N)) == 0
    assert lib.goi_deform_solve(*solve_args(M=0, relax=2.0)) < 0  # the numbers are still checked


E = "goi_deform_energy: "


def energy_args(M=8, k=2, x=F, idx=F, weight=N, y=F, q=F, out=F, ws=F):
    return (M, k, x, idx, weight, y, q, out, ws, N)


@pytest.mark.parametrize("a,message", [
    (energy_args(M=-1), E + "need M >= 0"), (energy_args(k=0), E + "need k >= 1"), (energy_args(M=1 << 29, k=2), E + "need M * k < 2^30"),
    (energy_args(out=N), E + "a required pointer is NULL"), (energy_args(M=0, out=N), E + "a required pointer is NULL"),
    (energy_args(x=N), E + "a required pointer is NULL"), (energy_args(idx=N), E + "a required pointer is NULL"),
    (energy_args(y=N), E + "a required pointer is NULL"), (energy_args(q=N), E + "a required pointer is NULL"),
    (energy_args(out=FOUR), E + "energy must be 8-byte aligned"),
    (energy_args(x=ODD), E + "x, idx, weight, y and q must be 4-byte aligned"),
    (energy_args(weight=ODD), E + "x, idx, weight, y and q must be 4-byte aligned"),
    (energy_args(ws=N), E + "NULL workspace"), (energy_args(ws=MIS), E + "workspace must be 256-byte aligned"),
])
def test_energy_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_deform_energy(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


A = "goi_deform_apply: "


def sh_struct():
    from goi_hyperplane_amd import deform
    return deform._sh_struct()


def apply_args(P=8, M=16, n=4, kb=4, sel=N, invert=0, bidx=F, bd2=F, sigma=0.5, nx=F, ny=F, nq=F, sh=True, sx=F, sr=F, sc=F, x=F, r=F,
               c=F, moments=0):
    return (P, M, n, kb, sel, invert, bidx, bd2, sigma, nx, ny, nq, C.byref(sh_struct()) if sh else None, sx, sr, sc, x, r, c, moments, N)


NULL_A = A + "a required pointer is NULL"
ALIGN_A = A + "every tensor must be 4-byte aligned"
APPLY_REFUSALS = [
    (apply_args(P=-1), A + "need 0 <= P < 2^31"), (apply_args(P=1 << 31), A + "need 0 <= P < 2^31"),
    (apply_args(M=0), A + "M must be 1, 4, 9 or 16"), (apply_args(M=5), A + "M must be 1, 4, 9 or 16"),
    (apply_args(n=-1), A + "need 0 <= n_nodes < 2^30"), (apply_args(n=1 << 30), A + "need 0 <= n_nodes < 2^30"),
    (apply_args(kb=0), A + "need 1 <= kb <= 8"), (apply_args(kb=9), A + "need 1 <= kb <= 8"),
    (apply_args(P=1 << 29, kb=4), A + "need P * kb < 2^31"),
    (apply_args(sigma=0.0), A + "sigma must be finite and > 0"), (apply_args(sigma=-1.0), A + "sigma must be finite and > 0"),
    (apply_args(sigma=NAN), A + "sigma must be finite and > 0"), (apply_args(sigma=INF), A + "sigma must be finite and > 0"),
    (apply_args(moments=2), A + "moments must be 0 or 1"), (apply_args(sh=False), A + "the SH constants are NULL"),
    (apply_args(M=1), A + "M = 1 has no features_rest"),
    (apply_args(bidx=N), NULL_A), (apply_args(bd2=N), NULL_A), (apply_args(nq=N), NULL_A), (apply_args(nx=N), NULL_A),
    (apply_args(ny=N), NULL_A), (apply_args(sx=N), NULL_A), (apply_args(sr=N), NULL_A), (apply_args(sc=N), NULL_A),
    (apply_args(x=N), NULL_A), (apply_args(r=N), NULL_A), (apply_args(c=N), NULL_A),
    (apply_args(moments=1, bidx=N), NULL_A), (apply_args(moments=1, nq=N), NULL_A),
    (apply_args(bidx=ODD), ALIGN_A), (apply_args(nq=ODD), ALIGN_A), (apply_args(sc=ODD), ALIGN_A), (apply_args(c=ODD), ALIGN_A),
    (apply_args(x=ODD), ALIGN_A),
]


@pytest.mark.parametrize("a,message", APPLY_REFUSALS)
def test_apply_refusals_before_any_device_call(lib, a, message):
    assert lib.goi_deform_apply(*a) < 0
    assert lib.goi_raster_last_error().decode() == message


def test_apply_with_nothing_to_do_touches_nothing(lib):
    """P = 0 and n_nodes = 0: no pointer is looked at, no device call is made (this machine has no device)"""
    nothing = dict(bidx=N, bd2=N, nx=N, ny=N, nq=N, sx=N, sr=N, sc=N, x=N, r=N, c=N)
    assert lib.goi_deform_apply(*apply_args(P=0, **nothing)) == 0
    assert lib.goi_deform_apply(*apply_args(n=0, **nothing)) == 0
    assert lib.goi_deform_apply(*apply_args(P=0, kb=9)) < 0  # the numbers are still checked
    assert lib.goi_raster_last_error().decode() == A + "need 1 <= kb <= 8"
