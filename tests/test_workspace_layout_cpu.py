"""The workspace layouts, without a GPU: every `*_bytes` function of the library is host-only, and csrc/workspace.h is plain C++.

PINS BELOW ARE DELIBERATE.  The table records what every size function (and the one exported piece offset) returned BEFORE the
modules were moved onto the one carver of csrc/workspace.h, on a grid that holds, per function, the smallest arguments the
entry accepts (zero counts included where it accepts them), a size that is no multiple of 64 elements, a large size and every
branch the layout has.  A layout that comes out one byte different is a piece that moved or a workspace the callers
under-allocate.  A change that MEANS to alter a layout updates the table in the same commit; nothing else should touch it.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


# function -> [(arguments, bytes)].  Notes on the branches:
#   backward scratch / contrib offset   S = 1, 16, 32: the row is 16, 32 or 48 floats
#   photometric                         flags 0, GRAD1, GRAD2, both: 0, 3, 3 or 4 stored maps
#   unique rows                         H W on both sides of GOI_CODEBOOK_RANK_MAX = 4096 and D on both sides of 8192: past either
#                                       the layout also holds the radix sort's buffers
#   mesh components / normals           take V = 0 and F = 0; clean / decimate need V, F >= 1
PINS = {
    "goi_raster_geom_bytes": [
        ((0,), 53316),
        ((1,), 53316),
        ((1000,), 164676),
        ((100_000,), 11777540),
        ((3_000_000,), 345542948),
    ],
    "goi_raster_image_bytes": [
        ((1, 1), 1568),
        ((200, 152), 132160),
        ((1237, 821), 4355328),
        ((3840, 2160), 35511296),
    ],
    "goi_raster_binning_bytes": [
        ((0,), 47168),
        ((1,), 47168),
        ((1000,), 63008),
        ((5_000_000,), 87854560),
    ],
    "goi_raster_backward_scratch_bytes": [
        ((0, 1), 1537),
        ((0, 16), 1793),
        ((0, 32), 2049),
        ((1000, 1), 262120),
        ((1000, 16), 518120),
        ((1000, 32), 774120),
        ((2_000_000, 1), 522084224),
        ((2_000_000, 16), 1034084224),
        ((2_000_000, 32), 1546084224),
    ],
    "goi_raster_debug_backward_contrib_offset": [
        ((0, 1), 1024),
        ((0, 16), 1280),
        ((0, 32), 1536),
        ((1000, 1), 260608),
        ((1000, 16), 516608),
        ((1000, 32), 772608),
        ((2_000_000, 1), 520083712),
        ((2_000_000, 16), 1032083712),
        ((2_000_000, 32), 1544083712),
    ],
    "goi_raster_debug_sort_workspace_bytes": [
        ((0, 0, 32), 45568),
        ((1, 0, 32), 45568),
        ((1000, 0, 32), 45568),
        ((5_000_000, 0, 32), 5353984),
        ((3_000_000, 0, 13), 6414848),
    ],
    "goi_raster_debug_scan_workspace_bytes": [
        ((0,), 320),
        ((1,), 324),
        ((1000,), 324),
        ((5_000_000,), 10088),
    ],
    "goi_raster_debug_reduce_workspace_bytes": [
        ((0,), 800),
        ((1,), 800),
        ((1000,), 832),
        ((5_000_000,), 209120),
    ],
    "goi_raster_densify_workspace_bytes": [
        ((0,), 768),
        ((1,), 1280),
        ((1000,), 17920),
        ((3_000_000,), 51024128),
    ],
    "goi_raster_photometric_workspace_bytes": [
        ((1, 1, 1, 1, 0), 512),
        ((1, 1, 1, 1, 1), 1280),
        ((1, 1, 1, 1, 2), 1280),
        ((1, 1, 1, 1, 3), 1536),
        ((1, 3, 152, 200, 0), 1536),
        ((1, 3, 152, 200, 1), 1095936),
        ((1, 3, 152, 200, 2), 1095936),
        ((1, 3, 152, 200, 3), 1460736),
        ((2, 3, 821, 1237, 0), 73472),
        ((2, 3, 821, 1237, 1), 73195520),
        ((2, 3, 821, 1237, 2), 73195520),
        ((2, 3, 821, 1237, 3), 97569536),
        ((1, 3, 2160, 3840, 0), 294144),
        ((1, 3, 2160, 3840, 1), 298892544),
        ((1, 3, 2160, 3840, 2), 298892544),
        ((1, 3, 2160, 3840, 3), 398425344),
    ],
    "goi_knn_workspace_bytes": [
        ((1,), 50944),
        ((1000,), 78592),
        ((1_000_000,), 36421376),
    ],
    "goi_semantic_dbscan_workspace_bytes": [
        ((1,), 49920),
        ((1000,), 156416),
        ((3_000_000,), 333421312),
    ],
    "goi_field_density_workspace_bytes": [
        ((1, 4, 1, 0.0), 48128),
        ((1000, 64, 8, 0.5), 133632),
        ((2_000_000, 256, 16, 4.0), 168632832),
    ],
    "goi_field_iso_workspace_bytes": [
        ((1, 1, 1), 1024),
        ((9, 7, 5), 3584),
        ((256, 256, 100), 59008512),
    ],
    "goi_mesh_components_workspace_bytes": [
        ((0, 0), 768),
        ((0, 5), 768),
        ((5, 0), 768),
        ((1000, 1999), 5376),
        ((2_000_000, 4_000_001), 10000384),
    ],
    "goi_mesh_clean_workspace_bytes": [
        ((1, 1), 49408),
        ((1000, 1999), 136704),
        ((2_000_000, 4_000_001), 178554880),
    ],
    "goi_mesh_decimate_workspace_bytes": [
        ((1, 1), 95488),
        ((1000, 1999), 194304),
        ((2_000_000, 4_000_001), 211099648),
    ],
    "goi_mesh_normals_workspace_bytes": [
        ((0, 0), 42496),
        ((0, 5), 46592),
        ((5, 0), 42496),
        ((1000, 1999), 162304),
        ((2_000_000, 4_000_001), 204793344),
    ],
    "goi_texture_rasterize_workspace_bytes": [
        ((0, 1, 1), 768),
        ((1000, 37, 53), 20224),
        ((2_000_000, 2048, 2048), 41554688),
    ],
    "goi_texture_grid_put_workspace_bytes": [
        ((0, 1, 1, 1), 42752),
        ((1000, 3, 37, 53), 153600),
        ((5_000_000, 4, 1024, 1024), 362262784),
    ],
    "goi_texture_fill_workspace_bytes": [
        ((1, 1), 512),
        ((37, 53), 4096),
        ((4096, 4096), 33554432),
    ],
    "goi_codebook_unique_rows_workspace_bytes": [
        ((1, 1, 1, 1), 1792),
        ((2, 10, 37, 53), 143360),
        ((1, 3, 64, 64), 164096),
        ((1, 3, 1, 4097), 358400),
        ((1, 8192, 3, 3), 296448),
        ((1, 8193, 3, 3), 343040),
        ((4, 16, 1080, 1920), 117334528),
    ],
    "goi_codebook_kmeans_workspace_bytes": [
        ((0, 1, 1, 1), 512),
        ((1000, 3, 37, 10), 9216),
        ((5_000_000, 8, 300, 256), 22467328),
    ],
    "goi_codebook_sim_workspace_bytes": [
        ((), 311296),
    ],
    "goi_codebook_fused_workspace_bytes": [
        ((0,), 351232),
        ((4,), 515328),
        ((1000,), 1662976),
        ((30_400,), 39375616),
        ((2_073_600,), 2656632832),
    ],
}


def _cases():
    return [pytest.param(name, args, want, id=f"{name[4:]}{args}") for name, rows in PINS.items() for args, want in rows]


@pytest.mark.parametrize("name,args,want", _cases())
def test_layout_is_pinned(lib, name, args, want):
    assert getattr(lib, name)(*args) == want


CARVER_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "workspace.h"
using goi::Carver;

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)

struct Piece { char* p; size_t bytes; };

// one sequence of takes: every element size, a zero count in the middle and at the end, sizes that are no multiple of 256
static int run(void* base, Piece* out, size_t* end, size_t* bytes) {
    Carver c(base);
    int n = 0;
    size_t before;
    CHECK(c.end() == 0 && c.bytes() == 0);
    out[n++] = {reinterpret_cast<char*>(c.take<uint8_t>(1)), 1};
    out[n++] = {reinterpret_cast<char*>(c.take<uint32_t>(3)), 12};
    before = c.end();
    out[n++] = {reinterpret_cast<char*>(c.take<double>(0)), 0};
    CHECK(c.end() == before);  // a zero count consumes nothing
    out[n++] = {reinterpret_cast<char*>(c.take<float>(1000)), 4000};
    out[n++] = {reinterpret_cast<char*>(c.take<uint8_t>(257)), 257};
    out[n++] = {reinterpret_cast<char*>(c.take<uint64_t>(64)), 512};  // (ends on a boundary)
    out[n++] = {reinterpret_cast<char*>(c.take<uint16_t>(5)), 10};
    before = c.end();
    out[n++] = {reinterpret_cast<char*>(c.take<uint32_t>(0)), 0};
    CHECK(c.end() == before);
    CHECK(c.bytes() % 256 == 0 && c.bytes() >= c.end() && c.bytes() - c.end() < 256);
    *end = c.end();
    *bytes = c.bytes();
    return n;
}

int main() {
    Piece sized[16], real[16];
    size_t end0 = 0, bytes0 = 0;
    const int n = run(nullptr, sized, &end0, &bytes0);
    CHECK(n == 8);
    for (int i = 0; i < n; i++) CHECK(sized[i].p == nullptr);  // sizing: every take returns NULL
    CHECK(end0 == 256 + 256 + 4096 + 512 + 512 + 10 && bytes0 == end0 + 246);  // (the last piece is not padded by end())
    char* buf = static_cast<char*>(std::aligned_alloc(256, bytes0 + 512));
    CHECK(buf != nullptr);
    const size_t shifts[] = {0, 1, 64, 255};
    for (size_t shift : shifts) {
        char* base = buf + shift;
        char* first = buf + (shift ? 256 : 0);  // the base rounded up
        size_t end1 = 0, bytes1 = 0;
        CHECK(run(base, real, &end1, &bytes1) == n);
        CHECK(end1 == end0 && bytes1 == bytes0);  // the same sequence sizes the same with and without a buffer
        CHECK(real[0].p == first);
        char* prev_end = first;
        for (int i = 0; i < n; i++) {
            CHECK(reinterpret_cast<uintptr_t>(real[i].p) % 256 == 0);
            CHECK(real[i].p >= prev_end);                                // disjoint and in call order
            CHECK(real[i].p - prev_end < 256);                           // and no further than the next boundary
            CHECK(!real[i].bytes || real[i].p + real[i].bytes <= first + end1);  // inside what end() reports
            if (real[i].bytes) prev_end = real[i].p + real[i].bytes;
        }
        CHECK(prev_end == first + end1);
    }
    std::free(buf);
    std::printf("ok\n");
    return 0;
}
"""


def test_carver(tmp_path):
    """csrc/workspace.h on its own, built with the host C++ compiler: NULL base sizes exactly like a real one, every piece is
    256-byte aligned from a base off by 0, 1, 64 and 255 bytes, pieces are disjoint and in call order, a zero count takes
    nothing, and bytes() pads end() by less than 256."""
    src = tmp_path / "carver.cpp"
    src.write_text(CARVER_PROGRAM)
    exe = tmp_path / "carver"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "goi_hyperplane_amd", "csrc"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
