"""Builds libgoi_raster.so (hand-written HIP for gfx950) in-tree with hipcc.

    python -m goi_hyperplane_amd.build [--force]

One hipcc invocation per translation unit (parallel), then a link.  The library lands next to
this file's package as goi_hyperplane_amd/lib/libgoi_raster.so so that it travels with the repo
snapshot to the GPU box (it is git-ignored, not gpurun-ignored).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libgoi_raster.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

COMMON = ["--offload-arch=" + ARCH] + os.environ.get("GOI_EXTRA_FLAGS", "").split() + ["-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
          "-munsafe-fp-atomics", "-Wall", "-Wno-unused-function"]
# per-file extra flags: the per-Gaussian kernels keep the reference's operation order
UNITS = {
    "api.hip": [],
    "scan_sort.hip": [],
    "preprocess_fwd.hip": ["-ffp-contract=off"],  # only the per-Gaussian arithmetic: radii / rectangles / depth keys integer-exact
    "preprocess_bwd.hip": ["-ffp-contract=off"],  # only the per-Gaussian arithmetic: radii / rectangles / depth keys integer-exact
    "binning.hip": [],
    "reduce_rows.hip": [],
    "render_fwd.hip": ["-fno-slp-vectorize"],
    "blend_stats.hip": [],
    "contrib.hip": [],
    "render_bwd.hip": ["-fno-slp-vectorize"],  # the vectoriser's packing costs the pair loop six moves and four VGPRs (the loop spells its roundings)
    "render_bwd_tile.hip": [],
    "render_bwd_sem.hip": [],
    "semantic_head.hip": [],
    "knn.hip": ["-ffp-contract=off"],
    "smooth.hip": ["-ffp-contract=off"],  # the gradient is compared bit for bit with its numpy restatement: t = a - b, acc + w * t, no FMA
    "segment.hip": ["-ffp-contract=off"],  # the feature gate is compared bit for bit: e = a - b, then the fmaf that is written out
    "instance.hip": ["-ffp-contract=off"],  # the float64 sums are compared bit for bit with their numpy restatement: t = w * d, acc + t * d, no FMA
    "grouping.hip": ["-ffp-contract=off"],  # the float64 means, pair terms and residual are held to their numpy restatement: one rounding per operation
    "adam.hip": ["-ffp-contract=off"],
    "codebook_loss.hip": [],
    "osh.hip": [],
    "dbscan.hip": ["-ffp-contract=off"],
    "masks.hip": [],
    "codebook_init.hip": [],
    "photometric.hip": [],
    "densify.hip": ["-ffp-contract=off"],  # the reference's elementwise torch ops, one rounding each
    "mcmc.hip": ["-ffp-contract=off"],  # the relocation sum and the noise are held to their float64 restatement: one rounding per operation
    "deform.hip": ["-ffp-contract=off"],  # the solve and the apply are held to their float32 restatement: one rounding per operation
    "display.hip": ["-ffp-contract=off"],  # the viewer's blend a*b + c*d is compared bit for bit: no FMA
    "pca.hip": ["-ffp-contract=off"],  # the projection and its normalisations are one rounding per operation
    "field.hip": ["-ffp-contract=off"],  # the iso-surface's vertices are one rounding per operation (the density loop names its FMAs)
    "mesh.hip": ["-ffp-contract=off"],  # null faces, cells, means and normals are compared bit for bit: one rounding per operation
    "texture.hip": ["-ffp-contract=off"],  # barycentrics, splat weights and upsampling are compared bit for bit: no FMA
    "edit.hip": ["-ffp-contract=off"],  # the edit is compared bit for bit with its numpy restatement: one rounding per operation
    "pose.hip": ["-ffp-contract=off"],  # the per-row pieces are held to their numpy restatement: one rounding per operation
}


EXT = os.path.join(LIBDIR, "_goi_C.so")  # the compiled torch binding (csrc/torch_binding.cpp), host C++ only
EXT_SRC = os.path.join(CSRC, "torch_binding.cpp")


def build_torch_binding(force: bool = False, verbose: bool = False) -> str:
    """g++ against the torch headers, linked with libgoi_raster.so (rpath $ORIGIN).  No hipcc, no hipify: the file
    contains no device code.  This is the binding a maintainer of the reference would build in place of
    submodules/diff-gaussian-rasterization (rasterize_points.cu + ext.cpp); _C.py uses it when it is there."""
    import sysconfig
    import torch
    hdr = os.path.join(ROOT, "include", "goi_raster.h")
    if not force and os.path.exists(EXT) and all(os.path.getmtime(f) <= os.path.getmtime(EXT) for f in (EXT_SRC, hdr, LIB)):
        return EXT
    tdir = os.path.dirname(torch.__file__)
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1",
           "-DUSE_ROCM=1", "-DTORCH_EXTENSION_NAME=_goi_C", "-DTORCH_API_INCLUDE_EXTENSION_H",
           f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
           "-I" + os.path.join(tdir, "include"), "-I" + os.path.join(tdir, "include", "torch", "csrc", "api", "include"),
           "-I" + sysconfig.get_paths()["include"], "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           EXT_SRC, "-o", EXT, "-L" + os.path.join(tdir, "lib"), "-ltorch", "-ltorch_cpu", "-ltorch_python", "-lc10",
           "-lc10_hip", "-ltorch_hip", "-L" + LIBDIR, "-lgoi_raster", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return EXT


def _newer(src: str, dst: str) -> bool:
    return (not os.path.exists(dst)) or os.path.getmtime(src) > os.path.getmtime(dst)


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")] + [
        os.path.join(ROOT, "include", "goi_raster.h")]
    hdr_time = max(os.path.getmtime(h) for h in headers)

    def compile_one(item):
        name, extra = item
        src = os.path.join(CSRC, name)
        obj = os.path.join(objdir, name + ".o")
        if force or _newer(src, obj) or hdr_time > os.path.getmtime(obj):
            cmd = [HIPCC] + COMMON + extra + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            return obj, True
        return obj, False

    with ThreadPoolExecutor(max_workers=4) as ex:
        results = list(ex.map(compile_one, UNITS.items()))
    objs = [o for o, _ in results]
    for stale in {f for f in os.listdir(objdir) if f.endswith(".hip.o")} - {os.path.basename(o) for o in objs}:
        os.remove(os.path.join(objdir, stale))  # a unit that left UNITS: tools/build_variant.sh links every object in here
    if force or any(c for _, c in results) or not os.path.exists(LIB):
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    try:
        build_torch_binding(force=force, verbose=verbose)
    except Exception as ex:  # noqa: BLE001 -- libgoi_raster.so is built and the ctypes binding needs nothing else
        import warnings
        if os.path.exists(EXT):
            os.remove(EXT)  # never leave a stale binding next to a newer library
        warnings.warn(f"the compiled torch binding (_goi_C.so) could not be built: {ex}; goi_hyperplane_amd._C falls back "
                      "to its ctypes binding of the same C ABI (same kernels, ~0.14 ms more host time per step)")
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
