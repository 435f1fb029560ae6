"""Writes ref_field_pins.npz: the reference's own gaussian_3d_coeff, build_scaling_rotation and strip_symmetric
(gui/gs_renderer.py:52-119) run in fp32 on the CPU.  The functions are executed from the reference's AST (the module imports
plyfile, simple_knn and the rasterizer), nothing re-typed, under make_golden.py's device redirection.  Only inputs and
outputs are recorded:

    coeff_xyz [N,3], coeff_cov [N,6] -> coeff_w [N]     offsets and covariances of random Gaussians, with rows that are
                                                        near-singular (one scale 1e-4 of the others), exactly singular
                                                        (det = 0: the 1e-24 decides) and indefinite (power > 0: weight 0)
    sr_scale [M,3], sr_rot [M,4] -> sr_L [M,3,3], sr_cov [M,6]     L = build_scaling_rotation(s, r) and
                                                        strip_symmetric(L @ L.transpose(1, 2)), quaternions of any norm

    python tests/golden/make_field_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

REF = make_golden.REF = os.environ.get("GOI_REFERENCE", make_golden.REF)
NAMES = ("strip_lowerdiag", "strip_symmetric", "gaussian_3d_coeff", "build_rotation", "build_scaling_rotation")


def reference_functions():
    tree = make_golden._ref_ast("gui/gs_renderer.py")
    stmts = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert len(stmts) == len(NAMES)
    return make_golden._exec_stmts(stmts, {"torch": torch}, "gui/gs_renderer.py")


def main():
    ns = reference_functions()
    g = torch.Generator().manual_seed(20)
    M = 320
    scale = torch.exp(torch.randn(M, 3, generator=g) * 0.8 - 2.5)
    scale[:40, 1] = scale[:40, 0] * 1e-4  # near-singular covariances
    rot = torch.randn(M, 4, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    with make_golden._cuda_is_cpu(), torch.no_grad():
        L = ns["build_scaling_rotation"](scale, rot)
        cov = ns["strip_symmetric"](L @ L.transpose(1, 2))
    N = 400
    ccov = cov[torch.randint(0, M, (N,), generator=g)].clone()
    ccov[300:330] = 0.0  # det = 0 exactly: inv_det = 1e24
    ccov[300:330, 0] = torch.rand(30, generator=g) * 1e-3
    ccov[330:370, 1] = ccov[330:370, 0] * 3.0  # |b| > sqrt(a d): indefinite, some powers > 0
    ccov[330:370, 3] = ccov[330:370, 0]
    xyz = torch.randn(N, 3, generator=g) * torch.sqrt(ccov[:, [0, 3, 5]].abs() + 1e-8) * 1.5
    with make_golden._cuda_is_cpu(), torch.no_grad():
        w = ns["gaussian_3d_coeff"](xyz.clone(), ccov.clone())
    out = dict(coeff_xyz=xyz.numpy(), coeff_cov=ccov.numpy(), coeff_w=w.numpy(), sr_scale=scale.numpy(), sr_rot=rot.numpy(),
               sr_L=L.numpy(), sr_cov=cov.numpy())
    path = os.path.join(HERE, "ref_field_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; zero weights:", int((w == 0).sum()), "nan:", int(torch.isnan(w).sum()),
          "weights in (0, 1):", int(((w > 0) & (w < 1)).sum()))


if __name__ == "__main__":
    main()
