"""Writes ref_mesh_pins.npz: the reference's own Mesh.auto_normal (gui/mesh.py:344-365) with its dot / length /
safe_normalize (gui/mesh.py:7-16), run in fp32 on the CPU.  The functions are executed from the reference's AST (the module
imports cv2 and trimesh), nothing re-typed, under make_golden.py's device redirection; the method runs against a namespace
object that holds only v and f.  Only inputs and outputs are recorded, per mesh of tests/mesh_reference.py (the iso-surfaces
of the sphere, torus, two-spheres and equal grids):

    <name>_v float32 [V,3], <name>_f int32 [F,3] -> <name>_vn float32 [V,3]

    python tests/golden/make_mesh_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import ast
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from tests import mesh_reference  # noqa: E402

REF = make_golden.REF = os.environ.get("GOI_REFERENCE", make_golden.REF)
HELPERS = ("dot", "length", "safe_normalize")
MESHES = ("sphere", "torus", "two_spheres", "equal")


def reference_auto_normal():
    tree = make_golden._ref_ast("gui/mesh.py")
    stmts = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in HELPERS]
    assert len(stmts) == len(HELPERS)
    ns = make_golden._exec_stmts(stmts + [make_golden._method(tree, "Mesh", "auto_normal")], {"torch": torch}, "gui/mesh.py")
    return ns["auto_normal"]


def main():
    auto_normal = reference_auto_normal()
    out, total = {}, 0
    for name in MESHES:
        v, f, _ = mesh_reference.grid_mesh(name)
        me = types.SimpleNamespace(v=torch.from_numpy(v.copy()), f=torch.from_numpy(f.copy()))
        with make_golden._cuda_is_cpu(), torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")  # torch.cross without dim
            auto_normal(me)
        out[name + "_v"], out[name + "_f"], out[name + "_vn"] = v, f, me.vn.numpy()
        total += len(v)
    path = os.path.join(HERE, "ref_mesh_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", total, "vertices")


if __name__ == "__main__":
    main()
