"""Writes ref_densify_pins.npz: the reference's own GaussianModel methods (scene/gaussian_model.py:291-513) run in fp32 on
the CPU.  The class is executed from the reference's AST (its module imports simple_knn and plyfile), nothing re-typed,
under make_golden.py's device redirection, on a small seeded model with a stepped 7-group torch.optim.Adam.

For the call, torch.normal is patched to draw the standard normals Z itself and return Z * std + mean, which is what torch
does internally (normal_(0, 1) on the output, then mul_(std), add_(mean)); Z is recorded so that a test can replay the
children.  Cases:
    dp_none      densify_and_prune(max_grad, min_opacity, extent, None)   clone, split, prune; denom-zero rows (0/0, x/0)
    dp_screen    densify_and_prune(..., max_screen_size=20)               plus the world-size prune of big Gaussians
    prune        prune_points(mask)
    reset        reset_opacity()
The inputs are stored once (in_*: parameters, statistics, each group's exp_avg / exp_avg_sq / step), the outputs per case
(<case>_*), with the thresholds and the model's seed.

    python tests/golden/make_densify_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from tests.densify_reference import PARAMS, STATS, make_model  # noqa: E402

REF = make_golden.REF = os.environ.get("GOI_REFERENCE", make_golden.REF)
CASE = dict(P=80, seed=5, scale_std=1.4, max_grad=2e-4, percent_dense=0.01, extent=4.0, min_opacity=0.1)


def reference_class():
    sys.path.insert(0, REF)
    from utils import general_utils as ge  # noqa
    tree = make_golden._ref_ast("scene/gaussian_model.py")
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GaussianModel")
    ns = {"torch": torch, "nn": nn, "np": np, "inverse_sigmoid": ge.inverse_sigmoid, "build_rotation": ge.build_rotation,
          "build_scaling_rotation": ge.build_scaling_rotation, "strip_symmetric": ge.strip_symmetric,
          "get_expon_lr_func": ge.get_expon_lr_func, "BasicPointCloud": object}  # (only an annotation of create_from_pcd)
    make_golden._exec_stmts([cls], ns, "scene/gaussian_model.py:GaussianModel")
    return ns["GaussianModel"]


def seeded():
    return make_model(CASE["P"], "cpu", seed=CASE["seed"], max_grad=CASE["max_grad"], percent_dense=CASE["percent_dense"],
                      extent=CASE["extent"], min_opacity=CASE["min_opacity"], scale_std=CASE["scale_std"])


def fresh(GM):
    """an instance of the reference class holding the seeded model and its optimizer"""
    src = seeded()
    g = GM(3, 16)
    for _, attr in PARAMS:
        setattr(g, attr, getattr(src, attr))
    for name in STATS:
        setattr(g, name, getattr(src, name))
    g.percent_dense = src.percent_dense
    g.optimizer = src.optimizer
    return g


def snapshot(g, prefix, out):
    for name, attr in PARAMS:
        p = getattr(g, attr)
        out[f"{prefix}{attr}"] = p.detach().numpy().copy()
        st = g.optimizer.state[p]
        out[f"{prefix}_{name}_exp_avg"] = st["exp_avg"].numpy().copy()
        out[f"{prefix}_{name}_exp_avg_sq"] = st["exp_avg_sq"].numpy().copy()
        out[f"{prefix}_{name}_step"] = np.float32(float(st["step"]))
    for name in STATS:
        out[f"{prefix}_{name}"] = getattr(g, name).numpy().copy()


class recorded_normal:
    """torch.normal drawing its standard normals from a seeded CPU generator and recording them"""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.z = []

    def __enter__(self):
        self.saved = torch.normal

        def normal(mean, std, *a, **k):
            z = torch.randn(std.shape, generator=self.gen)
            self.z.append(z)
            return z * std + mean
        torch.normal = normal
        return self

    def __exit__(self, *exc):
        torch.normal = self.saved
        return False


def main():
    GM = reference_class()
    out = {k: np.float64(v) for k, v in CASE.items()}
    snapshot(fresh(GM), "in", out)
    for case, mss in (("dp_none", None), ("dp_screen", 20)):
        g = fresh(GM)
        with make_golden._cuda_is_cpu(), recorded_normal(11) as rec:
            g.densify_and_prune(CASE["max_grad"], CASE["min_opacity"], CASE["extent"], mss)
        assert len(rec.z) == 1
        out[f"{case}_z"] = rec.z[0].numpy()
        snapshot(g, case, out)
    g = fresh(GM)
    mask = torch.rand(CASE["P"], generator=torch.Generator().manual_seed(3)) < 0.3
    out["prune_mask"] = mask.numpy()
    with make_golden._cuda_is_cpu():
        g.prune_points(mask)
    snapshot(g, "prune", out)
    g = fresh(GM)
    with make_golden._cuda_is_cpu():
        g.reset_opacity()
    snapshot(g, "reset", out)
    path = os.path.join(HERE, "ref_densify_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; rows:",
          {c: out[f"{c}_xyz"].shape[0] for c in ("in", "dp_none", "dp_screen", "prune")})


if __name__ == "__main__":
    main()
