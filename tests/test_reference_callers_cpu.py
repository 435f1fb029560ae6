"""The reference's own caller, replayed against this repository's drop-in package.

tests/golden/ref_caller_pins.json records, from the AST of the reference's gaussian_renderer/__init__.py (make_golden.py:
caller_pins), how its render() and trace() drive `diff_gaussian_rasterization`: the keywords of their
GaussianRasterizationSettings(...), GaussianRasterizer(...) and rasterizer(...) / rasterizer.trace(...) calls, and the attributes
they read off the camera, the model and the pipeline object.  Here those calls are made on CPU tensors with exactly the
recorded keywords, on this package's camera, model and pipeline objects: with the rasterizer's own SH and covariance paths and
with the Python-side ones (colours and cov3D precomputed).  There is no GPU in this container, so the call must bind every field
and keyword of this package's API and stop at the one place this package refuses: "no CPU fallback".  Any mismatch in names or
keywords raises something else (AttributeError, TypeError, KeyError) first."""
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ref_caller_pins.json")) as _fh:
    PINS = json.load(_fh)


def _replay(fn, python_paths=False):
    import diff_gaussian_rasterization as dgr
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera
    from goi_hyperplane_amd.scene import make_camera, make_scene
    pins = PINS[fn]
    pc = GaussianSet.from_scene(make_scene(50, S=10, seed=0), torch.device("cpu"))
    cam = TorchCamera(make_camera(64, 48), torch.device("cpu"))
    pipe = PipelineParams()
    pipe.convert_SHs_python = pipe.compute_cov3D_python = python_paths
    for obj, name in ((cam, "viewpoint_camera"), (pc, "pc"), (pipe, "pipe")):
        missing = [a for a in pins["reads"][name] if not hasattr(obj, a)]
        assert not missing, (name, missing)
    settings = {"image_height": int(cam.image_height), "image_width": int(cam.image_width),
                "tanfovx": math.tan(cam.FoVx * 0.5), "tanfovy": math.tan(cam.FoVy * 0.5), "bg": torch.zeros(3),
                "scale_modifier": 1.0, "viewmatrix": cam.world_view_transform, "projmatrix": cam.full_proj_transform,
                "sh_degree": pc.active_sh_degree, "campos": cam.camera_center, "prefiltered": False, "debug": pipe.debug}
    rs = dgr.GaussianRasterizationSettings(**{k: settings[k] for k in pins["calls"]["GaussianRasterizationSettings"]})
    rasterizer = dgr.GaussianRasterizer(**{k: rs for k in pins["calls"]["GaussianRasterizer"]})
    xyz = pc.get_xyz
    values = {"means3D": xyz, "means2D": torch.zeros_like(xyz, requires_grad=True) + 0, "opacities": pc.get_opacity,
              "shs": None if python_paths else pc.get_features,
              "colors_precomp": torch.full_like(xyz, 0.5) if python_paths else None,
              "scales": None if python_paths else pc.get_scaling, "rotations": None if python_paths else pc.get_rotation,
              "cov3D_precomp": pc.get_covariance(1.0) if python_paths else None,
              "semantics": pc.get_semantics, "img_sem": torch.zeros(10, 48, 64)}
    call, name = (rasterizer.trace, "rasterizer.trace") if fn == "trace" else (rasterizer, "rasterizer")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(**{k: values[k] for k in pins["calls"][name]})


@pytest.mark.parametrize("python_paths", [False, True])
def test_reference_render_reaches_this_packages_operator(python_paths):
    _replay("render", python_paths)


def test_reference_trace_reaches_this_packages_operator():
    _replay("trace")
