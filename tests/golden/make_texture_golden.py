"""Writes ref_texture_pins.npz: what the reference's own texture-bake stages give, on the CPU, for the inputs of
tests/texture_reference.py.  Nothing of the reference is re-typed: gui/grid_put.py (pure torch) and gui/cam_utils.py are
imported from the reference checkout (cam_utils imports trimesh at the top and orbit_camera does not use it: an empty stub is
registered in sys.modules), the dilation, erosion and nearest-neighbour search are scipy's and sklearn's, called as
gui/main.py:730-749 calls them.  Only inputs' names and outputs are recorded:

    put<N>_result [64, 64, 3], put<N>_count [64, 64]     mipmap_linear_grid_put_2d(64, 64, coords[valid], values[valid],
                                                         min_resolution=16, return_count=True), N in 0, 1, 5000 (CPU scatter_add_
                                                         is sequential)
    lin<N>_<size>_result / _count                        linear_grid_put_2d(size, size, ..., return_count=True), size 64 and 32
    fill_<mask>_region bool [96, 96]                     binary_dilation(mask, iterations=32) minus mask
    fill_<mask>_inpaint int32 [K, 2]                     np.nonzero(region) stacked: the order of the next two
    fill_<mask>_nearest int32 [K, 2]                     the search-band texel sklearn's kd-tree returned
    fill_<mask>_d2 int64 [K]                             its squared distance
    fill_<mask>_ties bool [K]                            more than one search-band texel at that distance
    orbit_poses float32 [26, 4, 4]                       orbit_camera(ver, hor, 2) for the 26 views of gui/main.py:632-633

    python tests/golden/make_texture_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from tests import texture_reference as ref  # noqa: E402

REF = os.environ.get("GOI_REFERENCE", make_golden.REF)
VERS = [0] * 8 + [-45] * 8 + [45] * 8 + [-89.9, 89.9]
HORS = [0, 45, -45, 90, -90, 135, -135, 180] * 3 + [0, 0]


def reference_module(relpath, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from scipy.ndimage import binary_dilation, binary_erosion
    from sklearn.neighbors import NearestNeighbors
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    grid_put = reference_module("gui/grid_put.py", "ref_grid_put")
    cam_utils = reference_module("gui/cam_utils.py", "ref_cam_utils")
    out = {}
    for N in ref.PUT_SIZES:
        coords, values, valid = ref.put_case(N)
        co, va = torch.from_numpy(coords[valid].copy()), torch.from_numpy(values[valid].copy())
        with torch.no_grad():
            res, cnt = grid_put.mipmap_linear_grid_put_2d(ref.PUT_H, ref.PUT_W, co, va, min_resolution=ref.PUT_MIN_RESOLUTION,
                                                          return_count=True)
            out[f"put{N}_result"], out[f"put{N}_count"] = res.numpy(), cnt.numpy()[..., 0]
            for size in (64, 32):
                res, cnt = grid_put.linear_grid_put_2d(size, size, co, va, return_count=True)
                out[f"lin{N}_{size}_result"], out[f"lin{N}_{size}_count"] = res.numpy(), cnt.numpy()[..., 0]
    for name, mask in ref.fill_masks().items():
        mask = mask.copy()
        # gui/main.py:734-746
        inpaint_region = binary_dilation(mask, iterations=ref.FILL_RADIUS)
        inpaint_region[mask] = 0
        search_region = mask.copy()
        not_search_region = binary_erosion(search_region, iterations=3)
        search_region[not_search_region] = 0
        search_coords = np.stack(np.nonzero(search_region), axis=-1)
        inpaint_coords = np.stack(np.nonzero(inpaint_region), axis=-1)
        out[f"fill_{name}_region"] = inpaint_region
        out[f"fill_{name}_inpaint"] = inpaint_coords.astype(np.int32)
        if len(inpaint_coords) and len(search_coords):
            knn = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(search_coords)
            _, indices = knn.kneighbors(inpaint_coords)
            near = search_coords[indices[:, 0]]
            d2 = ((near - inpaint_coords).astype(np.int64) ** 2).sum(axis=1)
            all_d2 = ((inpaint_coords[:, None, :] - search_coords[None, :, :]).astype(np.int64) ** 2).sum(axis=2)
            assert np.array_equal(all_d2.min(axis=1), d2)
            ties = (all_d2 == d2[:, None]).sum(axis=1) > 1
        else:
            near, d2, ties = np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
        out[f"fill_{name}_nearest"], out[f"fill_{name}_d2"], out[f"fill_{name}_ties"] = near.astype(np.int32), d2, ties
        print(name, "inpaint", len(inpaint_coords), "ties %.1f %%" % (100.0 * ties.mean() if len(ties) else 0.0))
    out["orbit_poses"] = np.stack([cam_utils.orbit_camera(v, h, 2) for v, h in zip(VERS, HORS)]).astype(np.float32)
    path = os.path.join(HERE, "ref_texture_pins.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
