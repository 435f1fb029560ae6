"""One exact forward of the product through the C ABI, called raw (ctypes on include/goi_raster.h, no binding in between), with
everything it filled kept: what the tests that drive the frame's other entries directly (goi_raster_backward,
goi_raster_debug_backward_blend, goi_raster_debug_views) start from."""
import ctypes as C

import numpy as np
import torch


GUARD = 64  # floats: 256 bytes, so that what lies between two guard bands keeps the allocation's alignment


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class RawFrame:
    """goi_raster_forward over the scene `sc` (goi_hyperplane_amd.scene: SH colours, scales and rotations) from `cam` on `dev`:
    the operand tensors (.t), the scene struct (.scene), the four maps and radii, the three workspaces, N = num_rendered."""

    def __init__(self, sc, cam, bg, dev):
        from goi_hyperplane_amd import _C, _lib
        self.lib = lib = _lib.load()
        P, S, W, H = sc.P, sc.S, cam.image_width, cam.image_height
        self.P, self.S, self.W, self.H, self.dev = P, S, W, H, dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.t = dict(bg=t(np.asarray(bg, np.float32)), means3D=t(sc.means3D), shs=t(sc.shs), semantics=t(sc.semantics),
                      opacity=t(sc.opacities), scales=t(sc.scales), rotations=t(sc.rotations), view=t(cam.world_view_transform),
                      proj=t(cam.full_proj_transform), campos=t(cam.camera_center))
        x = self.t
        self.scene = _C._scene(P, S, H, W, x["bg"], x["means3D"], x["shs"], None, x["semantics"], x["opacity"], x["scales"],
                               x["rotations"], 1.0, None, x["view"], x["proj"], cam.tanfovx, cam.tanfovy, sc.sh_degree, x["campos"],
                               False, False)
        f32 = dict(dtype=torch.float32, device=dev)
        # (the semantic map sits between two NaN guard bands of GUARD floats: a channel written beyond the S-th is seen)
        self.semmap_guarded = torch.full((S * H * W + 2 * GUARD,), float("nan"), **f32)
        self.color, self.semmap = torch.empty((3, H, W), **f32), self.semmap_guarded[GUARD:GUARD + S * H * W].view(S, H, W)
        self.depth, self.alpha = torch.empty((H, W), **f32), torch.empty((H, W), **f32)
        self.radii = torch.empty((P,), dtype=torch.int32, device=dev)
        self.geom = torch.empty(lib.goi_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
        self.img = torch.empty(lib.goi_raster_image_bytes(W, H), dtype=torch.uint8, device=dev)
        alloc = _C._BinningAllocator(torch.device(dev))
        n = lib.goi_raster_forward(C.byref(self.scene), ptr(self.geom), ptr(self.img), alloc.cb, None, ptr(self.color),
                                   ptr(self.semmap), ptr(self.depth), ptr(self.alpha), ptr(self.radii), None, 0, None)
        if alloc.error is not None:
            raise alloc.error
        assert n >= 0, _lib.last_error()
        self.N, self.binning = int(n), alloc.tensor
        torch.cuda.synchronize()

    def views(self):
        """goi_raster_debug_views of the frame (N > 0) -> dict of device tensors"""
        from goi_hyperplane_amd import _C
        return _C.debug_views(self.P, self.W, self.H, self.N, self.geom, self.binning, self.img)
