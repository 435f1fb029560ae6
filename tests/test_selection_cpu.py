"""CPU-only checks of the in-place selection's surface (no GPU, no compute calls): the two forward entries declare, export and
mirror in the ctypes table the selection pair (const uint8_t* keep, int invert) in front of the stream; the ABI version is the
same in the header, the loader, the library and the compiled binding; the selection argument of GaussianRasterizer.forward is
checked by the project's rules (wrong dtype: TypeError, wrong length or not contiguous: ValueError, a CPU tensor: RuntimeError --
never converted, never copied); and in_place=True without a mask is the plain call."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("goi_raster_forward", "goi_raster_forward_async")
# ABI 9 folded these into ENTRIES, goi_raster_ticket_result and goi_raster_backward
REMOVED = ("goi_raster_forward_selected", "goi_raster_forward_async_selected", "goi_raster_forward_async_cut",
           "goi_raster_ticket_result2", "goi_raster_backward2", "goi_raster_backward3", "goi_raster_backward4")


@pytest.fixture(scope="module")
def lib():
    from goi_hyperplane_amd import build
    build.build()
    from goi_hyperplane_amd import _lib
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "goi_raster.h")).read()


def test_header_declares_the_selection_of_both_forwards():
    hdr = _header()
    for name in ENTRIES:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, name
        args = [" ".join(a.split()) for a in decl.group(1).split(",")]
        # (const uint8_t* keep, int invert) immediately in front of the stream
        assert args[-3:] == ["const uint8_t* keep", "int invert", "void* stream"], name
    for name in REMOVED:
        assert not re.search(r"\b%s\s*\(" % name, hdr), name


def test_ctypes_table_has_their_signatures_and_the_library_exports_them(lib):
    from goi_hyperplane_amd import _lib
    for name in ENTRIES:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[-3:] == [C.c_void_p, C.c_int, C.c_void_p], name
        assert getattr(lib, name).argtypes == args
    for name in REMOVED:
        assert name not in _lib.SYMBOLS and not hasattr(lib, name), name


def test_abi_version_is_consistent(lib):
    from goi_hyperplane_amd import _C, _lib
    version = int(re.search(r"#define GOI_RASTER_ABI_VERSION (\d+)", _header()).group(1))
    assert version == 9
    line9 = re.search(r"/\* 9: (.*?)\n \* 8: ", _header(), re.S)
    assert line9 and all(re.search(r"\b%s\b" % name, line9.group(1)) for name in REMOVED)
    assert _lib.ABI_VERSION == version == lib.goi_raster_abi_version()
    _C.set_binding("compiled")
    ext = _C._ext()
    assert ext.abi_version() == version == ext.library_abi_version()
    for name in ("rasterize_gaussians_selected", "rasterize_gaussians_async_selected"):
        assert callable(getattr(ext, name)), name
    assert callable(_C.rasterize_gaussians_selected)


def _rasterizer(P=4):
    from goi_hyperplane_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    z = torch.zeros
    rs = GaussianRasterizationSettings(32, 32, 0.5, 0.5, z(3), 1.0, torch.eye(4), torch.eye(4), 3, z(3), False, False)
    m = z(P, 3)
    kw = dict(colors_precomp=z(P, 3), scales=z(P, 3), rotations=z(P, 4), semantics=z(P, 10))
    return GaussianRasterizer(rs), (m, m, z(P, 1)), kw


def test_selection_errors():
    r, args, kw = _rasterizer(4)
    for bad in (torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), [True] * 4):
        with pytest.raises(TypeError, match="selection must be a torch.bool or torch.uint8"):
            r(*args, selection=bad, **kw)
    for dtype in (torch.bool, torch.uint8):
        with pytest.raises(ValueError, match="selection has 5 elements, the model 4 Gaussians"):
            r(*args, selection=torch.zeros(5, dtype=dtype), **kw)
        with pytest.raises(ValueError, match="selection must be contiguous"):
            r(*args, selection=torch.zeros(8, dtype=dtype)[::2], **kw)
        # a CPU tensor is refused, not moved: the package has no CPU path
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            r(*args, selection=torch.ones(4, dtype=dtype), selection_invert=True, **kw)
    # the selection is keyword-only: the reference's positional call is what it was
    with pytest.raises(TypeError):
        r(*args, None, None, None, None, None, None, torch.ones(4, dtype=torch.bool))
    # ... and without one the call goes where it always went (here: the loud refusal of CPU operands)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(*args, selection=None, **kw)


def test_raw_operator_checks_the_selection_too():
    from goi_hyperplane_amd import _C
    z = torch.zeros
    args = (z(3), z(4, 3), z(4, 3), z(4, 10), z(4, 1), z(4, 3), z(4, 4), 1.0, torch.Tensor([]), torch.eye(4), torch.eye(4), 0.5,
            0.5, 32, 32, torch.Tensor([]), 3, z(3), False, False)
    with pytest.raises(TypeError, match="selection must be"):
        _C.rasterize_gaussians_selected(*args, z(4), False)
    with pytest.raises(ValueError, match="selection has 3 elements"):
        _C.rasterize_gaussians_selected(*args, z(3, dtype=torch.bool), False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _C.rasterize_gaussians_selected(*args, z(4, dtype=torch.bool), False)


def test_in_place_without_a_mask_is_the_plain_call(monkeypatch):
    from goi_hyperplane_amd import _C
    from goi_hyperplane_amd.render import GaussianSet, PipelineParams, TorchCamera, render, render_gui
    from goi_hyperplane_amd.scene import make_camera, make_scene
    P, S, W, H = 12, 10, 32, 16
    calls = []

    def plain(*args):
        assert len(args) == 20
        calls.append(args)
        z = torch.zeros
        return (0, z(3, H, W), z(S, H, W), z(1, H, W), z(1, H, W), z(P, dtype=torch.int32), z(0, dtype=torch.uint8),
                z(0, dtype=torch.uint8), z(0, dtype=torch.uint8))

    def selected(*_args):
        raise AssertionError("no mask: the selected operator must not be called")

    monkeypatch.setattr(_C, "rasterize_gaussians", plain)
    monkeypatch.setattr(_C, "rasterize_gaussians_selected", selected)
    dev = torch.device("cpu")
    pc = GaussianSet.from_scene(make_scene(P, S=S, seed=1), dev)
    cam = TorchCamera(make_camera(W, H), dev)
    bg = torch.zeros(3)
    for kw in (dict(in_place=True), dict(in_place=True, mask_invert=True), dict(mask_invert=True), {}):
        out = render(cam, pc, PipelineParams(), bg, **kw)
        assert out["radii"].shape == (P,) and out["viewspace_points"].shape == (P, 3)
    assert len(calls) == 4 and all(c[1].data_ptr() == pc.get_xyz.data_ptr() and c[1].shape[0] == P for c in calls)  # never a copy
    out = render_gui(cam, pc, bg, in_place=True)
    assert len(calls) == 5 and out["image"].shape == (3, H, W)
