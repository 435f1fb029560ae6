"""MI355X-native differentiable Gaussian rasterizer with a semantic-feature channel."""
import importlib

__all__ = ["grouping", "instance", "pose", "segment", "smooth"]


def __getattr__(name):
    """`goi_hyperplane_amd.grouping` / `.instance` / `.pose` / `.segment` / `.smooth` without an import of their own; loaded on first use, so importing the package stays
    free."""
    if name in __all__:
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
