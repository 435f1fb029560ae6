"""A PCA picture of the semantic features on the device (csrc/pca.hip): the three principal components of the
S-dimensional feature field as a colour.  The reference computes it on the host on every call (gui/main_edit.py:1841-1870
visual_latent, utils/visual_latent.py:32-40: the rendered [S, H, W] map copied to the host, sklearn's
PCA(n_components=3).fit_transform on its HW x S rows, and q * 255 written as uint8 with no normalisation).

    fit, fit_views, fit_gaussians   a PcaBasis: sklearn.decomposition.PCA(3)'s mean_, components_ and
                                    explained_variance_ (covariance with divisor n - 1, descending order, the entry of
                                    largest magnitude of each component positive: sklearn >= 1.5)
    transform                       q = (x - mean) . components, raw (what fit_transform returns) or normalised for display
    gaussian_colors                 the Gaussians' own features as [P, 3] colours for render(..., override_color=...)

A basis fitted once (on the Gaussians' features, or over a camera set) gives every frame of an orbit the same colours; a
basis fitted per frame flickers.  Samples come as "planar" [S, ...] (a rendered map, read in place) or "rows" [n, S].

Normalisations of transform (float32, one rounding per operation; tests/pca_reference.py restates them in numpy):

    "raw"     q
    "sigma"   clamp(0.5 + q / ((2 k) * max(sqrt(explained_variance), FLT_MIN)), 0, 1), k = k_sigma.  The scale belongs to the
              basis, not the frame, so colours are stable over a video.  k = 2 (+-2 sigma span the range) is a display
              choice: larger is greyer, smaller saturates more pixels.
    "minmax"  (q - min) / ((max - min) + f32(1e-20)) per view and component, NaNs skipped: test_step's depth
              normalisation (gui/main.py:569)

The moments are accumulated about a pivot (the mean of the used samples among 2048 spread over the first sample set)
and corrected exactly in the solve, so features far from zero lose nothing.  Everything runs on the current stream, nothing is read back, there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, ptr, stream

# GOI_PCA_* of include/goi_raster.h
PLANAR, ROWS = 0, 1
LAYOUTS = {"planar": PLANAR, "rows": ROWS}
RAW, SIGMA, MINMAX = 0, 1, 2
NORMALIZATIONS = {"raw": RAW, "sigma": SIGMA, "minmax": MINMAX}
MIN_DIM, MAX_DIM = 3, 32
_NO_CPU = "goi_hyperplane_amd.pca: tensors must live on a ROCm GPU; there is no CPU fallback"


def basis_floats(S: int) -> int:
    """GOI_PCA_BASIS_FLOATS(S)"""
    return 4 * S + 5


class PcaBasis:
    """A view over the device basis `data` (float32 [4 S + 5]): mean [S], components [3, S], explained_variance [3],
    total_variance and count (0-d tensors; count is rounded to float32).  Nothing is copied or read back."""

    def __init__(self, data: torch.Tensor, S: int):
        if data.dtype != torch.float32 or data.dim() != 1 or int(data.numel()) != basis_floats(S) or not data.is_contiguous():
            raise ValueError(f"PcaBasis: data must be a contiguous float32 [{basis_floats(S)}] tensor for S = {S}")
        self.data, self.S = data, int(S)

    @property
    def mean(self):
        return self.data[:self.S]

    @property
    def components(self):
        return self.data[self.S:4 * self.S].view(3, self.S)

    @property
    def explained_variance(self):
        return self.data[4 * self.S:4 * self.S + 3]

    @property
    def total_variance(self):
        return self.data[4 * self.S + 3]

    @property
    def count(self):
        return self.data[4 * self.S + 4]


def _layout(layout) -> int:
    if layout not in LAYOUTS:
        raise ValueError(f"pca: unknown layout {layout!r}; expected one of {sorted(LAYOUTS)}")
    return LAYOUTS[layout]


def _samples(fn, x, code):
    """(S, n) of a sample tensor; raises for anything the kernels do not take."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{fn}: x must be a tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(f"{fn}: x must be float32, got {x.dtype}")
    if x.dim() < 2:
        raise ValueError(f"{fn}: x must be [S, ...] (planar) or [n, S] (rows), got shape {tuple(x.shape)}")
    if code == ROWS and x.dim() != 2:
        raise ValueError(f"{fn}: rows are [n, S], got shape {tuple(x.shape)}")
    S = int(x.shape[1] if code == ROWS else x.shape[0])
    n = int(x.numel()) // max(S, 1)
    if not MIN_DIM <= S <= MAX_DIM:
        raise ValueError(f"{fn}: need {MIN_DIM} <= S <= {MAX_DIM} feature channels, got {S}")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{fn}: need 1 <= n < 2^31 samples, got {n}")
    return S, n


def _mask(fn, mask, n, dev):
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{fn}: mask must be a bool or uint8 tensor")
    if int(mask.numel()) != n:
        raise ValueError(f"{fn}: mask has {int(mask.numel())} elements, the {n} samples need {n}")
    if not mask.is_cuda:
        raise RuntimeError(_NO_CPU)
    if mask.device != dev:
        raise ValueError(f"{fn}: all tensors must live on one device")
    m = mask.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


class Fit:
    """One fit in progress: add(x, ...) accumulates a sample set into the device workspace (first call: it also fixes the
    pivot), solve() gives the PcaBasis of everything added.  This is how a camera set is fitted without keeping a map."""

    def __init__(self, S: int, device):
        if not MIN_DIM <= S <= MAX_DIM:
            raise ValueError(f"pca.Fit: need {MIN_DIM} <= S <= {MAX_DIM} feature channels, got {S}")
        self.S, self.device = int(S), torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        self._lib = _lib.load()
        # the caching allocator hands out 512-byte aligned blocks: the workspace's 256 bytes hold
        self.workspace = torch.empty(int(self._lib.goi_semantic_pca_workspace_bytes(self.S, 0)), dtype=torch.uint8,
                                     device=self.device)
        self.calls = 0

    def reset(self) -> "Fit":
        """Start another fit in the same workspace: the next add overwrites what it holds."""
        self.calls = 0
        return self

    def add(self, x: torch.Tensor, layout="planar", mask=None) -> "Fit":
        code = _layout(layout)
        S, n = _samples("pca.fit", x, code)
        if S != self.S:
            raise ValueError(f"pca.fit: this fit has {self.S} channels, x has {S}")
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        if x.device != self.device:
            raise ValueError("pca.fit: all tensors must live on one device")
        m = _mask("pca.fit", mask, n, self.device)
        src = x.contiguous()
        with torch.cuda.device(self.device):
            check(self._lib.goi_semantic_pca_accumulate(ptr(src), code, S, n, ptr(m), 1 if self.calls == 0 else 0,
                                                        ptr(self.workspace), stream(self.device)))
        self.calls += 1
        return self

    def solve(self) -> PcaBasis:
        if self.calls == 0:
            raise ValueError("pca.fit: nothing was added")
        data = torch.empty(basis_floats(self.S), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self._lib.goi_semantic_pca_solve(self.S, ptr(self.workspace), ptr(data), stream(self.device)))
        return PcaBasis(data, self.S)


def _check_fit(fn, x, layout, mask):
    code = _layout(layout)
    S, n = _samples(fn, x, code)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"{fn}: mask must be a bool or uint8 tensor")
        if int(mask.numel()) != n:
            raise ValueError(f"{fn}: mask has {int(mask.numel())} elements, the {n} samples need {n}")
    if not x.is_cuda or (mask is not None and not mask.is_cuda):
        raise RuntimeError(_NO_CPU)
    return S


def fit(x: torch.Tensor, layout="planar", mask: torch.Tensor | None = None) -> PcaBasis:
    """The basis of x's samples: float32 [S, ...] ("planar": a rendered [S, H, W] map) or [n, S] ("rows"), 3 <= S <= 32.
    mask: bool / uint8 with one element per sample, nonzero = use it (fit a frame on alpha > t, or on the decoded
    foreground, so that an empty background does not own the first component); samples that are not used may hold
    anything.  With fewer than two used samples the components and variances are zero and `count` says so."""
    S = _check_fit("pca.fit", x, layout, mask)
    return Fit(S, x.device).add(x, layout, mask).solve()


def fit_views(maps, masks=None) -> PcaBasis:
    """ONE basis over several [S, H, W] maps (they may differ in size), as if their samples were concatenated: every map
    is accumulated into the same workspace and none is kept.  masks: None, or one mask (or None) per map.  The sums are
    exact for any number of views; only the basis's `count` is a float32 and rounds above 2^24 samples (ten 1600 x 1056
    maps).  Nothing computed depends on it."""
    maps = list(maps)
    if not maps:
        raise ValueError("pca.fit_views: no maps")
    masks = [None] * len(maps) if masks is None else list(masks)
    if len(masks) != len(maps):
        raise ValueError(f"pca.fit_views: {len(maps)} maps but {len(masks)} masks")
    S = [_samples("pca.fit_views", x, PLANAR)[0] for x in maps]
    if any(s != S[0] for s in S):
        raise ValueError(f"pca.fit_views: the maps differ in their channel count: {S}")
    for x, m in zip(maps, masks):
        _check_fit("pca.fit_views", x, "planar", m)
    f = Fit(S[0], maps[0].device)
    for x, m in zip(maps, masks):
        f.add(x, "planar", m)
    return f.solve()


def fit_gaussians(pc) -> PcaBasis:
    """The basis of the Gaussians' own features pc.get_semantics [P, S]: view-independent, so every frame projected with
    it has the same colours."""
    return fit(pc.get_semantics.detach(), layout="rows")


def transform(x: torch.Tensor, basis: PcaBasis, layout="planar", normalize="raw", k_sigma: float = 2.0,
              out: torch.Tensor | None = None, out_layout=None) -> torch.Tensor:
    """q = (x - mean) . components for every sample.  "planar" x [S, H, W] -> [3, H, W] (a `base` of display.compose),
    [V, S, H, W] -> [V, 3, H, W] (every view its own minimum and maximum under "minmax"), [S, n] -> [3, n]; "rows" x
    [n, S] -> [n, 3] (a colors_precomp).  out_layout ("planar" / "rows", default: as the input) picks the other output
    layout: [..., H, W, 3] / [n, 3] from planar samples, [3, n] from rows; the values are the same bits.  normalize and
    k_sigma: see the module docstring.  out: a contiguous float32 tensor of the result's shape to write into."""
    code = _layout(layout)
    ocode = code if out_layout is None else _layout(out_layout)
    if normalize not in NORMALIZATIONS:
        raise ValueError(f"pca.transform: unknown normalize {normalize!r}; expected one of {sorted(NORMALIZATIONS)}")
    mode = NORMALIZATIONS[normalize]
    if not isinstance(basis, PcaBasis):
        raise TypeError(f"pca.transform: basis must be a PcaBasis, got {type(basis).__name__}")
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"pca.transform: x must be a tensor, got {type(x).__name__}")
    V, batched = 1, False
    if code == PLANAR and x.dim() == 4:
        V, batched = int(x.shape[0]), True
        if not 1 <= V <= 65535:
            raise ValueError(f"pca.transform: need 1 <= V <= 65535 views, got {V}")
        S, n = _samples("pca.transform", x[0], code)
        spatial = tuple(x.shape[2:])
    else:
        S, n = _samples("pca.transform", x, code)
        spatial = tuple(x.shape[1:]) if code == PLANAR else (n,)
    if S != basis.S:
        raise ValueError(f"pca.transform: the basis has {basis.S} channels, x has {S}")
    k = float(k_sigma)
    if mode == SIGMA and not (0.0 < k <= 3.0e38):
        raise ValueError(f"pca.transform: k_sigma must be finite and > 0, got {k_sigma!r}")
    shape = ((3,) + spatial) if ocode == PLANAR else (spatial + (3,))
    if batched:
        shape = (V,) + shape
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float32
                            or not out.is_contiguous()):
        raise ValueError(f"pca.transform: out must be a contiguous float32 tensor of shape {shape}")
    used = [x, basis.data] + ([out] if out is not None else [])
    if not all(t.is_cuda for t in used):
        raise RuntimeError(_NO_CPU)
    dev = x.device
    if any(t.device != dev for t in used):
        raise ValueError("pca.transform: all tensors must live on one device")

    lib = _lib.load()
    src = x.contiguous()
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    ws = torch.empty((V, 3, 2), dtype=torch.int32, device=dev) if mode == MINMAX else None
    with torch.cuda.device(dev):
        check(lib.goi_semantic_pca_apply(ptr(src), code, S, n, V, ptr(basis.data), mode, k, ptr(out), ocode, ptr(ws),
                                         stream(dev)))
    return out


def gaussian_colors(pc, basis: PcaBasis | None = None, normalize="sigma", k_sigma: float = 2.0) -> torch.Tensor:
    """[P, 3] colours in [0, 1] of the Gaussians' own features, for render(..., override_color=...): the rasterizer then
    blends the PCA colours themselves.  basis None: fit_gaussians(pc).  "raw" is refused: it is not a colour."""
    if normalize == "raw":
        raise ValueError("pca.gaussian_colors: normalize must be 'sigma' or 'minmax' (raw projections are not colours)")
    sem = pc.get_semantics.detach()
    if basis is None:
        basis = fit(sem, layout="rows")
    return transform(sem, basis, layout="rows", normalize=normalize, k_sigma=k_sigma)
