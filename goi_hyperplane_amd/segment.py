"""Instance segmentation of the Gaussians on their k-NN graph (csrc/segment.hip over the C ABI).

    edges(idx, features=None, tau=inf, dist2=None, max_dist2=None, labels=None, rows=None, mutual=False) -> uint8 [P,k]
    components(idx, join=None, rows=None, min_size=1)                                   -> Segments
    instances(xyz, features, k=8, tau=..., max_dist2=None, labels=None, selection=None, mutual=False, min_size=1) -> Segments
    select(segments, seeds)                                                             -> bool [P]
    pick(camera, pc, bg_color, xy, segments, **kw)                                      -> bool [P]

WHICH GAUSSIANS ARE THIS OBJECT?  Two objects that touch are one cluster of positions (cluster.dbscan), but their learned
features differ -- and smooth.loss makes those features consistent inside an object.  So: keep the edges of `knn.graph` whose
two rows agree (`edges`), and take the connected components of what is left (`components`).  That is a 3D instance decomposition
of the whole model, or of a selection, without a prompt and without a render; a click is then one table look-up (`pick`).

`edges`: with j = idx[i,m], join[i,m] = 1 iff 0 <= j < P and j != i (-1 tails, ids out of range and self edges never join), and
rows[i] and rows[j], and labels[i] >= 0 and labels[i] == labels[j], and dist2[i,m] <= max_dist2, and d <= tau with

    d = 0;  for c = 0 .. S-1:  e = f[i,c] - f[j,c];  d = fmaf(e, e, d)          (fp32, in that order)

and, with `mutual`, i is in row j's list as well -- every clause only where its argument is given.  d is the squared Euclidean
distance of the two feature rows.  For a COSINE gate pass rows normalised to unit length: |a - b|^2 = 2 - 2 cos(a, b), so
cos >= c is tau = 2 - 2 c.  A NaN d never joins; tau = +inf joins every other d.

`components`: the graph is taken as UNDIRECTED -- an edge that only one endpoint lists unites both.  root[i] is the smallest id
of row i's component, size[i] its number of rows, label[i] the dense rank (ascending root) of the component among those with
size >= min_size and -1 for a dropped one, count the number of kept components.  A row with rows[i] == 0 is in no component
(root -1, size 0, label -1) and every edge that touches it is ignored.  All integers, independent of the schedule.

Tensors on a ROCm GPU only; there is no CPU fallback.  Nothing here synchronises the host: count and status stay on the device.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib, contrib, knn
from ._lib import check, ptr, stream

_NO_CPU = "goi_hyperplane_amd.segment: tensors must live on a ROCm GPU; there is no CPU fallback"
S_MAX = 32             # goi_knn_segment_edges: 1 <= S <= 32
MAX_ENTRIES = 2 ** 30  # P * k below this
MUTUAL, MAX_DIST2 = 1, 2  # GOI_SEGMENT_* flags of include/goi_raster.h
STATUS_UNION = 4          # GOI_SEGMENT_STATUS_UNION


class Segments(NamedTuple):
    """What components() returns, all on the device: label / root / size int32 [P], count int32 [1] (the number of kept
    components), status int32 [1] (GOI_SEGMENT_STATUS_* bits, 0 after a good call: look at it where the results are read back).
    graph: None, or from instances() the (idx, dist2, join) it built, for reuse."""
    label: torch.Tensor
    root: torch.Tensor
    size: torch.Tensor
    count: torch.Tensor
    status: torch.Tensor
    graph: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None


def _tensor(t, who, what, dtypes):
    """a tensor of one of `dtypes`; where it lives is looked at last (_on_gpu), so that a wrong dtype or shape is named as such"""
    if not torch.is_tensor(t):
        raise TypeError(f"segment.{who}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"segment.{who}: {what} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
    return t


def _on_gpu(who, **tensors):
    """every given tensor on ONE ROCm GPU (None: not given)"""
    given = {name: t for name, t in tensors.items() if t is not None}
    if any(not t.is_cuda for t in given.values()):
        raise RuntimeError(_NO_CPU)
    first = next(iter(given.values())).device
    for name, t in given.items():
        if t.device != first:
            raise ValueError(f"segment.{who}: {name} is on {t.device}, expected {first}")


def _idx(idx, who):
    """int32 [P,k], k >= 1, P * k < 2^30, contiguous"""
    idx = _tensor(idx, who, "idx", (torch.int32,))
    if idx.dim() != 2 or idx.shape[1] < 1:
        raise ValueError(f"segment.{who}: idx must have shape (P, k) with k >= 1")
    if idx.shape[0] * idx.shape[1] >= MAX_ENTRIES:
        raise ValueError(f"segment.{who}: need P * k < 2^30")
    return idx.contiguous()


def _bytes(m, P, who, what):
    """bool (or uint8) [P] -> contiguous uint8 (a view of a contiguous bool: no copy); None stays None"""
    if m is None:
        return None
    m = _tensor(m, who, what, (torch.bool, torch.uint8))
    if tuple(m.shape) != (P,):
        raise ValueError(f"segment.{who}: {what} must have shape ({P},)")
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def edges(idx, features=None, tau=math.inf, dist2=None, max_dist2=None, labels=None, rows=None, mutual=False):
    """-> uint8 [P,k]: 1 where entry (i, m) of the graph joins its two rows (module docstring).  idx int32 [P,k]; features
    float32 [P,S], 1 <= S <= 32 (absent: no feature gate; normalise the rows for a cosine gate); tau: the largest squared feature
    distance that joins; dist2 float32 [P,k] with max_dist2: the largest squared distance that joins (max_dist2 needs dist2; dist2
    alone cuts nothing); labels int64 [P]: only rows of one label >= 0 join; rows bool [P]: only rows inside join; mutual: only
    edges that both endpoints list.  The same bits on every call.  Asynchronous, no read-back."""
    idx = _idx(idx, "edges")
    P, k = int(idx.shape[0]), int(idx.shape[1])
    S = 1
    if features is not None:
        features = _tensor(features, "edges", "features", (torch.float32,))
        if features.dim() != 2 or features.shape[0] != P or not 1 <= features.shape[1] <= S_MAX:
            raise ValueError(f"segment.edges: features must have shape ({P}, S) with 1 <= S <= {S_MAX}")
        features = features.detach().contiguous()
        S = int(features.shape[1])
    tau = float(tau)
    if math.isnan(tau):
        raise ValueError("segment.edges: tau is NaN")
    if dist2 is not None:
        dist2 = _tensor(dist2, "edges", "dist2", (torch.float32,))
        if dist2.shape != idx.shape:
            raise ValueError(f"segment.edges: dist2 must have idx's shape {tuple(idx.shape)}")
        dist2 = dist2.detach().contiguous()
    flags = MUTUAL if mutual else 0
    if max_dist2 is not None:
        if dist2 is None:
            raise ValueError("segment.edges: max_dist2 needs dist2")
        max_dist2 = float(max_dist2)
        if math.isnan(max_dist2):
            raise ValueError("segment.edges: max_dist2 is NaN")
        flags |= MAX_DIST2
    if labels is not None:
        labels = _tensor(labels, "edges", "labels", (torch.int64,))
        if tuple(labels.shape) != (P,):
            raise ValueError(f"segment.edges: labels must have shape ({P},)")
        labels = labels.contiguous()
    rows = _bytes(rows, P, "edges", "rows")
    _on_gpu("edges", idx=idx, features=features, dist2=dist2, labels=labels, rows=rows)
    lib = _lib.load()
    dev = idx.device
    with torch.cuda.device(dev):
        join = torch.empty((P, k), dtype=torch.uint8, device=dev)
        check(lib.goi_knn_segment_edges(P, S, k, ptr(idx), ptr(features), tau, ptr(dist2), max_dist2 if max_dist2 is not None else 0.0,
                                        flags, ptr(labels), ptr(rows), ptr(join), stream(dev)))
    return join


def components(idx, join=None, rows=None, min_size=1):
    """-> Segments(label, root, size, count, status): the connected components of the undirected graph of the joining edges
    (module docstring).  join uint8 or bool [P,k] as edges() returns it (absent: every valid edge that is not a self edge joins);
    rows bool [P]: the rows that take part; min_size >= 1: smaller components get label -1 and are not counted.  Asynchronous,
    no read-back."""
    idx = _idx(idx, "components")
    P, k = int(idx.shape[0]), int(idx.shape[1])
    if join is not None:
        join = _tensor(join, "components", "join", (torch.uint8, torch.bool))
        if join.shape != idx.shape:
            raise ValueError(f"segment.components: join must have idx's shape {tuple(idx.shape)}")
        join = join.contiguous()
        join = join.view(torch.uint8) if join.dtype == torch.bool else join
    rows = _bytes(rows, P, "components", "rows")
    if isinstance(min_size, bool) or not isinstance(min_size, int):
        raise TypeError("segment.components: min_size must be an int")
    if not 1 <= min_size < 2 ** 31:
        raise ValueError("segment.components: need 1 <= min_size < 2^31")
    _on_gpu("components", idx=idx, join=join, rows=rows)
    lib = _lib.load()
    dev = idx.device
    with torch.cuda.device(dev):
        out = torch.empty((3, P), dtype=torch.int32, device=dev)
        word = torch.zeros((2,), dtype=torch.int32, device=dev)  # count, status (an empty graph: 0 components, status 0)
        ws = _lib.workspace(lib.goi_knn_segment_components_workspace_bytes(P, k), dev)
        check(lib.goi_knn_segment_components(P, k, ptr(idx), ptr(join), ptr(rows), min_size, ptr(out[1]), ptr(out[2]), ptr(out[0]),
                                             ptr(word[0:1]), ptr(word[1:2]), ptr(ws), stream(dev)))
    return Segments(out[0], out[1], out[2], word[0:1], word[1:2])


def instances(xyz, features, k=8, tau=math.inf, max_dist2=None, labels=None, selection=None, mutual=False, min_size=1):
    """-> Segments with .graph = (idx, dist2, join): the instances of a model (or of `selection`, bool [P]) in three calls,

        idx, dist2 = knn.graph(xyz, k, selection)
        join = edges(idx, features, tau, dist2, max_dist2, labels, rows=selection, mutual=mutual)
        components(idx, join, rows=selection, min_size=min_size)

    e.g.  seg = segment.instances(pc.get_xyz, torch.nn.functional.normalize(pc._semantics, dim=1), tau=0.5, min_size=50).
    tau: the largest squared feature distance inside an object (features=None: positions and labels alone).  The graph is
    returned for reuse: another tau is another edges() + components() on the same idx.  A row outside the selection is in no
    component."""
    idx, dist2 = knn.graph(xyz, k, selection)
    join = edges(idx, features, tau, dist2, max_dist2, labels, selection, mutual)
    return components(idx, join, selection, min_size)._replace(graph=(idx, dist2, join))


def select(segments, seeds):
    """-> bool [P]: the rows whose label equals that of any seed.  seeds: an integer tensor of row ids on the device, any shape;
    a seed of -1 (or outside [0, P)) and a seed whose label is -1 (a dropped component, a row outside the selection) select
    nothing.  Torch glue on [P] arrays; it does not synchronise."""
    if not isinstance(segments, Segments):
        raise TypeError("segment.select: segments must be what components() or instances() returned")
    label = segments.label
    if not torch.is_tensor(seeds) or seeds.dtype not in (torch.int64, torch.int32):
        raise TypeError("segment.select: seeds must be an int64 or int32 tensor")
    _on_gpu("select", label=label, seeds=seeds)
    P = int(label.shape[0])
    if P == 0:
        return torch.zeros((0,), dtype=torch.bool, device=label.device)
    seeds = seeds.reshape(-1).to(torch.int64)
    inside = (seeds >= 0) & (seeds < P)
    seed_label = torch.where(inside, label[seeds.clamp(0, P - 1)].to(torch.int64), torch.full_like(seeds, -1))
    # a table by label (labels are below P): slot P takes the seeds that select nothing, slot P + 1 stays False for label -1
    chosen = torch.zeros((P + 2,), dtype=torch.bool, device=label.device)
    chosen.index_fill_(0, torch.where(seed_label >= 0, seed_label, torch.full_like(seed_label, P)), True)
    return chosen.index_select(0, torch.where(label >= 0, label, torch.full_like(label, P + 1)).to(torch.int64))


def pick(camera, pc, bg_color, xy, segments, **kw):
    """-> bool [P]: the instance(s) under pixel(s) xy -- select(segments, contrib.pick(camera, pc, bg_color, xy, **kw)): the
    Gaussian that dominates the pixel, grown into its object.  Nothing under the pixel selects nothing."""
    return select(segments, contrib.pick(camera, pc, bg_color, xy, **kw))
