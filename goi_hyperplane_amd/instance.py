"""Per-instance statistics and whole-object selection over a partition of the Gaussians (csrc/instance.hip over the C ABI;
DESIGN.md 4.30).

    members(segments_or_label, capacity=None)                                             -> Members(ptr, rows, K)
    stats(segments_or_label, xyz, features=None, weight=None, hit=None, members=None, capacity=None) -> InstanceStats
    vote(stats, min_fraction=0.5, min_hits=1, bit=0)                                      -> bool [K]
    rows_of(segments_or_label, keep)                                                      -> bool [P]
    select(segments, hit, min_fraction=0.5, min_hits=1, capacity=None)                    -> bool [P]

WHAT IS THIS OBJECT, AND DID THE PROMPT MEAN IT?  `segment.instances` partitions the model into objects; this module reduces
per-row data over that partition.  A row is in instance label[i] iff 0 <= label[i] < K; every other label (-1: a dropped
component or a row outside the selection; a label at or above K: a capacity that was too small) is in no instance.

`members`: the partition as lists -- the rows of instance k are rows[ptr[k] : ptr[k+1]] in ascending row id, ptr[K] is the number
of rows in an instance and rows is -1 from there on.

`stats`: for every instance, in ONE pass over the lists: n, hits [K,8] (members with bit b of `hit` set: eight prompts are scored
at once; a bool tensor is bit 0), wsum W = sum w, centroid = sum w x / W, lo / hi (the exact bounding box; a NaN is skipped, an
instance without a number gets +inf / -inf), cov = sum w (x-c)(x-c)^T / W as xx xy xz yy yz zz, feature = sum w f / W.  The sums
are float64, of positions relative to the instance's first member, in an order that depends on the instance's own member list
and on nothing else (csrc/instance.hip spells it out; tests/instance_reference.py restates it in numpy): the same bits on every
call, for any K, whatever else is in the model.  W == 0 gives 0 for centroid, cov and feature.

`vote` / `rows_of` / `select`: an instance is kept when at least min_hits of its rows and at least min_fraction of them are hit
(integers only), and the kept instances are handed back as rows -- a speckled per-Gaussian mask becomes whole objects.

Tensors on a ROCm GPU only; there is no CPU fallback.  Everything stays on the device; the one read-back is `capacity=None`,
which has to read the number of instances to size the outputs -- pass an int (any upper bound does) and nothing synchronises.
"""
from __future__ import annotations

from fractions import Fraction
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream
from .segment import Segments

_NO_CPU = "goi_hyperplane_amd.instance: tensors must live on a ROCm GPU; there is no CPU fallback"
S_MAX = 32          # goi_instance_stats: 1 <= S <= 32
MAX_ROWS = 2 ** 30  # P and K below this
CHUNK = 256         # members per chunk of the summation order


class Members(NamedTuple):
    """What members() returns, on the device: ptr int32 [K+1], rows int32 [P]; K: the number of instances the lists are for."""
    ptr: torch.Tensor
    rows: torch.Tensor
    K: int


class InstanceStats(NamedTuple):
    """What stats() returns, all on the device (module docstring): n int32 [K], hits int32 [K,8], wsum [K], centroid [K,3],
    lo / hi [K,3], cov [K,6], feature [K,S] or None, and the Members it went over (for reuse)."""
    n: torch.Tensor
    hits: torch.Tensor
    wsum: torch.Tensor
    centroid: torch.Tensor
    lo: torch.Tensor
    hi: torch.Tensor
    cov: torch.Tensor
    feature: Optional[torch.Tensor]
    members: Members


def _tensor(t, who, what, dtypes):
    """a tensor of one of `dtypes`; where it lives is looked at last (_on_gpu), so that a wrong dtype or shape is named as such"""
    if not torch.is_tensor(t):
        raise TypeError(f"instance.{who}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"instance.{who}: {what} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
    return t


def _on_gpu(who, **tensors):
    """every given tensor on ONE ROCm GPU (None: not given)"""
    given = {name: t for name, t in tensors.items() if t is not None}
    if any(not t.is_cuda for t in given.values()):
        raise RuntimeError(_NO_CPU)
    first = next(iter(given.values())).device
    for name, t in given.items():
        if t.device != first:
            raise ValueError(f"instance.{who}: {name} is on {t.device}, expected {first}")


def _label(segments_or_label, who):
    """(label int32 [P] contiguous, the Segments it came from or None)"""
    seg = segments_or_label if isinstance(segments_or_label, Segments) else None
    label = _tensor(seg.label if seg is not None else segments_or_label, who, "label", (torch.int32,))
    if label.dim() != 1:
        raise ValueError(f"instance.{who}: label must have shape (P,)")
    if label.shape[0] >= MAX_ROWS:
        raise ValueError(f"instance.{who}: need P < 2^30")
    return label.contiguous(), seg


def _capacity(capacity, label, seg, who):
    """K: the int given, or -- the one read-back -- the Segments' count (a bare label array: its largest label + 1)"""
    if capacity is None:
        if not label.is_cuda:
            raise RuntimeError(_NO_CPU)
        if seg is not None:
            return int(seg.count.cpu()[0])
        return max(int(label.max().cpu()) + 1, 0) if label.numel() else 0
    if isinstance(capacity, bool) or not isinstance(capacity, int):
        raise TypeError(f"instance.{who}: capacity must be an int or None")
    if not 0 <= capacity < MAX_ROWS:
        raise ValueError(f"instance.{who}: need 0 <= capacity < 2^30")
    return capacity


def _per_row(t, P, who, what, dtypes, tail=()):
    """an optional per-row tensor of shape (P, *tail), detached and contiguous"""
    if t is None:
        return None
    t = _tensor(t, who, what, dtypes)
    if tuple(t.shape) != (P,) + tuple(tail):
        raise ValueError(f"instance.{who}: {what} must have shape {(P,) + tuple(tail)}")
    return t.detach().contiguous()


def members(segments_or_label, capacity=None):
    """-> Members(ptr, rows, K): the partition as lists (module docstring).  segments_or_label: a segment.Segments or its label
    int32 [P]; capacity: K, the number of instances to list -- None reads segments.count back (the one synchronisation), an int
    synchronises nothing; labels at or above it are in no instance.  The same integers on every call."""
    label, seg = _label(segments_or_label, "members")
    K = _capacity(capacity, label, seg, "members")
    _on_gpu("members", label=label)
    lib = _lib.load()
    dev, P = label.device, int(label.shape[0])
    with torch.cuda.device(dev):
        mptr = torch.empty((K + 1,), dtype=torch.int32, device=dev)
        rows = torch.empty((P,), dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.goi_instance_members_workspace_bytes(P, K), dev)
        check(lib.goi_instance_members(P, K, ptr(label), ptr(mptr), ptr(rows), ptr(ws), stream(dev)))
    return Members(mptr, rows, K)


_members = members  # (stats has a parameter of that name)


def stats(segments_or_label, xyz, features=None, weight=None, hit=None, members=None, capacity=None):  # noqa: A002
    """-> InstanceStats (module docstring).  xyz float32 [P,3] (None: every position is the origin, for a caller that wants the
    counts alone); features float32 [P,S], 1 <= S <= 32; weight float32 [P] (absent: 1); hit bool or uint8 [P] (uint8: eight
    flag bits); members: what members() returned for this partition (absent: built here, from `capacity` as in members()).
    Asynchronous; with members= or an int capacity nothing is read back."""
    label, seg = _label(segments_or_label, "stats")
    P = int(label.shape[0])
    xyz = _per_row(xyz, P, "stats", "xyz", (torch.float32,), (3,))
    S = 1
    if features is not None:
        features = _tensor(features, "stats", "features", (torch.float32,))
        if features.dim() != 2 or features.shape[0] != P or not 1 <= features.shape[1] <= S_MAX:
            raise ValueError(f"instance.stats: features must have shape ({P}, S) with 1 <= S <= {S_MAX}")
        features = features.detach().contiguous()
        S = int(features.shape[1])
    weight = _per_row(weight, P, "stats", "weight", (torch.float32,))
    hit = _per_row(hit, P, "stats", "hit", (torch.bool, torch.uint8))
    if hit is not None and hit.dtype == torch.bool:
        hit = hit.view(torch.uint8)
    if members is not None:
        if not isinstance(members, Members):
            raise TypeError("instance.stats: members must be what members() returned")
        if tuple(members.rows.shape) != (P,) or tuple(members.ptr.shape) != (members.K + 1,):
            raise ValueError(f"instance.stats: members is not for {P} rows")
    _on_gpu("stats", label=label, xyz=xyz, features=features, weight=weight, hit=hit,
            member_ptr=None if members is None else members.ptr, member_rows=None if members is None else members.rows)
    if members is None:
        members = _members(seg if seg is not None else label, capacity)
    K = members.K
    lib = _lib.load()
    dev = label.device
    with torch.cuda.device(dev):
        # two allocations, cut into the contiguous outputs: hits [K,8] | n [K], and centroid | lo | hi | cov | wsum | feature
        ints = torch.empty((K * 9,), dtype=torch.int32, device=dev)
        hits, n = ints[:K * 8].view(K, 8), ints[K * 8:]
        Sf = S if features is not None else 0
        flt = (torch.zeros if P == 0 else torch.empty)((K * (16 + Sf),), dtype=torch.float32, device=dev)
        centroid, lo, hi = (flt[K * 3 * i:K * 3 * (i + 1)].view(K, 3) for i in range(3))
        cov, wsum = flt[K * 9:K * 15].view(K, 6), flt[K * 15:K * 16]
        # (an empty model's features have no address: the library takes them as absent and writes no feature row -- zeros above)
        feature = flt[K * 16:].view(K, S) if features is not None else None
        ws = _lib.workspace(lib.goi_instance_stats_workspace_bytes(P, K), dev)
        check(lib.goi_instance_stats(P, K, S, ptr(members.ptr), ptr(members.rows), ptr(xyz), ptr(features), ptr(weight), ptr(hit),
                                     ptr(n), ptr(hits), ptr(wsum), ptr(centroid), ptr(lo), ptr(hi), ptr(cov), ptr(feature), ptr(ws),
                                     stream(dev)))
    return InstanceStats(n, hits, wsum, centroid, lo, hi, cov, feature, members)


def fraction_of(min_fraction):
    """min_fraction as an exact rational (num, den), 0 <= num <= den < 2^32: a Fraction or an int as it is, a float as the
    shortest decimal that reads back as that float (0.7 is 7 / 10, not the binary number next to it)"""
    if isinstance(min_fraction, bool) or not isinstance(min_fraction, (int, float, Fraction)):
        raise TypeError("instance.vote: min_fraction must be a number or a Fraction")
    q = Fraction(repr(min_fraction)) if isinstance(min_fraction, float) else Fraction(min_fraction)
    if not 0 <= q <= 1:
        raise ValueError("instance.vote: need 0 <= min_fraction <= 1")
    q = q.limit_denominator(2 ** 32 - 1)
    return q.numerator, q.denominator


def vote(stats, min_fraction=0.5, min_hits=1, bit=0):  # noqa: A002
    """-> bool [K]: the instances with hits >= min_hits and hits / n >= min_fraction for flag `bit`, decided in int64 as
    hits * den >= num * n with min_fraction = num / den (fraction_of): no float rounding, a tie is kept.  An empty instance
    has no hit, so min_hits >= 1 never keeps it.  Torch glue on [K] arrays; it does not synchronise."""
    if not isinstance(stats, InstanceStats):
        raise TypeError("instance.vote: stats must be what stats() returned")
    if isinstance(min_hits, bool) or not isinstance(min_hits, int) or not 0 <= min_hits < 2 ** 31:
        raise ValueError("instance.vote: min_hits must be an int, 0 <= min_hits < 2^31")
    if isinstance(bit, bool) or not isinstance(bit, int) or not 0 <= bit < 8:
        raise ValueError("instance.vote: bit must be an int, 0 <= bit < 8")
    num, den = fraction_of(min_fraction)
    h, n = stats.hits[:, bit].to(torch.int64), stats.n.to(torch.int64)
    return (h >= min_hits) & (h * den >= num * n)


def rows_of(segments_or_label, keep):
    """-> bool [P]: the rows of the kept instances.  keep: bool [K]; a row whose label is outside [0, K) -- -1 included -- is
    in no instance and is not returned.  Torch glue on a gather; it does not synchronise."""
    label, _ = _label(segments_or_label, "rows_of")
    keep = _tensor(keep, "rows_of", "keep", (torch.bool,))
    if keep.dim() != 1:
        raise ValueError("instance.rows_of: keep must have shape (K,)")
    _on_gpu("rows_of", label=label, keep=keep)
    K = int(keep.shape[0])
    table = torch.cat([keep, torch.zeros((1,), dtype=torch.bool, device=keep.device)])  # slot K stays False
    inside = (label >= 0) & (label < K)
    return table.index_select(0, torch.where(inside, label, torch.full_like(label, K)).to(torch.int64))


def select(segments, hit, min_fraction=0.5, min_hits=1, capacity=None):
    """-> bool [P]: `hit` (bool [P]: a per-row mask with holes and speckle) turned into whole instances --
    rows_of(segments, vote(stats(segments, None, hit=hit), min_fraction, min_hits)).  capacity as in members()."""
    hit = _tensor(hit, "select", "hit", (torch.bool,))
    return rows_of(segments, vote(stats(segments, None, hit=hit, capacity=capacity), min_fraction, min_hits))
