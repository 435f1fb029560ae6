"""Non-rigid edits of a selection of Gaussians on the device (csrc/deform.hip): drag a handle and bend an arm.

The standard embedded-deformation / as-rigid-as-possible edit (Sumner et al. 2007, Sorkine & Alexa 2007): a sparse graph of
control nodes is laid over the selection, some nodes are pinned or dragged, the others follow so that every node's neighbourhood
moves as rigidly as it can, and every Gaussian blends the motions of the nodes it is bound to.  `edit.transform` is the special
case of one rotation for the whole object.

    sample_nodes(xyz, selection=None, spacing=..., invert=False)      -> int64 [M]: the Gaussians that become control nodes
    solve(x, idx, constrained, target, weight=None, transposed=None, y0=None, q0=None,
          iterations=10, polar_iters=4, relax=0.8)                     -> (y float32 [M,3], q float32 [M,4])
    energy(x, idx, y, q, weight=None)                                  -> float64 0-d
    Deformation(g, selection=None, *, spacing, k=8, kb=4, invert=False, sigma=None)
        .constrain(nodes, targets)  .release(nodes=None)  .nearest_node(point)  .drag(nodes, translation=, rotation=, pivot=)
        .solve(iterations=10)  .energy()  .apply()  .reset()  .commit(moments=True)

With x the nodes' rest positions, y their deformed positions, R_i = R(q_i) their rotations and (i, m) the edges of the node graph
idx [M,k] (`knn.graph(x, k)`; entry (i, m) is an edge iff 0 <= idx[i,m] < M and idx[i,m] != i),

    E = sum_i sum_m w[i,m] |(y_i - y_j) - R_i (x_i - x_j)|^2,   j = idx[i,m].

One `solve` iteration is two launches.  POSITIONS, a Jacobi step from the old y and q: a constrained node takes its target, a free
node moves `relax` of the way to the minimiser of E over its own y_i (out-edges in row order, then in-edges in the transpose's
order, so the sum's order depends on the graph alone).  ROTATIONS: A_i = sum_m w (y_i - y_j)(x_i - x_j)^T and polar_iters steps of
the warm-started quaternion iteration of Mueller et al. 2016 towards the polar factor of A_i; a zero torque (an isolated node,
coincident or collinear neighbours) leaves q_i where it was.  The rotations returned are those OF the positions returned.
relax = 1 is the plain Jacobi step, which can oscillate for ever on a bipartite component without a constraint; the default 0.8
damps that mode by 0.6 per iteration and never raises E.

`apply`: a selected Gaussian bound to nodes a (`knn.query` of the Gaussians against the nodes, kb of them) gets, from the REST
copies taken when the session began (repeated drags never accumulate rounding),

    w_a = exp(-(d_a^2 - d_0^2) / (2 sigma^2)) normalised,        d_0 the nearest node's distance
    x'  = x + sum_a w_a [(y_a - x_a) + (R_a - I)(x - x_a)]
    q_g = normalize(sum_a w_a s_a q_a),  s_a = +-1 aligning q_a with the first;   _rotation' = q_g (x) r
    every stored band l = 1..3 of _features_rest times D_l(R(q_g)) per channel, built per Gaussian in the kernel

and _scaling, _features_dc, _opacity, _semantics and every unselected or unbound row keep their bits: ARAP has no scale.  With
nothing displaced (y = x, q = identity) every tensor keeps its bits.  A model with a semantic mask set is refused, as by
edit.transform.  Every tensor written through a raw pointer has its version counter bumped.  fp32 tensors on a ROCm GPU only;
there is no CPU fallback.  solve, energy, apply and commit never synchronise the host; building the session synchronises it
several times, once per session (sample_nodes: nonzero, unique and the node count).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib, densify, edit, knn, smooth
from ._lib import check, ptr, stream, workspace

_NO_CPU = "goi_hyperplane_amd.deform: tensors must live on a ROCm GPU; there is no CPU fallback"
KB_MAX = 8             # goi_deform_apply: 1 <= kb <= 8
MAX_ENTRIES = 2 ** 30  # M * k below this

# The 2 l + 1 directions at which the kernel evaluates band l (normalised below).  Band 1: the axes.  Bands 2 and 3: found once by
# a search for a well-conditioned basis matrix (condition numbers 1.55 and 1.93), kept as three decimals.
_DIRS = (
    ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
    ((0.678, 0.332, -0.656), (0.378, -0.693, 0.614), (0.777, -0.477, -0.41), (0.934, -0.109, 0.342), (0.034, -0.018, 0.999)),
    ((-0.505, -0.156, -0.849), (0.469, 0.826, -0.314), (-0.042, 0.44, 0.897), (-0.759, -0.131, 0.638), (-0.771, 0.433, -0.467),
     (-0.179, 0.953, -0.244), (-0.262, -0.881, -0.395)),
)
_SH = []


def sh_constants():
    """[(dirs float64 [2l+1, 3] unit, inv float64 [2l+1, 2l+1]) for l = 1, 2, 3]: within band l, Y_l(R^T d) = Y_l(d) D_l(R) for
    every direction d (edit.sh_rotation), so with Y0 = Y_l(dirs), D_l(R) c = inv(Y0) (Y_l(R^T dirs) c): what deform_apply_k does
    per Gaussian.  Formed once, in float64."""
    if not _SH:
        for l, dirs in enumerate(_DIRS, start=1):
            d = np.asarray(dirs, dtype=np.float64)
            d = d / np.linalg.norm(d, axis=1, keepdims=True)
            Y0 = edit._sh_basis(d, 3)[:, l * l:(l + 1) * (l + 1)]
            _SH.append((d, np.linalg.inv(Y0)))
    return list(_SH)


def _sh_struct():
    """GoiDeformSH: the constants rounded to fp32 once"""
    t = _lib.GoiDeformSH()
    for l, (d, inv) in enumerate(sh_constants(), start=1):
        getattr(t, f"dirs{l}")[:] = d.reshape(-1).tolist()
        getattr(t, f"inv{l}")[:] = inv.reshape(-1).tolist()
    return t


# ---- validation: everything that can be wrong before the device matters ------------------------------------------------------
def _tensor(t, fn, what, dtypes, shape=None):
    if not torch.is_tensor(t):
        raise TypeError(f"deform.{fn}: {what} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"deform.{fn}: {what} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"deform.{fn}: {what} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _on_gpu(fn, **tensors):
    given = {name: t for name, t in tensors.items() if t is not None}
    if any(not t.is_cuda for t in given.values()):
        raise RuntimeError(_NO_CPU)
    first = next(iter(given.values())).device
    for name, t in given.items():
        if t.device != first:
            raise ValueError(f"deform.{fn}: {name} is on {t.device}, expected {first}")
    return first


def _int(v, fn, what, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"deform.{fn}: {what} must be an int")
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"deform.{fn}: need {lo} <= {what}" + (f" <= {hi}" if hi is not None else "") + f", got {v}")
    return v


def _positive(v, fn, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise TypeError(f"deform.{fn}: {what} must be a number") from None
    if not math.isfinite(v) or v <= 0:
        raise ValueError(f"deform.{fn}: {what} must be finite and > 0, got {v}")
    return v


def _bytes(m):
    """bool or uint8 [n], contiguous -> uint8 (a view of a bool: no copy); None stays None"""
    if m is None:
        return None
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _graph_args(fn, x, idx, weight):
    x = _tensor(x, fn, "x", (torch.float32,))
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"deform.{fn}: x has shape {tuple(x.shape)}, expected [M, 3]")
    M = int(x.shape[0])
    idx = _tensor(idx, fn, "idx", (torch.int32,))
    if idx.dim() != 2 or idx.shape[0] != M or idx.shape[1] < 1:
        raise ValueError(f"deform.{fn}: idx must have shape ({M}, k) with k >= 1")
    if M * int(idx.shape[1]) >= MAX_ENTRIES:
        raise ValueError(f"deform.{fn}: need M * k < 2^30")
    if weight is not None:
        _tensor(weight, fn, "weight", (torch.float32,), tuple(idx.shape))
    return M, int(idx.shape[1])


# ---- the deformation graph -----------------------------------------------------------------------------------------------------
def sample_nodes(xyz, selection=None, spacing=None, invert=False):
    """int64 [M], ascending: the selected Gaussians that become control nodes, one per occupied cube of side `spacing` of the
    lattice anchored at the selection's `lo` corner (edit.selection_bounds): the cube of a point is floor((x - lo) / spacing) in
    fp32, the node of a cube the lowest Gaussian id in it.  An empty selection gives no node.

    This runs once per editing session and has to size its output: it is torch glue on the device (nonzero, unique, an amin
    scatter) with read-backs of the counts, NOT a hot path, and it synchronises the host."""
    fn = "sample_nodes"
    _tensor(xyz, fn, "xyz", (torch.float32,))
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"deform.{fn}: xyz has shape {tuple(xyz.shape)}, expected [P, 3]")
    spacing = _positive(spacing, fn, "spacing")
    P = int(xyz.shape[0])
    if selection is not None:
        _tensor(selection, fn, "selection", (torch.bool, torch.uint8), (P,))
    dev = _on_gpu(fn, xyz=xyz, selection=selection)
    xyz = xyz.detach().contiguous()
    lo = edit.selection_bounds(xyz, selection, invert)["lo"]
    if selection is None:
        ids = torch.arange(P, dtype=torch.int64, device=dev)
    else:
        ids = torch.nonzero((selection != 0) != bool(invert)).squeeze(1)
    if ids.numel() == 0:
        return ids
    side = torch.full((1,), spacing, dtype=torch.float32, device=dev)  # (a device divisor: a true fp32 division, no reciprocal)
    cells = torch.floor((xyz[ids] - lo) / side).to(torch.int64)
    uniq, inverse = torch.unique(cells, dim=0, return_inverse=True)
    first = torch.full((int(uniq.shape[0]),), P, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, inverse, ids, "amin")
    return torch.sort(first).values


# ---- the solve --------------------------------------------------------------------------------------------------------------------
def solve(x, idx, constrained=None, target=None, *, weight=None, transposed=None, y0=None, q0=None, iterations=10, polar_iters=4,
          relax=0.8):
    """-> (y float32 [M,3], q float32 [M,4] unit (w, x, y, z)) after `iterations` iterations of (positions, rotations) from the warm
    start y0 (default x) and q0 (default the identity); see the module docstring.  x [M,3]: rest positions; idx int32 [M,k]: the
    node graph; weight [M,k] or None (1; smooth.gaussian_weights fits); transposed: smooth.transpose(idx), built here when not
    given; constrained bool / uint8 [M] with target [M,3], or None for no constraint.  iterations = 0 returns the warm start.
    2 * iterations launches on the current stream, no read-back."""
    fn = "solve"
    M, k = _graph_args(fn, x, idx, weight)
    iterations = _int(iterations, fn, "iterations", 0)
    polar_iters = _int(polar_iters, fn, "polar_iters", 0)
    try:
        relax = float(relax)
    except (TypeError, ValueError):
        raise TypeError(f"deform.{fn}: relax must be a number") from None
    if not 0.0 < relax <= 1.0:
        raise ValueError(f"deform.{fn}: need 0 < relax <= 1, got {relax}")
    if (constrained is None) != (target is None):
        raise ValueError(f"deform.{fn}: constrained and target come together")
    if constrained is not None:
        _tensor(constrained, fn, "constrained", (torch.bool, torch.uint8), (M,))
        _tensor(target, fn, "target", (torch.float32,), (M, 3))
    if y0 is not None:
        _tensor(y0, fn, "y0", (torch.float32,), (M, 3))
    if q0 is not None:
        _tensor(q0, fn, "q0", (torch.float32,), (M, 4))
    if transposed is not None:
        if not isinstance(transposed, (tuple, list)) or len(transposed) != 2:
            raise TypeError(f"deform.{fn}: transposed must be the pair smooth.transpose(idx) returned")
        _tensor(transposed[0], fn, "transposed[0]", (torch.int32,), (M + 1,))
        _tensor(transposed[1], fn, "transposed[1]", (torch.int32,), (M * k,))
    dev = _on_gpu(fn, x=x, idx=idx, weight=weight, constrained=constrained, target=target, y0=y0, q0=q0,
                  **({} if transposed is None else {"transposed[0]": transposed[0], "transposed[1]": transposed[1]}))
    x, idx = x.detach().contiguous(), idx.contiguous()
    with torch.cuda.device(dev):
        y = (x if y0 is None else y0.detach()).clone().contiguous()
        if q0 is None:
            q = torch.zeros((M, 4), dtype=torch.float32, device=dev)
            q[:, 0] = 1.0
        else:
            q = q0.detach().clone().contiguous()
        if M == 0 or iterations == 0:
            return y, q
        in_ptr, in_edge = smooth.transpose(idx) if transposed is None else (transposed[0].contiguous(), transposed[1].contiguous())
        weight = None if weight is None else weight.detach().contiguous()
        target = None if target is None else target.detach().contiguous()
        lib = _lib.load()
        ws = workspace(lib.goi_deform_solve_workspace_bytes(M), dev)
        check(lib.goi_deform_solve(M, k, ptr(x), ptr(idx), ptr(weight), ptr(in_ptr), ptr(in_edge), ptr(_bytes(constrained)),
                                   ptr(target), iterations, polar_iters, relax, ptr(y), ptr(q), ptr(ws), stream(dev)), ValueError)
    return y, q


def energy(x, idx, y, q, weight=None):
    """-> float64 0-d on the device: E of the module docstring, every term formed in float64 from the fp32 inputs and summed in a
    fixed order (the same bits on every call).  No read-back."""
    fn = "energy"
    M, k = _graph_args(fn, x, idx, weight)
    _tensor(y, fn, "y", (torch.float32,), (M, 3))
    _tensor(q, fn, "q", (torch.float32,), (M, 4))
    dev = _on_gpu(fn, x=x, idx=idx, y=y, q=q, weight=weight)
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty((), dtype=torch.float64, device=dev)
        ws = workspace(lib.goi_deform_energy_workspace_bytes(M), dev)
        weight = None if weight is None else weight.detach().contiguous()
        check(lib.goi_deform_energy(M, k, ptr(x.detach().contiguous()), ptr(idx.contiguous()), ptr(weight), ptr(y.detach().contiguous()),
                                    ptr(q.detach().contiguous()), ptr(out), ptr(ws), stream(dev)), ValueError)
    return out


# ---- the apply --------------------------------------------------------------------------------------------------------------------
def apply_nodes(dst, src, bind, nodes, sigma, selection=None, invert=False, moments=False):
    """One launch of deform_apply_k.  dst = (xyz [P,3], rotation [P,4], features_rest [P,M-1,3]) is written in place; src = the
    REST tensors of the same shapes (moments=False), which may be dst; bind = (idx int32 [P,kb], dist2 float32 [P,kb]) from
    knn.query(xyz, x, kb); nodes = (x [n,3], y [n,3], q [n,4]).  moments=True: dst holds Adam first moments (None for a group
    that has none), turned in place by each row's blended rotation, and src is not read.  Bumps the version counter of every
    tensor it writes.  What Deformation.apply and .commit call; no host synchronisation."""
    fn = "apply_nodes"
    bidx, bd2 = bind
    nx, ny, nq = nodes
    _tensor(bidx, fn, "bind idx", (torch.int32,))
    if bidx.dim() != 2 or not 1 <= bidx.shape[1] <= KB_MAX:
        raise ValueError(f"deform.{fn}: bind idx must have shape (P, kb) with 1 <= kb <= {KB_MAX}")
    P, kb = int(bidx.shape[0]), int(bidx.shape[1])
    _tensor(bd2, fn, "bind dist2", (torch.float32,), (P, kb))
    _tensor(nx, fn, "nodes x", (torch.float32,))
    if nx.dim() != 2 or nx.shape[1] != 3:
        raise ValueError(f"deform.{fn}: nodes x has shape {tuple(nx.shape)}, expected [n, 3]")
    n = int(nx.shape[0])
    _tensor(ny, fn, "nodes y", (torch.float32,), (n, 3))
    _tensor(nq, fn, "nodes q", (torch.float32,), (n, 4))
    sigma = _positive(sigma, fn, "sigma")
    xyz, rot, rest = dst
    if rest is None and not moments:
        raise ValueError(f"deform.{fn}: features_rest is missing")
    Msh = None
    for what, t, row in (("xyz", xyz, (P, 3)), ("rotation", rot, (P, 4))):
        if t is None and moments:
            continue
        _tensor(t, fn, what, (torch.float32,), row)
    for t in (rest,) + (() if moments else (src[2],)):
        if t is None:
            continue
        _tensor(t, fn, "features_rest", (torch.float32,))
        if t.dim() != 3 or t.shape[0] != P or t.shape[2] != 3 or int(t.shape[1]) + 1 not in (1, 4, 9, 16):
            raise ValueError(f"deform.{fn}: features_rest has shape {tuple(t.shape)}, expected [{P}, M - 1, 3] with M in (1, 4, 9, 16)")
        if Msh is not None and int(t.shape[1]) + 1 != Msh:
            raise ValueError(f"deform.{fn}: the rest copy of features_rest has another shape")
        Msh = int(t.shape[1]) + 1
    if Msh is None:
        Msh = 1
    if not moments:
        _tensor(src[0], fn, "rest xyz", (torch.float32,), (P, 3))
        _tensor(src[1], fn, "rest rotation", (torch.float32,), (P, 4))
    if selection is not None:
        _tensor(selection, fn, "selection", (torch.bool, torch.uint8), (P,))
    named = {"bind idx": bidx, "bind dist2": bd2, "nodes x": nx, "nodes y": ny, "nodes q": nq, "xyz": xyz, "rotation": rot,
             "features_rest": rest, "selection": selection}
    if not moments:
        named.update({"rest xyz": src[0], "rest rotation": src[1], "rest features_rest": src[2]})
    dev = _on_gpu(fn, **named)
    for what, t in named.items():
        if t is not None and what in ("xyz", "rotation", "features_rest") and not t.is_contiguous():
            raise ValueError(f"deform.{fn}: {what} must be contiguous (it is written in place)")
    s = (None, None, None) if moments else tuple(None if t is None else t.detach().contiguous() for t in src)
    lib = _lib.load()
    sh = _sh_struct()
    rest_w = rest if Msh > 1 else None
    with torch.cuda.device(dev):
        check(lib.goi_deform_apply(P, Msh, n, kb, ptr(_bytes(selection)), 1 if invert else 0, ptr(bidx.contiguous()),
                                   ptr(bd2.contiguous()), sigma, ptr(nx.detach().contiguous()), ptr(ny.detach().contiguous()),
                                   ptr(nq.detach().contiguous()), ctypes.byref(sh), ptr(s[0]), ptr(s[1]),
                                   ptr(s[2]) if Msh > 1 else None, ptr(xyz), ptr(rot), ptr(rest_w), 1 if moments else 0,
                                   stream(dev)), ValueError)
    for w in (xyz, rot, rest_w):
        if w is not None:
            torch.autograd.graph.increment_version(w)


# ---- the session ------------------------------------------------------------------------------------------------------------------
class Deformation:
    """One editing session on the model `g` (any object with the reference GaussianModel's attributes, as edit.transform takes
    them).  Holds whole-tensor clones of _xyz, _rotation and _features_rest as the REST state, the control nodes (sample_nodes at
    `spacing`), their graph (knn.graph, k) with its transpose, the binding of every selected Gaussian to its kb nearest nodes
    (knn.query) and the current node positions y and rotations q, which the next solve starts from.  sigma (default: spacing) is
    the width of the binding weights.  Building it synchronises (sample_nodes); after that only nearest_node and a bool node mask do."""

    def __init__(self, g, selection=None, *, spacing, k=8, kb=4, invert=False, sigma=None):
        fn = "Deformation"
        spacing = _positive(spacing, fn, "spacing")
        self.sigma = spacing if sigma is None else _positive(sigma, fn, "sigma")
        _int(k, fn, "k", 1, knn.K_MAX)
        _int(kb, fn, "kb", 1, KB_MAX)
        if getattr(g, "_semantics_masks", None) is not None:
            raise ValueError(f"deform.{fn}: the model has a semantic mask set (set_semantic_masks); clear it "
                             "(set_semantic_masks(None)) before editing the model")
        xyz = _tensor(g._xyz, fn, "_xyz", (torch.float32,))
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError(f"deform.{fn}: _xyz has shape {tuple(xyz.shape)}, expected [P, 3]")
        P = int(xyz.shape[0])
        _tensor(g._rotation, fn, "_rotation", (torch.float32,), (P, 4))
        rest = _tensor(g._features_rest, fn, "_features_rest", (torch.float32,))
        if rest.dim() != 3 or rest.shape[0] != P or rest.shape[2] != 3 or int(rest.shape[1]) + 1 not in (1, 4, 9, 16):
            raise ValueError(f"deform.{fn}: _features_rest has shape {tuple(rest.shape)}, expected [{P}, M - 1, 3] with M in "
                             "(1, 4, 9, 16)")
        if selection is not None:
            _tensor(selection, fn, "selection", (torch.bool, torch.uint8), (P,))
        dev = _on_gpu(fn, _xyz=xyz, _rotation=g._rotation, _features_rest=rest, selection=selection)
        for what in ("_xyz", "_rotation", "_features_rest"):
            if not getattr(g, what).is_contiguous():
                raise ValueError(f"deform.{fn}: {what} must be contiguous")
        self.g, self.P, self.k, self.kb, self.spacing, self.device = g, P, k, kb, spacing, dev
        # the effective selection as one bool mask: knn.query and the kernels take it as it is
        self.mask = None if selection is None else ((selection != 0) != bool(invert)).contiguous()
        self._take_rest()
        self.node_ids = sample_nodes(self.rest[0], self.mask, spacing)
        self.M = int(self.node_ids.shape[0])
        self._build(self.rest[0][self.node_ids].contiguous())
        self.constrained = torch.zeros((self.M,), dtype=torch.uint8, device=dev)
        self.target = self.x.clone()

    def _take_rest(self):
        g = self.g
        self.rest = (g._xyz.detach().clone(), g._rotation.detach().clone(), g._features_rest.detach().clone())

    def _build(self, x):
        """the graph, its transpose and the binding over the rest node positions x; y = x, q = identity"""
        self.x = x
        if self.M:
            self.idx, self.dist2 = knn.graph(x, self.k)
            self.transposed = smooth.transpose(self.idx)
            self.bind = knn.query(self.rest[0], x, self.kb, query_mask=self.mask)
        else:
            self.idx = torch.empty((0, self.k), dtype=torch.int32, device=self.device)
            self.dist2 = torch.empty((0, self.k), dtype=torch.float32, device=self.device)
            self.transposed = None
            self.bind = (torch.full((self.P, self.kb), -1, dtype=torch.int32, device=self.device),
                         torch.full((self.P, self.kb), math.inf, dtype=torch.float32, device=self.device))
        self.y = x.clone()
        self.q = torch.zeros((self.M, 4), dtype=torch.float32, device=self.device)
        self.q[:, 0] = 1.0

    def _nodes(self, nodes, fn):
        """int64 ids on the device from ids (a tensor, a sequence, one int) or a bool mask [M].  Host ids outside [0, M) raise;
        ids that are already on the device are not read back: _put ignores those outside [0, M), it never indexes with them."""
        if torch.is_tensor(nodes) and nodes.dtype == torch.bool:
            if tuple(nodes.shape) != (self.M,):
                raise ValueError(f"deform.{fn}: a node mask must have shape ({self.M},)")
            return torch.nonzero(nodes.to(self.device)).squeeze(1)
        ids = torch.as_tensor(nodes, dtype=torch.int64).reshape(-1)
        if ids.device.type == "cpu":
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.M):
                raise ValueError(f"deform.{fn}: node ids must lie in [0, {self.M})")
        return ids.to(self.device)

    def constrain(self, nodes, targets):
        """pins the nodes (ids or a bool mask [M]) at `targets` [n, 3] (or one [3] for all of them)"""
        ids = self._nodes(nodes, "constrain")
        t = torch.as_tensor(targets, dtype=torch.float32).to(self.device)
        if t.dim() == 1:
            t = t.expand(int(ids.shape[0]), 3)
        if tuple(t.shape) != (int(ids.shape[0]), 3):
            raise ValueError(f"deform.constrain: targets has shape {tuple(t.shape)}, expected ({int(ids.shape[0])}, 3)")
        self.constrained = self._put(self.constrained, ids, 1)
        self.target = self._put(self.target, ids, t)
        return self

    def _put(self, dst, ids, value):
        """dst with value written at the rows `ids`; an id outside [0, M) writes to a spare row that is cut off again"""
        slot = torch.where((ids >= 0) & (ids < self.M), ids, self.M)
        out = torch.cat([dst, dst.new_zeros((1,) + tuple(dst.shape[1:]))])
        out[slot] = value
        return out[:self.M].contiguous()

    def release(self, nodes=None):
        """frees the nodes (None: every node); they keep their current positions as the warm start"""
        if nodes is None:
            self.constrained.zero_()
        else:
            self.constrained = self._put(self.constrained, self._nodes(nodes, "release"), 0)
        return self

    def nearest_node(self, point):
        """the id (an int: this reads back) of the node whose REST position is nearest to `point` (three numbers); -1 without nodes"""
        p = torch.as_tensor(point, dtype=torch.float32).reshape(1, 3).to(self.device)
        if self.M == 0:
            return -1
        return int(knn.query(p, self.x, 1)[0][0, 0])

    def drag(self, nodes, *, translation=None, rotation=None, pivot=None):
        """constrains the nodes to the image of their REST positions under x -> p + t + R (x - p): rotation a 3x3 matrix or a
        (w, x, y, z) quaternion, translation three numbers (edit.Similarity), pivot three numbers, a device tensor [3] or None for
        the centroid of the nodes' rest positions (formed on the device).  Dragging a node again replaces its target."""
        fn = "drag"
        sim = edit.Similarity(rotation, translation, 1.0, fn)
        ids = self._nodes(nodes, fn)
        ok = (ids >= 0) & (ids < self.M)
        x = self.x[ids.clamp(0, max(self.M - 1, 0))] if self.M else self.x.new_zeros((int(ids.shape[0]), 3))
        if pivot is None:  # the centroid of the valid ids' rest positions
            p = ((x.double() * ok.unsqueeze(1)).sum(dim=0) / ok.sum().clamp(min=1)).float()
        else:
            p = torch.as_tensor(pivot, dtype=torch.float32).reshape(3).to(self.device)
        R = torch.tensor(sim.R, dtype=torch.float32, device=self.device)
        t = torch.tensor(sim.t, dtype=torch.float32, device=self.device)
        return self.constrain(ids, (x - p) @ R.T + p + t)

    def solve(self, iterations=10, polar_iters=4, relax=0.8, weight=None):
        """`iterations` more iterations from the current y and q (the warm start of the next call)"""
        if self.M:
            self.y, self.q = solve(self.x, self.idx, self.constrained, self.target, weight=weight, transposed=self.transposed,
                                   y0=self.y, q0=self.q, iterations=iterations, polar_iters=polar_iters, relax=relax)
        return self

    def energy(self, weight=None):
        return energy(self.x, self.idx, self.y, self.q, weight)

    def _model(self):
        g = self.g
        for what, t in (("_xyz", g._xyz), ("_rotation", g._rotation), ("_features_rest", g._features_rest)):
            if tuple(t.shape) != tuple(self.rest[("_xyz", "_rotation", "_features_rest").index(what)].shape):
                raise ValueError(f"deform: the model's {what} changed shape since the session began")
        return g._xyz, g._rotation, g._features_rest

    def apply(self):
        """writes the deformed selection into the model, in place, from the REST copies: one launch, no synchronisation"""
        if self.M:
            apply_nodes(self._model(), self.rest, self.bind, (self.x, self.y, self.q), self.sigma, self.mask)
        return self

    def _restore(self, dst, src):
        """the selected rows of src into dst, without a boolean index's synchronisation"""
        for d, s in zip(dst, src):
            if self.mask is None:
                d.detach().copy_(s)
            else:
                m = self.mask.view((self.P,) + (1,) * (d.dim() - 1))
                d.detach().copy_(torch.where(m, s, d.detach()))

    def reset(self):
        """puts the REST rows of the selection back into the model, bit for bit, sets y = x and q = identity and frees every node"""
        self._restore(self._model(), self.rest)
        self.y = self.x.clone()
        self.q.zero_()
        self.q[:, 0] = 1.0
        self.target = self.x.clone()
        return self.release()

    def commit(self, moments=True):
        """after apply(): makes the current state the new REST.  With moments=True the Adam first moments (exp_avg of the groups
        xyz, rotation and f_rest, found through densify._groups) of the selected rows are turned by each row's blended rotation --
        R m, q_g (x) m, D_l m, the device functions apply uses; exp_avg_sq, `step` and every other group stay as they are, exactly
        as edit.transform documents.  The nodes' deformed positions become their rest positions, the graph and the binding are
        rebuilt over them, and constrained nodes stay pinned where they are."""
        fn = "commit"
        model = self._model()
        if moments and self.M:
            opt, groups = densify._groups(self.g, fn)
            mom = []
            for name, p in (("xyz", model[0]), ("rotation", model[1]), ("f_rest", model[2])):
                st = opt.state.get(p, None) if opt is not None and name in groups else None
                m = st.get("exp_avg") if st else None
                if m is not None:
                    _tensor(m, fn, f"the exp_avg of group {name!r}", (torch.float32,), tuple(p.shape))
                mom.append(m)
            if any(m is not None for m in mom):
                apply_nodes(tuple(mom), None, self.bind, (self.x, self.y, self.q), self.sigma, self.mask, moments=True)
        self._restore(self.rest, tuple(t.detach() for t in model))
        self.target = torch.where(self.constrained.bool().unsqueeze(1), self.target, self.y)
        self._build(self.y.clone())
        return self
