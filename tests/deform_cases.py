"""Named small cases for goi_hyperplane_amd.deform: node graphs for the solve, models and node motions for the apply.  Pure numpy;
tests/test_deform_cpu.py holds every case to "the float32 twin stays within 1e-4 of the bounding-box diagonal of the float64
run", which is a condition on these inputs, and tests/test_gpu_deform.py runs the kernels on them."""
import math

import numpy as np


def knn_graph(x, k):
    """int32 [M,k]: the k nearest OTHER points, ties to the lower id, -1 tails (knn.graph restated in float64)"""
    M = x.shape[0]
    idx = np.full((M, k), -1, dtype=np.int32)
    d = ((x[:, None, :].astype(np.float64) - x[None, :, :]) ** 2).sum(-1)
    for i in range(M):
        order = [j for j in np.lexsort((np.arange(M), d[i])) if j != i][:k]
        idx[i, :len(order)] = order
    return idx


def bind_numpy(xyz, nx, kb, mask=None):
    """(idx int32 [P,kb], dist2 float32 [P,kb]): knn.query restated (fp32 distances, -1 / +inf tails and unselected rows)"""
    P, n = xyz.shape[0], nx.shape[0]
    idx = np.full((P, kb), -1, dtype=np.int32)
    d2 = np.full((P, kb), np.inf, dtype=np.float32)
    if n and P:
        d = ((xyz[:, None, :].astype(np.float32) - nx[None, :, :].astype(np.float32)) ** 2).sum(-1).astype(np.float32)
        for i in range(P):
            if mask is not None and not mask[i]:
                continue
            order = np.lexsort((np.arange(n), d[i]))[:kb]
            idx[i, :len(order)] = order
            d2[i, :len(order)] = d[i, order]
    return idx, d2


def axis_angle(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(deg) / 2
    return np.concatenate([[math.cos(h)], math.sin(h) * a])


def quat_matrix(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def bar(M, seed, length=4.0, width=0.5):
    """M points in a bar along x, jittered: a regular lattice has ties and degenerate neighbourhoods, a jittered one has neither"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0, length, M), rng.uniform(-width, width, M), rng.uniform(-width, width, M)], axis=1)
    return x[np.argsort(x[:, 0])].astype(np.float32)


def _handle(x, frac_lo, frac_hi, q=None, t=(0, 0, 0), pivot=None):
    """(constrained uint8 [M], target float32 [M,3]): the low end pinned in place, the high end moved by x -> p + t + R (x - p)"""
    lo, hi = x[:, 0].min(), x[:, 0].max()
    s = (x[:, 0] - lo) / (hi - lo)
    fixed, moved = s <= frac_lo, s >= frac_hi
    target = x.astype(np.float64).copy()
    R = np.eye(3) if q is None else quat_matrix(q)
    p = np.array([hi, 0.0, 0.0]) if pivot is None else np.asarray(pivot, dtype=np.float64)
    target[moved] = (x[moved].astype(np.float64) - p) @ R.T + p + np.asarray(t, dtype=np.float64)
    return (fixed | moved).astype(np.uint8), target.astype(np.float32)


def twist_warm(x, frac_lo, frac_hi, deg):
    """(y0 float32 [M,3], q0 float32 [M,4]): the bar twisted about its axis through (hi, 0, 0) by an angle that grows linearly from
    0 at frac_lo to `deg` at frac_hi -- exact on both ends of _handle(x, frac_lo, frac_hi, the same turn)"""
    lo, hi = x[:, 0].min(), x[:, 0].max()
    s = np.clip(((x[:, 0] - lo) / (hi - lo) - frac_lo) / (frac_hi - frac_lo), 0, 1)
    p = np.array([hi, 0.0, 0.0])
    y, q = np.empty(x.shape), np.empty((len(x), 4))
    for i in range(len(x)):
        q[i] = axis_angle((1, 0, 0), deg * s[i])
        y[i] = quat_matrix(q[i]) @ (x[i].astype(np.float64) - p) + p
    return y.astype(np.float32), q.astype(np.float32)


def _case(name, x, idx, weight=None, constrained=None, target=None, y0=None, q0=None):
    return dict(name=name, x=np.ascontiguousarray(x, dtype=np.float32), idx=np.ascontiguousarray(idx, dtype=np.int32), weight=weight,
                constrained=constrained, target=target, y0=y0, q0=q0)


def hostile_graph():
    """M = 300, k = 8: -1 tails, ids out of range, self and duplicate edges, an isolated node, two coincident nodes, a collinear
    run, and a hub that more than 100 rows point at; Gaussian weights"""
    M, k = 300, 8
    x = bar(M, 11, length=6.0).astype(np.float32)
    x[41] = x[40]                                   # two coincident nodes
    x[60:66] = x[60] + np.arange(6, dtype=np.float32)[:, None] * np.float32(0.125) * np.array([1, 0, 0], np.float32)  # collinear
    idx = knn_graph(x, k)
    idx[60:66] = -1
    for i in range(60, 66):                         # the collinear run sees only itself: rank-1 covariances
        idx[i, 0] = i - 1 if i > 60 else 61
        idx[i, 1] = i + 1 if i < 65 else 64
    idx[5, 3:] = -1                                 # -1 tail
    idx[6, 2], idx[6, 5] = M, -7                    # out of range
    idx[7, 1] = 7                                   # self edge
    idx[8, 4] = idx[8, 0]                           # duplicate edge
    idx[9, :] = -1                                  # isolated: no out-edge ...
    idx[idx == 9] = -1                              # ... and no in-edge
    idx[150:270, 7] = 100                           # a hub: in-degree >= 120
    d2 = ((x[:, None, :] - x[np.clip(idx, 0, M - 1)]) ** 2).sum(-1)
    weight = np.exp(-d2 / (2 * 0.5 ** 2)).astype(np.float32)
    con, tgt = _handle(x, 0.1, 0.9, axis_angle((1, 0, 0), 40.0), t=(0.0, 0.3, 0.0))
    return _case("hostile_300_k8", x, idx, weight, con, tgt)


def solve_cases():
    out = []
    one = np.array([[0.5, -1.0, 2.0]], dtype=np.float32)
    out.append(_case("one_node_free_k1", one, np.full((1, 1), -1)))
    out.append(_case("one_node_pinned_k1", one, np.full((1, 1), -1), None, np.ones(1, np.uint8), one + np.float32(0.25)))
    two = np.array([[0, 0, 0], [1, 0.5, 0]], dtype=np.float32)
    out.append(_case("two_nodes_k3", two, knn_graph(two, 3), None, np.array([1, 0], np.uint8), two + np.float32([[0, 0, 0.5], [0, 0, 0]])))
    x = bar(63, 3)
    con, tgt = _handle(x, 0.15, 0.85, None, t=(0.4, 0.5, -0.2))
    out.append(_case("translate_63_k3", x, knn_graph(x, 3), None, con, tgt))
    # A handle turned about the bar's axis with the other end pinned, from a warm start that twists the bar linearly between the
    # two: what a drag that is already under way looks like.  Started cold, the nodes between the ends see two rotations that
    # cancel, sum r_c . a_c passes through 0, omega explodes and fp32 and float64 part ways at those nodes in the first iterations
    # (quaternion differences of 0.04 .. 1 for 179 degrees): a property of the undamped iteration that no bound on a kernel can
    # be built on, so the cases start where the twin stays within 2e-7 of float64 at every checked iteration.
    for deg, M, seed in ((90.0, 64, 4), (179.0, 65, 5)):
        x = bar(M, seed)
        con, tgt = _handle(x, 0.2, 0.8, axis_angle((1, 0, 0), deg))
        warm_y, warm_q = twist_warm(x, 0.2, 0.8, deg)
        out.append(_case(f"twist{int(deg)}_warm_{M}_k8", x, knn_graph(x, 8), None, con, tgt, warm_y, warm_q))
    x = bar(65, 6)
    out.append(_case("unconstrained_65_k1", x, knn_graph(x, 1), None, None, None,
                     (x + np.random.default_rng(7).normal(0, 0.05, x.shape)).astype(np.float32)))
    out.append(hostile_graph())
    x = bar(64, 8)
    con, tgt = _handle(x, 0.2, 0.8, axis_angle((0, 0, 1), 60.0), pivot=(2.0, 0.0, 0.0))
    warm_q = np.tile(axis_angle((0, 0, 1), 20.0), (64, 1)).astype(np.float32)
    warm_y = (x.astype(np.float64) @ quat_matrix(axis_angle((0, 0, 1), 20.0)).T).astype(np.float32)
    out.append(_case("bend60_warm_64_k8", x, knn_graph(x, 8), None, con, tgt, warm_y, warm_q))
    return out


def bar_case(M=64, seed=12, k=8):
    """the bar of the energy tests: one end pinned, the other turned 90 degrees about the bar's axis"""
    x = bar(M, seed)
    con, tgt = _handle(x, 0.2, 0.8, axis_angle((1, 0, 0), 90.0))
    return _case(f"bar_{M}", x, knn_graph(x, k), None, con, tgt)


def chain_case(M=16):
    """an unconstrained chain (a bipartite graph) whose start holds the alternating mode a plain Jacobi step never damps"""
    x = np.stack([np.arange(M, dtype=np.float32), np.zeros(M, np.float32), np.zeros(M, np.float32)], axis=1)
    idx = np.full((M, 2), -1, dtype=np.int32)
    idx[1:, 0] = np.arange(M - 1)
    idx[:-1, 1] = np.arange(1, M)
    y0 = x.copy()
    y0[:, 1] = np.where(np.arange(M) % 2 == 0, 0.25, -0.25).astype(np.float32)
    return _case("chain", x, idx, None, None, None, y0)


# ---- models and node motions for the apply ---------------------------------------------------------------------------------------
def bend_nodes(nx, max_deg, seed):
    """a smooth bend about z growing along x, plus a shift; every third node's quaternion negated (q and -q are one rotation), node 0
    the exact identity"""
    rng = np.random.default_rng(seed)
    n = nx.shape[0]
    ny, nq = np.empty((n, 3), np.float32), np.empty((n, 4), np.float32)
    lo, hi = (nx[:, 0].min(), nx[:, 0].max()) if n else (0, 1)
    for a in range(n):
        s = (nx[a, 0] - lo) / max(hi - lo, 1e-6)
        q = axis_angle((0.2, 0.1, 1.0), max_deg * s)
        ny[a] = quat_matrix(q) @ nx[a].astype(np.float64) + np.array([0.1, -0.2, 0.05]) * s + rng.normal(0, 0.01, 3)
        nq[a] = (-q if a % 3 == 2 else q)
    if n:
        ny[0], nq[0] = nx[0], (1, 0, 0, 0)
    return ny, nq


def apply_cases():
    """dicts: xyz, rot, rest [P, Msh - 1, 3], nodes (x, y, q), mask (bool [P] or None), kb, sigma, spacing"""
    out = []
    shapes = [(0, 16, 4, "all"), (1, 16, 1, "all"), (63, 4, 4, "half"), (64, 9, 8, "inverted"), (65, 1, 4, "all"),
              (2000, 16, 4, "half"), (65, 16, 8, "empty"), (300, 9, 4, "few_nodes"), (64, 16, 4, "identity")]
    for P, Msh, kb, sel in shapes:
        rng = np.random.default_rng(1000 + P + Msh)
        xyz = bar(P, 20 + P) if P else np.zeros((0, 3), np.float32)
        rot = rng.normal(size=(P, 4)).astype(np.float32)
        rest = rng.normal(0, 0.3, size=(P, Msh - 1, 3)).astype(np.float32)
        mask = None
        if sel in ("half", "inverted", "few_nodes"):
            mask = rng.random(P) < 0.5
        elif sel == "empty":
            mask = np.zeros(P, bool)
        n = 0 if P == 0 else (2 if sel == "few_nodes" else max(1, min(P // 8, 40)))
        pool = np.arange(P) if mask is None or not mask.any() else np.nonzero(mask)[0]
        nx = xyz[np.sort(rng.choice(pool, size=min(n, pool.size), replace=False))] if P else np.zeros((0, 3), np.float32)
        ny, nq = bend_nodes(nx, 70.0, P)
        if sel == "identity":
            ny, nq = nx.copy(), np.tile(np.float32([1, 0, 0, 0]), (nx.shape[0], 1))
        out.append(dict(name=f"P{P}_M{Msh}_kb{kb}_{sel}", xyz=xyz, rot=rot, rest=rest, nodes=(nx, ny, nq), mask=mask, kb=kb,
                        sigma=0.4, inverted=sel == "inverted"))
    return out
