"""A numpy restatement of csrc/deform.hip, parametrised by dtype.  Run in float64 it is the reference; run in float32 it is the
"float32 twin": the kernel's operations in the kernel's order, one rounding each, so that the twin's distance from the float64
run measures what fp32 arithmetic costs on a case.  The GPU tests hold the kernels within 8 x that distance (or 64 ulps of the
case's coordinate scale, whichever is larger) of the float64 run.

Everything is vectorised over the nodes / Gaussians and loops over the slots of a row, so a row's sums run in the kernel's order."""
import numpy as np

from goi_hyperplane_amd import deform, edit
from goi_hyperplane_amd.render import SH_C1, SH_C2, SH_C3


# ---- quaternions ------------------------------------------------------------------------------------------------------------------
def quat_matrix(q, minus_identity=False):
    """[n,4] (w, x, y, z) -> [n,3,3]; with minus_identity R - I formed from the quaternion's terms"""
    dt = q.dtype.type
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    two = dt(2)
    if minus_identity:
        d0, d1, d2 = -two * (yy + zz), -two * (xx + zz), -two * (xx + yy)
    else:
        d0, d1, d2 = dt(1) - two * (yy + zz), dt(1) - two * (xx + zz), dt(1) - two * (xx + yy)
    R = np.empty((q.shape[0], 3, 3), dtype=q.dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = d0, two * (xy - wz), two * (xz + wy)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = two * (xy + wz), d1, two * (yz - wx)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = two * (xz - wy), two * (yz + wx), d2
    return R


def rotate3(R, v):
    """[n,3,3], [n,3] -> [n,3], each component (R0 v0 + R1 v1) + R2 v2"""
    return np.stack([(R[:, i, 0] * v[:, 0] + R[:, i, 1] * v[:, 1]) + R[:, i, 2] * v[:, 2] for i in range(3)], axis=1)


def quat_left(a, b):
    """a (x) b, rows of (w, x, y, z), each component summed left to right"""
    return np.stack([((a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1]) - a[:, 2] * b[:, 2]) - a[:, 3] * b[:, 3],
                     ((a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]) + a[:, 2] * b[:, 3]) - a[:, 3] * b[:, 2],
                     ((a[:, 0] * b[:, 2] - a[:, 1] * b[:, 3]) + a[:, 2] * b[:, 0]) + a[:, 3] * b[:, 1],
                     ((a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2]) - a[:, 2] * b[:, 1]) + a[:, 3] * b[:, 0]], axis=1)


def quat_normalize(q):
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    ok = (n > 0) & np.isfinite(n)
    with np.errstate(all="ignore"):
        return np.where(ok[:, None], q / np.where(ok, n, 1)[:, None], q)


# ---- the graph --------------------------------------------------------------------------------------------------------------------
def edges(idx):
    """bool [M,k]: entry (i, m) is an edge iff 0 <= idx[i,m] < M and idx[i,m] != i"""
    M = idx.shape[0]
    return (idx >= 0) & (idx < M) & (idx != np.arange(M)[:, None])


def transpose(idx):
    """smooth.transpose restated: (in_ptr [M+1], in_edge [M*k]) over the entries with 0 <= idx < M (self edges included)"""
    M, k = idx.shape
    flat = idx.reshape(-1).astype(np.int64)
    e = np.nonzero((flat >= 0) & (flat < M))[0]
    order = e[np.argsort(flat[e], kind="stable")]
    in_ptr = np.zeros(M + 1, dtype=np.int32)
    np.cumsum(np.bincount(flat[e], minlength=M), out=in_ptr[1:])
    in_edge = np.full(M * k, -1, dtype=np.int32)
    in_edge[:order.size] = order
    return in_ptr, in_edge


def _weights(weight, idx, dt):
    return np.ones(idx.shape, dtype=dt) if weight is None else np.asarray(weight).astype(dt)


def position_step(x, idx, weight, transposed, constrained, target, relax, y, q):
    """one Jacobi step of the positions from the old y and q; every array of y's dtype"""
    dt = y.dtype.type
    M, k = idx.shape
    w_all = _weights(weight, idx, dt)
    ok = edges(idx)
    R = quat_matrix(q)
    acc = np.zeros((M, 3), dtype=dt)
    W = np.zeros(M, dtype=dt)
    rows = np.arange(M)
    for m in range(k):
        use = ok[:, m]
        j = np.where(use, idx[:, m], rows)
        w = w_all[:, m]
        r = rotate3(R, x - x[j])
        acc = np.where(use[:, None], acc + w[:, None] * ((y[j] - y) + r), acc)
        W = np.where(use, W + w, W)
    in_ptr, in_edge = transposed
    n = M * k
    lo = np.clip(in_ptr[:-1], 0, n)
    hi = np.clip(np.maximum(in_ptr[1:], lo), 0, n)
    wf = w_all.reshape(-1)
    for r_ in range(int((hi - lo).max()) if M else 0):
        has = lo + r_ < hi
        e = np.where(has, in_edge[np.minimum(lo + r_, n - 1)], -1)
        has &= (e >= 0) & (e < n)
        e = np.where(has, e, 0)
        src = e // k
        has &= src != rows
        src = np.where(has, src, rows)
        w = wf[e]
        r = rotate3(R[src], x[src] - x)
        acc = np.where(has[:, None], acc + w[:, None] * ((y[src] - y) - r), acc)
        W = np.where(has, W + w, W)
    free = W > 0
    with np.errstate(all="ignore"):
        step = dt(relax) * (acc / np.where(free, W, 1)[:, None])  # y + relax (yhat - y): exact zeros on an undeformed graph
    out = np.where(free[:, None] & (step != 0), y + step, y)
    if constrained is not None:
        out = np.where(np.asarray(constrained).astype(bool)[:, None], np.asarray(target).astype(dt), out)
    return out


def covariance(x, idx, weight, y):
    """A_i = sum over out-edges of w (y_i - y_j)(x_i - x_j)^T, [M,3,3], slots in row order"""
    dt = y.dtype.type
    M, k = idx.shape
    w_all = _weights(weight, idx, dt)
    ok = edges(idx)
    rows = np.arange(M)
    A = np.zeros((M, 3, 3), dtype=dt)
    for m in range(k):
        use = ok[:, m]
        j = np.where(use, idx[:, m], rows)
        dd = (y - y[j])[:, :, None] * (x - x[j])[:, None, :]
        A = np.where(use[:, None, None], A + w_all[:, m][:, None, None] * dd, A)
    return A


def polar_steps(A, q, polar_iters):
    """polar_iters steps of omega = (sum_c r_c x a_c) / (|sum_c r_c . a_c| + 1e-9), q <- normalize(exp(omega) (x) q)"""
    dt = q.dtype.type
    q = q.copy()
    for _ in range(polar_iters):
        R = quat_matrix(q)
        t = np.zeros((q.shape[0], 3), dtype=dt)
        s = np.zeros(q.shape[0], dtype=dt)
        for c in range(3):
            r0, r1, r2, a0, a1, a2 = R[:, 0, c], R[:, 1, c], R[:, 2, c], A[:, 0, c], A[:, 1, c], A[:, 2, c]
            t = t + np.stack([r1 * a2 - r2 * a1, r2 * a0 - r0 * a2, r0 * a1 - r1 * a0], axis=1)
            s = s + ((r0 * a0 + r1 * a1) + r2 * a2)
        om = t / (np.abs(s) + dt(1e-9))[:, None]
        th = np.sqrt((om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1]) + om[:, 2] * om[:, 2])
        go = (th > 0) & np.isfinite(th)  # (no torque, or an omega that overflowed: q stays)
        th1 = np.where(go, th, 1).astype(dt)
        h = dt(0.5) * th1
        f = np.sin(h) / th1
        dq = np.concatenate([np.cos(h)[:, None], f[:, None] * om], axis=1).astype(dt)
        q = np.where(go[:, None], quat_normalize(quat_left(dq, q)), q)
    return q


def rotation_step(x, idx, weight, y, q, polar_iters):
    return polar_steps(covariance(x, idx, weight, y), q, polar_iters)


def solve(x, idx, weight, constrained, target, y0=None, q0=None, iterations=10, polar_iters=4, relax=0.8, dtype=np.float64):
    """-> (y, q) of `dtype` after `iterations` iterations of (positions, rotations) from the warm start"""
    x = np.asarray(x).astype(dtype)
    M = x.shape[0]
    y = x.copy() if y0 is None else np.asarray(y0).astype(dtype)
    q = np.tile(np.array([1, 0, 0, 0], dtype=dtype), (M, 1)) if q0 is None else np.asarray(q0).astype(dtype)
    if M == 0:
        return y, q
    T = transpose(idx)
    for _ in range(iterations):
        y = position_step(x, idx, weight, T, constrained, target, relax, y, q)
        q = rotation_step(x, idx, weight, y, q, polar_iters)
    return y, q


def energy(x, idx, weight, y, q):
    """E in float64 from inputs of any dtype"""
    x, y, q = (np.asarray(a).astype(np.float64) for a in (x, y, q))
    M, k = idx.shape
    if M == 0:
        return 0.0
    w_all = _weights(weight, idx, np.float64)
    ok = edges(idx)
    R = quat_matrix(q)
    rows = np.arange(M)
    total = np.zeros(M)
    for m in range(k):
        j = np.where(ok[:, m], idx[:, m], rows)
        d = (y - y[j]) - rotate3(R, x - x[j])
        total += np.where(ok[:, m], w_all[:, m] * (d * d).sum(axis=1), 0.0)
    return float(total.sum())


# ---- the apply --------------------------------------------------------------------------------------------------------------------
def bind_weights(bidx, bd2, n_nodes, sigma, dtype):
    """(used bool [P,kb], first int [P] (-1: none), w [P,kb] normalised, 0 where unused)"""
    dt = np.dtype(dtype).type
    P, kb = bidx.shape
    d = np.asarray(bd2).astype(dtype)
    used = (bidx >= 0) & (bidx < n_nodes) & np.isfinite(np.asarray(bd2))
    first = np.where(used.any(axis=1), used.argmax(axis=1), -1)
    d0 = d[np.arange(P), np.maximum(first, 0)]
    c = dt(1.0 / (2.0 * float(sigma) * float(sigma)))
    w = np.zeros((P, kb), dtype=dtype)
    wsum = np.zeros(P, dtype=dtype)
    with np.errstate(all="ignore"):
        for m in range(kb):
            wm = np.exp(-((np.where(used[:, m], d[:, m], d0) - d0) * c)).astype(dtype)
            w[:, m] = np.where(used[:, m], wm, 0)
            wsum = np.where(used[:, m], wsum + wm, wsum)
        w = np.where(used, w / np.where(wsum > 0, wsum, 1)[:, None], 0).astype(dtype)
    return used, first, w


def blended_rotation(bidx, used, first, w, nq):
    """q_g [P,4] = normalize(sum_a w_a s_a q_a) (the identity for a row without a node) and turn bool [P]: a non-zero vector part"""
    dt = nq.dtype.type
    P, kb = bidx.shape
    q1 = nq[np.where(first >= 0, bidx[np.arange(P), np.maximum(first, 0)], 0)] if nq.shape[0] else np.zeros((P, 4), dtype=nq.dtype)
    qg = np.zeros((P, 4), dtype=nq.dtype)
    for m in range(kb):
        u = used[:, m]
        qa = nq[np.where(u, bidx[:, m], 0)] if nq.shape[0] else qg
        dot = ((qa[:, 0] * q1[:, 0] + qa[:, 1] * q1[:, 1]) + qa[:, 2] * q1[:, 2]) + qa[:, 3] * q1[:, 3]
        ws = np.where(dot < 0, -w[:, m], w[:, m])
        qg = np.where(u[:, None], qg + ws[:, None] * qa, qg)
    qg = quat_normalize(qg)
    bound = first >= 0
    qg = np.where(bound[:, None], qg, np.array([1, 0, 0, 0], dtype=dt))
    return qg, bound & ((qg[:, 1] != 0) | (qg[:, 2] != 0) | (qg[:, 3] != 0))


def sh_band(u, l):
    """band l of the basis at unit directions u [n,3] -> [n, 2l+1], the kernel's expressions"""
    dt = u.dtype.type
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    if l == 1:
        return np.stack([-dt(SH_C1) * y, dt(SH_C1) * z, -dt(SH_C1) * x], axis=1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 2:
        c = [dt(v) for v in SH_C2]
        return np.stack([c[0] * xy, c[1] * yz, c[2] * ((dt(2) * zz - xx) - yy), c[3] * xz, c[4] * (xx - yy)], axis=1)
    c = [dt(v) for v in SH_C3]
    return np.stack([c[0] * y * (dt(3) * xx - yy), c[1] * xy * z, c[2] * y * ((dt(4) * zz - xx) - yy),
                     c[3] * z * ((dt(2) * zz - dt(3) * xx) - dt(3) * yy), c[4] * x * ((dt(4) * zz - xx) - yy), c[5] * z * (xx - yy),
                     c[6] * x * (xx - dt(3) * yy)], axis=1)


def lane_rotate_bands(R, coeff):
    """the per-lane construction: coeff [n, M-1, 3] -> D_l(R) coeff per band and channel, R [n,3,3]; coeff's dtype"""
    dtype = coeff.dtype
    out = coeff.copy()
    for l, (dirs, inv) in enumerate(deform.sh_constants(), start=1):
        first, N = l * l - 1, 2 * l + 1
        if first + N > coeff.shape[1]:
            break
        dirs, inv = dirs.astype(dtype), inv.astype(dtype)
        v = []
        for n in range(N):
            d = dirs[n]
            u = np.stack([(R[:, 0, j] * d[0] + R[:, 1, j] * d[1]) + R[:, 2, j] * d[2] for j in range(3)], axis=1)  # R^T d
            b = sh_band(u, l)
            acc = b[:, 0, None] * coeff[:, first, :]
            for k in range(1, N):
                acc = acc + b[:, k, None] * coeff[:, first + k, :]
            v.append(acc)
        for i in range(N):
            acc = inv[i, 0] * v[0]
            for n in range(1, N):
                acc = acc + inv[i, n] * v[n]
            out[:, first + i, :] = acc
    return out


def lane_sh_rotation(R):
    """float64 [16,16]: the matrix the per-lane construction multiplies by, for one rotation R [3,3]"""
    D = np.zeros((16, 16))
    D[0, 0] = 1.0
    eye = np.eye(15)
    for col in range(15):
        c = np.zeros((1, 15, 3))
        c[0, :, 0] = eye[col]
        D[1:, 1 + col] = lane_rotate_bands(np.asarray(R, dtype=np.float64)[None], c)[0, :, 0]
    return D


def host_rotate_bands(R, coeff):
    """float64: coeff [n, M-1, 3] times edit.sh_rotation(R_n) per row"""
    out = coeff.astype(np.float64).copy()
    nb = coeff.shape[1]
    deg = {0: 0, 3: 1, 8: 2, 15: 3}[nb]
    for i in range(coeff.shape[0]):
        D = edit.sh_rotation(_polar(R[i]), deg)[1:, 1:]
        out[i] = D @ coeff[i].astype(np.float64)
    return out


def _polar(R):
    """the nearest exact rotation (edit.sh_rotation refuses a matrix that is off by more than 1e-6)"""
    u, _, vt = np.linalg.svd(np.asarray(R, dtype=np.float64))
    return u @ vt


def apply(xyz, rotation, rest, bidx, bd2, nodes, sigma, mask=None, dtype=np.float64, sh="lane"):
    """-> (xyz', rotation', rest', q_g, turn) of `dtype`: goi_deform_apply with moments = 0 on copies.  mask: bool [P] of the
    selected rows (None: all).  sh = "lane": the kernel's construction in `dtype`; "host": edit.sh_rotation(R_g) in float64."""
    dt = np.dtype(dtype).type
    nx, ny, nq = (np.asarray(a).astype(dtype) for a in nodes)
    x, r, c = (np.asarray(a).astype(dtype) for a in (xyz, rotation, rest))
    P, kb = bidx.shape
    used, first, w = bind_weights(bidx, bd2, nx.shape[0], sigma, dtype)
    if mask is not None:
        used = used & np.asarray(mask).astype(bool)[:, None]
        first = np.where(np.asarray(mask).astype(bool), first, -1)
    qg, turn = blended_rotation(bidx, used, first, w, nq)
    acc = np.zeros((P, 3), dtype=dtype)
    for m in range(kb):
        u = used[:, m]
        a = np.where(u, bidx[:, m], 0)
        if nx.shape[0] == 0:
            break
        Rm = quat_matrix(nq[a], minus_identity=True)
        term = (ny[a] - nx[a]) + rotate3(Rm, x - nx[a])
        acc = np.where(u[:, None], acc + w[:, m][:, None] * term, acc)
    x_new = np.where(acc == 0, x, x + acc)
    Rg = quat_matrix(qg)
    r_new = np.where(turn[:, None], quat_left(qg, r), r)
    if c.shape[1] == 0:
        c_new = c
    elif sh == "lane":
        c_new = np.where(turn[:, None, None], lane_rotate_bands(Rg, c), c)
    else:
        c_new = c.copy()
        rows = np.nonzero(turn)[0]
        c_new[rows] = host_rotate_bands(Rg[rows], c[rows])
    return x_new.astype(dtype), r_new.astype(dtype), c_new.astype(dtype), qg, turn


def turn_moments(m_xyz, m_rot, m_rest, qg, turn, dtype=np.float64, sh="lane"):
    """the moment turn of commit(): R_g m, q_g (x) m, D_l m on the rows with `turn`"""
    qg = qg.astype(dtype)
    Rg = quat_matrix(qg)
    mx, mr, mc = (np.asarray(a).astype(dtype) for a in (m_xyz, m_rot, m_rest))
    mx = np.where(turn[:, None], rotate3(Rg, mx), mx)
    mr = np.where(turn[:, None], quat_left(qg, mr), mr)
    if mc.shape[1]:
        if sh == "lane":
            mc = np.where(turn[:, None, None], lane_rotate_bands(Rg, mc), mc)
        else:
            rows = np.nonzero(turn)[0]
            mc = mc.copy()
            mc[rows] = host_rotate_bands(Rg[rows], mc[rows])
    return mx, mr, mc


# ---- sample_nodes -----------------------------------------------------------------------------------------------------------------
def sample_nodes(xyz, mask, spacing):
    """int64 ids, ascending: the lowest selected id of every occupied cube, the lattice anchored at the selection's lo, fp32"""
    xyz = np.asarray(xyz, dtype=np.float32)
    ids = np.arange(xyz.shape[0]) if mask is None else np.nonzero(np.asarray(mask).astype(bool))[0]
    if ids.size == 0:
        return ids.astype(np.int64)
    pts = xyz[ids]
    cells = np.floor((pts - pts.min(axis=0)) / np.float32(spacing)).astype(np.int64)
    seen = {}
    for i, c in zip(ids.tolist(), map(tuple, cells.tolist())):
        seen.setdefault(c, i)
    return np.array(sorted(seen.values()), dtype=np.int64)
