"""The two entries of csrc/mcmc.hip restated in numpy (include/goi_raster.h spells the definitions): the sampling in Python
integers, the row arithmetic in float64 in the stated order, one operation per line where the order matters.

    relocate(opacity, draws, selection, min_opacity, max_moves, frac, n_max, groups) -> dict
    noise(xyz, rotation, scaling, opacity, z, selection, k, x0, step) -> new xyz as float64 (the caller rounds)

`groups` is a list of (array [P, row_len] float32, mode) in the entry's order; the arrays are not modified, the dict holds
their new values ("groups"), the float64 values the device rounds once ("opacity64" / "scale64" by source row), counts, hits,
the dead ids, the sources of the draws, and o', D, c by source row."""
import math

import numpy as np

PARAM, OPACITY, SCALING, MOMENT = 0, 1, 2, 3
N_MAX = 51
ONE_LESS = 1.0 - 2.0 ** -24
BINOM = [[float(math.comb(n, k)) for k in range(N_MAX)] for n in range(N_MAX)]
Q = [1.0 / math.sqrt(float(k + 1)) for k in range(N_MAX)]


def classify(opacity, selection, min_opacity):
    """(w [P] Python ints, dead [P] bool, alive [P] bool)"""
    op = np.asarray(opacity, np.float32)
    sel = np.ones(op.shape, bool) if selection is None else np.asarray(selection) != 0
    o64 = op.astype(np.float64)
    with np.errstate(invalid="ignore"):
        dead = sel & (o64 <= min_opacity)
        alive = sel & (o64 > min_opacity)
    w = [int(min(float(o), 1.0) * 16777216.0) if a and float(o) > 0.0 else 0 for o, a in zip(op, alive)]
    return w, dead, alive


def relocation_sum(o_new, N):
    """D: one accumulator, m outer, k inner, the running power restarted for every m, odd k subtracted"""
    o_new = float(o_new)
    D = 0.0
    for m in range(1, N + 1):
        p = 1.0
        for k in range(m):
            p = p * o_new
            term = (BINOM[m - 1][k] * Q[k]) * p
            D = D - term if k & 1 else D + term
    return D


def new_values(opacity, N, min_opacity):
    """(o, o', D, c, new raw opacity as float64) of a source"""
    o = min(float(np.float64(np.float32(opacity))), ONE_LESS)
    o_new = o if N == 1 else 1.0 - float(np.power(np.float64(1.0 - o), np.float64(1.0 / float(N))))
    D = relocation_sum(o_new, N)
    c = o / D
    x = min(max(o_new, min_opacity), ONE_LESS)
    return o, o_new, D, c, float(np.log(np.float64(x / (1.0 - x))))


def sample(opacity, draws, selection, min_opacity, max_moves, frac, n_max=N_MAX):
    w, dead, alive = classify(opacity, selection, min_opacity)
    P = len(w)
    C, run = [], 0
    for x in w:
        run += x
        C.append(run)
    T = run
    dead_ids = [i for i in range(P) if dead[i]]
    n_dead, n_alive = len(dead_ids), int(alive.sum())
    moves = min(n_dead, len(draws), int(max_moves), n_alive * int(frac[0]) // int(frac[1]))
    if T == 0:
        moves = 0
    src, hits = [], [0] * P
    for j in range(moves):
        u = int(draws[j]) & 0xFFFFFFFF
        t = (u * T) >> 32
        lo, hi = 0, P - 1
        while lo < hi:  # min{ i : C_i > t }
            mid = (lo + hi) // 2
            if C[mid] > t:
                hi = mid
            else:
                lo = mid + 1
        src.append(lo)
        hits[lo] += 1
    return {"w": w, "C": C, "T": T, "dead": dead_ids, "alive": alive, "moves": moves, "src": src, "hits": hits,
            "counts": [moves, n_dead, n_alive, sum(1 for h in hits if h)]}


def relocate(opacity, draws, selection, min_opacity, max_moves, frac, n_max, groups):
    s = sample(opacity, draws, selection, min_opacity, max_moves, frac, n_max)
    out = [np.array(a, np.float32, copy=True) for a, _ in groups]
    scaling = next((np.asarray(a, np.float32) for a, m in groups if m == SCALING), None)
    values, op64, sc64 = {}, {}, {}
    for i, r in enumerate(s["hits"]):
        if r:
            N = min(r + 1, n_max)
            o, o_new, D, c, raw = new_values(opacity[i], N, min_opacity)
            values[i] = {"N": N, "o": o, "o_new": o_new, "D": D, "c": c}
            op64[i] = raw
            if scaling is not None:
                lc = float(np.log(np.float64(c)))
                sc64[i] = [float(np.float64(scaling[i, a])) + lc for a in range(3)]
    for (a, mode), new in zip(groups, out):
        old = np.asarray(a, np.float32)
        for j, sj in enumerate(s["src"]):
            d = s["dead"][j]
            if mode == PARAM:
                new[d] = old[sj]
            elif mode == OPACITY:
                new[d] = np.float32(op64[sj])
            elif mode == SCALING:
                new[d] = np.asarray(sc64[sj], np.float64).astype(np.float32)
        for i in values:
            if mode == OPACITY:
                new[i] = np.float32(op64[i])
            elif mode == SCALING:
                new[i] = np.asarray(sc64[i], np.float64).astype(np.float32)
            elif mode == MOMENT:
                new[i] = 0.0
    s.update({"groups": out, "values": values, "opacity64": op64, "scale64": sc64})
    return s


def rotation(q):
    """build_rotation of one raw quaternion (r, x, y, z) in float64: squares summed left to right, then q / norm"""
    q0, q1, q2, q3 = (float(v) for v in q)
    n = math.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
    r, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)],
            [2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)],
            [2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]]


def gate(opacity, k, x0):
    return 1.0 / (1.0 + float(np.exp(np.float64(-k * ((1.0 - float(opacity)) - x0)))))


def noise(xyz, rot, scaling, opacity, z, selection, k, x0, step):
    """new xyz [P, 3] as float64 (frozen rows: the old values, exactly)"""
    xyz = np.asarray(xyz, np.float32)
    out = xyz.astype(np.float64)
    with np.errstate(all="ignore"):
        for i in range(xyz.shape[0]):
            if selection is not None and not selection[i]:
                continue
            R = rotation(rot[i])
            g = gate(np.float32(opacity[i]), k, x0)
            s = [float(np.exp(np.float64(np.float32(scaling[i, b])))) for b in range(3)]
            M = [[R[a][b] * s[b] for b in range(3)] for a in range(3)]
            v = [(float(np.float32(z[i, b])) * g) * step for b in range(3)]
            for a in range(3):
                delta = 0.0
                for c in range(3):
                    sig = M[a][0] * M[c][0] + M[a][1] * M[c][1] + M[a][2] * M[c][2]
                    delta = sig * v[0] if c == 0 else delta + sig * v[c]
                out[i, a] = float(xyz[i, a]) + delta
    return out
