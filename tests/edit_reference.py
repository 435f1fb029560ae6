"""What goi_hyperplane_amd.edit.transform must compute, in numpy: the float32 restatement that FIXES the operation order of
csrc/edit.hip (every numpy float32 operation rounds once, as the kernel's do under -ffp-contract=off; dot products run in
index order), and the same formulas in float64 with unrounded constants, against which the running-error bounds are checked.

    x' = (s r + p) + t,  r_i = (R[i][0] d_0 + R[i][1] d_1) + R[i][2] d_2,  d = x - p        a pure translation: x + t
    q' = q_R (x) q       each component summed left to right
    scaling' = scaling + log s
    c'_i = sum_j D_l[i][j] c_j, j ascending, per band l = 1..3 and channel
    first moments: R m, q_R (x) m, D_l m (the linear part only)

The host constants (R, q_R, D_l, log s) come from goi_hyperplane_amd.edit's own float64 host code: tests/test_edit_cpu.py holds
that against tests/sh_basis_ref.py; here they are only rounded and used."""
import math

import numpy as np

from goi_hyperplane_amd import edit

U = 2.0 ** -24  # unit roundoff of fp32
BANDS = ((0, 3), (3, 5), (8, 7))  # (first coefficient of _features_rest, coefficients) of bands 1..3


def gamma(n):
    return n * U / (1 - n * U)


def constants(rotation=None, translation=None, scale=1.0, pivot=(0.0, 0.0, 0.0), dtype=np.float32):
    """The numbers the kernel is handed, in `dtype` (float32: rounded once; float64: as the host formed them)."""
    sim = edit.Similarity(rotation, translation, scale)
    D = edit.sh_rotation(sim.R, 3)
    return dict(R=sim.R.astype(dtype), q=sim.q.astype(dtype), t=sim.t.astype(dtype), p=np.asarray(pivot, np.float64).astype(dtype),
                s=dtype(sim.s), log_s=dtype(math.log(sim.s)), rotate=sim.rotate, scale=sim.scale,
                D=[D[1:4, 1:4].astype(dtype), D[4:9, 4:9].astype(dtype), D[9:16, 9:16].astype(dtype)])


def rotate3(R, v):
    return np.stack([(R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2] for i in range(3)], axis=1)


def quat_left(a, b):
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([((a[0] * b0 - a[1] * b1) - a[2] * b2) - a[3] * b3,
                     ((a[0] * b1 + a[1] * b0) + a[2] * b3) - a[3] * b2,
                     ((a[0] * b2 - a[1] * b3) + a[2] * b0) + a[3] * b1,
                     ((a[0] * b3 + a[1] * b2) - a[2] * b1) + a[3] * b0], axis=1)


def rotate_rest(D, rest):
    """rest [n, M-1, 3] -> the same shape, every stored band multiplied by its matrix"""
    out = rest.copy()
    for (first, n), Dl in zip(BANDS, D):
        if first + n > rest.shape[1]:
            break
        for i in range(n):
            acc = Dl[i, 0] * rest[:, first, :]
            for j in range(1, n):
                acc = acc + Dl[i, j] * rest[:, first + j, :]
            out[:, first + i, :] = acc
    return out


def position(c, x):
    if not (c["rotate"] or c["scale"]):
        return x + c["t"][None, :]
    r = rotate3(c["R"], x - c["p"][None, :])
    return (c["s"] * r + c["p"][None, :]) + c["t"][None, :]


def transform(arrays, sel, c):
    """arrays: {"_xyz", "_rotation", "_scaling", "_features_rest"} and optionally the first moments {"m_xyz", "m_rotation",
    "m_features_rest"}, numpy arrays of c's dtype; sel: bool [P].  Returns the edited copies (unselected rows untouched)."""
    out = {k: v.copy() for k, v in arrays.items()}
    if not sel.any():
        return out
    out["_xyz"][sel] = position(c, arrays["_xyz"][sel])
    if c["rotate"]:
        out["_rotation"][sel] = quat_left(c["q"], arrays["_rotation"][sel])
        out["_features_rest"][sel] = rotate_rest(c["D"], arrays["_features_rest"][sel])
        if "m_xyz" in arrays:
            out["m_xyz"][sel] = rotate3(c["R"], arrays["m_xyz"][sel])
        if "m_rotation" in arrays:
            out["m_rotation"][sel] = quat_left(c["q"], arrays["m_rotation"][sel])
        if "m_features_rest" in arrays:
            out["m_features_rest"][sel] = rotate_rest(c["D"], arrays["m_features_rest"][sel])
    if c["scale"]:
        out["_scaling"][sel] = arrays["_scaling"][sel] + c["log_s"]
    return out


# ---- running-error bounds of the float32 restatement against the float64 one ---------------------------------------------
# Each bound is gamma_k times the sum of the magnitudes that enter a result, k = the most roundings any term goes through
# (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), the rounding of the constants to fp32 included.
def rest_bound(c64, rest):
    """gamma_8 sum_j |D_ij| |c_j|: a band has at most 7 terms -- one rounding of D_ij, one product and at most 6 sums each"""
    mag = rotate_rest([np.abs(D) for D in c64["D"]], np.abs(rest))
    return gamma(8) * mag


def position_bound(c64, x):
    """A term of s R (x - p) is rounded at most 8 times (p, the difference, R_ij, the product, two sums, s, the product with
    s), then come the sums with p and t (and t's own rounding): gamma_12 over every magnitude that enters covers all of it."""
    if not (c64["rotate"] or c64["scale"]):
        return gamma(2) * (np.abs(x) + np.abs(c64["t"])[None, :])
    mag = c64["s"] * rotate3(np.abs(c64["R"]), np.abs(x) + np.abs(c64["p"])[None, :]) + np.abs(c64["p"])[None, :] + \
        np.abs(c64["t"])[None, :]
    return gamma(12) * mag


def quat_bound(c64, q):
    """four terms: one rounding of q_R's component, one product, at most three sums"""
    return gamma(5) * _abs_quat(np.abs(c64["q"]), np.abs(q))


def _abs_quat(a, b):
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([a[0] * b0 + a[1] * b1 + a[2] * b2 + a[3] * b3, a[0] * b1 + a[1] * b0 + a[2] * b3 + a[3] * b2,
                     a[0] * b2 + a[1] * b3 + a[2] * b0 + a[3] * b1, a[0] * b3 + a[1] * b2 + a[2] * b1 + a[3] * b0], axis=1)


# ---- models -----------------------------------------------------------------------------------------------------------------
MOMENTS = (("xyz", "_xyz", "m_xyz"), ("rotation", "_rotation", "m_rotation"), ("f_rest", "_features_rest", "m_features_rest"))


def arrays_of(g):
    """the numpy arrays transform() takes, from a model (tensors on any device), with the first moments its optimizer holds"""
    out = {attr: getattr(g, attr).detach().cpu().numpy().copy() for attr in ("_xyz", "_rotation", "_scaling", "_features_rest")}
    if getattr(g, "optimizer", None) is not None:
        names = {grp["name"] for grp in g.optimizer.param_groups}
        for name, attr, key in MOMENTS:
            st = g.optimizer.state.get(getattr(g, attr), None) if name in names else None
            if st and "exp_avg" in st:
                out[key] = st["exp_avg"].detach().cpu().numpy().copy()
    return out


def random_rotation(seed):
    """float64 [3, 3], a proper rotation from a seeded unit quaternion"""
    q = np.random.default_rng(seed).normal(size=4)
    return edit._quat_to_matrix(q / np.linalg.norm(q))
