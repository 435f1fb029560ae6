"""A numpy restatement of the PCA stage (goi_hyperplane_amd/pca.py, csrc/pca.hip): what sklearn.decomposition.PCA(3)
computes for these shapes (its covariance_eigh solver), and the three display normalisations.

    fit(rows, mask=None, dtype=float64)   masked mean, covariance with divisor n - 1, eigh, the three largest eigenpairs
                                          in descending order, the entry of largest magnitude of each component positive
                                          (sklearn >= 1.5: svd_flip(u_based_decision=False)), negative eigenvalues
                                          clipped to 0.  dtype=float32 runs the same steps in float32: its distance from
                                          the float64 run is the yardstick for a float32 implementation's error.
    project(rows, basis)                  (x - mean) . components, float64
    sigma(q, explained_variance, k)       float32, one rounding per operation, as the kernel writes them
    minmax(q)

tests/test_pca_cpu.py holds fit and project to sklearn's own results (tests/golden/ref_pca_pins.npz)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Basis = namedtuple("Basis", "mean components explained_variance total_variance count")
F32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny
EPS32 = float(np.finfo(np.float32).eps)


def fit(rows, mask=None, dtype=np.float64) -> Basis:
    """rows [n, S]; mask [n] (nonzero = use) or None."""
    X = np.asarray(rows)
    if mask is not None:
        X = X[np.asarray(mask).reshape(-1) != 0]
    X = X.astype(dtype)
    n, S = X.shape
    if n < 2:
        mean = X[0].copy() if n == 1 else np.zeros(S, dtype)
        return Basis(mean, np.zeros((3, S), dtype), np.zeros(3, dtype), dtype(0), n)
    mean = X.mean(axis=0, dtype=dtype)
    Xc = X - mean
    cov = (Xc.T @ Xc) / dtype(n - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind="stable")[:3]
    comps = v[:, order].T.copy()
    for k in range(3):
        if comps[k, np.argmax(np.abs(comps[k]))] < 0:
            comps[k] = -comps[k]
    return Basis(mean, comps, np.maximum(w[order], 0), np.trace(cov), n)


def eigenvalues(rows, mask=None):
    """All eigenvalues of the float64 covariance, descending: how well conditioned a case's top three directions are."""
    X = np.asarray(rows, np.float64)
    if mask is not None:
        X = X[np.asarray(mask).reshape(-1) != 0]
    Xc = X - X.mean(axis=0)
    return np.sort(np.linalg.eigvalsh(Xc.T @ Xc / (len(X) - 1)))[::-1]


def project(rows, basis) -> np.ndarray:
    """[n, 3] float64: what PCA.transform returns."""
    return (np.asarray(rows, np.float64) - np.asarray(basis.mean, np.float64)) @ np.asarray(basis.components, np.float64).T


def sigma(q, explained_variance, k=2.0) -> np.ndarray:
    """q [..., 3] float32 (component last), explained_variance [3] float32 ->
    clamp(0.5 + q / ((2 k) * max(sqrt(ev), FLT_MIN)), 0, 1); a NaN gives 0 (fmaxf / fminf drop it)."""
    q = np.asarray(q, F32)
    ev = np.asarray(explained_variance, F32)
    den = F32(F32(2.0) * F32(k)) * np.maximum(np.sqrt(ev, dtype=F32), F32(FLT_MIN))
    with np.errstate(all="ignore"):
        v = (q / den).astype(F32)
        v = (F32(0.5) + v).astype(F32)
        return np.fmin(np.fmax(v, F32(0)), F32(1)).astype(F32)


def minmax(q) -> np.ndarray:
    """q [n, 3] float32 of ONE view -> (q - min) / ((max - min) + 1e-20f) per component, NaNs skipped by min and max."""
    q = np.asarray(q, F32)
    with np.errstate(all="ignore"):
        mn = np.nanmin(q, axis=0).astype(F32)
        mx = np.nanmax(q, axis=0).astype(F32)
        den = ((mx - mn).astype(F32) + F32(1e-20)).astype(F32)
        return ((q - mn).astype(F32) / den).astype(F32)


def sample(S, n, seed, offset=0.0):
    """[n, S] float32 rows whose covariance has the spectrum 16, 4, 1, 1/4 and then 1/100 and below along random
    orthogonal directions (population ratios of 4 between the top four, so a finite sample keeps them well apart), about
    a mean of a few tenths; offset: every channel moved by `offset` times its standard deviation."""
    rng = np.random.default_rng(seed)
    scales = np.concatenate([[4.0, 2.0, 1.0, 0.5], 0.1 / (1.0 + np.arange(max(S - 4, 0)))])[:S]
    Q, _ = np.linalg.qr(rng.normal(size=(S, S)))
    x = (rng.normal(size=(n, S)) * scales) @ Q.T + rng.uniform(-0.3, 0.3, S)
    if offset:
        x = x + offset * np.sqrt(np.diag((Q * scales ** 2) @ Q.T))
    return x.astype(np.float32)
