"""Writes tests/golden/ref_dbscan_pins.npz: sklearn.cluster.DBSCAN(eps, min_samples).fit(X) labels and core indices on
point sets that pin every rule of csrc/dbscan.hip (run where sklearn is installed; the tests only read the file).

Points lie on a 2^-10 lattice and are stored as int32 multiples of 2^-10, so every near pair's d2 is exact in fp32 and in
float64 and the GPU must match sklearn exactly.  For each case the generator asserts that no pair's d2 lies within
1e-5 * eps^2 of eps^2, so no decision depends on rounding.

    python tests/golden/make_dbscan_golden.py
"""
from __future__ import annotations

import os

import numpy as np

UNIT = 2.0 ** -10
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_dbscan_pins.npz")


def lattice(x):
    return np.round(np.asarray(x, np.float64) / UNIT).astype(np.int32)


def blobs(rng, n, centers, spread, extent, noise):
    n_noise = int(n * noise)
    c = rng.uniform(-extent, extent, size=(centers, 3))
    which = rng.integers(0, centers, size=n - n_noise)
    pts = np.concatenate([c[which] + rng.normal(0.0, spread, size=(n - n_noise, 3)),
                          rng.uniform(-extent - 1, extent + 1, size=(n_noise, 3))])
    return lattice(pts[rng.permutation(n)])


def cube(center, side, k):
    """k^3 points on a regular grid of the given side around center."""
    g = np.linspace(-side / 2, side / 2, k)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.asarray(center, np.float64)


def cases():
    rng = np.random.default_rng(20261015)
    out = {}
    pts = off_boundary(off_boundary(blobs(rng, 40000, centers=4, spread=0.3, extent=4.0, noise=0.1), 0.35), 0.35)
    out["blobs600"] = (pts, 0.35, 600)
    out["blobs10"] = (pts, 0.35, 10)
    # a border point within eps of core points of two clusters, itself not core (19 neighbours): min_samples 20, eps 0.32, two
    # 3x3x3 cubes (27 points, spacing 0.1) whose facing faces are 0.5 apart, the point in the middle of that gap
    a, b = cube((0.0, 0.0, 0.0), 0.2, 3), cube((0.7, 0.0, 0.0), 0.2, 3)
    mid = np.array([[0.35, 0.0, 0.0]])
    for order in ("border_first", "border_last", "b_first", "mixed"):
        if order == "border_first":
            p = np.concatenate([mid, a, b])
        elif order == "border_last":
            p = np.concatenate([a, b, mid])
        elif order == "b_first":
            p = np.concatenate([b, mid, a])
        else:
            p = np.concatenate([a, b, mid])[np.random.default_rng(7).permutation(55)]
        out[f"border_{order}"] = (lattice(p), 0.32, 20)
    # thousands of exact duplicates (densification clones Gaussians) next to a sparse cloud
    dup = np.repeat(np.array([[1.0, 2.0, 3.0]]), 3000, axis=0)
    cloud = off_boundary(lattice(rng.uniform(0.0, 4.0, size=(2000, 3))), 0.35) * UNIT
    out["duplicates"] = (lattice(np.concatenate([cloud[:1000], dup, cloud[1000:]])), 0.35, 600)
    out["min_samples_1"] = (off_boundary(lattice(rng.uniform(0, 3, size=(3000, 3))), 0.2), 0.2, 1)
    out["min_samples_gt_n"] = (off_boundary(lattice(rng.uniform(0, 1, size=(500, 3))), 0.35), 0.35, 501)
    # a dense blob and stray points 10^4 units away from it and from each other
    far = np.concatenate([rng.normal(0.0, 0.2, size=(2000, 3)),
                          np.array([[1e4, 0, 0], [-1e4, 0, 0], [0, 1e4, 0], [0, 0, -1e4], [1e4, 1e4, 1e4], [1e4 + 0.1, 1e4, 1e4]])])
    out["far_extent"] = (off_boundary(lattice(far[rng.permutation(len(far))]), 0.35), 0.35, 50)
    out["n1"] = (lattice([[0.5, -0.25, 2.0]]), 0.35, 1)
    return out


def near_pairs(ipts, eps):
    """Pairs whose exact d2 lies within 1e-5 eps^2 of eps^2 (float64 on lattice points is exact)."""
    from scipy.spatial import cKDTree
    x = ipts.astype(np.float64) * UNIT
    pairs = cKDTree(x).query_pairs(eps * 1.00001, output_type="ndarray")
    if not len(pairs):
        return pairs
    d2 = ((x[pairs[:, 0]] - x[pairs[:, 1]]) ** 2).sum(1)
    e2 = float(np.float32(eps)) ** 2
    return pairs[np.abs(d2 - e2) <= 1e-5 * e2]


def off_boundary(ipts, eps):
    """Drops one point of every pair on the eps boundary (random cases only)."""
    bad = near_pairs(ipts, eps)
    return np.delete(ipts, np.unique(bad.max(axis=1)), axis=0) if len(bad) else ipts


def check_margin(pts_f32, eps):
    """No pair's exact d2 within 1e-5 eps^2 of eps^2 (float64 on lattice points is exact)."""
    assert not len(near_pairs(lattice(pts_f32.astype(np.float64)), eps)), "a pair sits on the eps boundary"


def main():
    from sklearn.cluster import DBSCAN
    import sklearn
    data = {"sklearn_version": np.array(sklearn.__version__), "unit": np.float64(UNIT)}
    names = []
    for name, (ipts, eps, ms) in cases().items():
        pts = (ipts.astype(np.float64) * UNIT).astype(np.float32)
        assert np.array_equal(pts.astype(np.float64) / UNIT, ipts)
        check_margin(pts, eps)
        db = DBSCAN(eps=eps, min_samples=ms).fit(pts)
        data[f"{name}_pts"] = ipts
        data[f"{name}_eps"] = np.float64(eps)
        data[f"{name}_min_samples"] = np.int64(ms)
        data[f"{name}_labels"] = db.labels_.astype(np.int32)
        data[f"{name}_core"] = db.core_sample_indices_.astype(np.int32)
        names.append(name)
        print(f"{name:24s} n={len(pts):6d} eps={eps} min_samples={ms} clusters={db.labels_.max() + 1} "
              f"noise={(db.labels_ == -1).sum()} core={len(db.core_sample_indices_)}")
    data["cases"] = np.array(names)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
