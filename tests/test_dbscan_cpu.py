"""Exact DBSCAN without a GPU: the numpy restatement (tests/dbscan_reference.py, the fp32 neighbour form of
csrc/dbscan.hip) reproduces sklearn's labels pinned in tests/golden/ref_dbscan_pins.npz and, where sklearn is installed,
live sklearn on fresh lattice data; the public entry points validate their arguments and refuse CPU input (no fallback)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.dbscan_reference import dbscan_reference, lattice_blobs

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "ref_dbscan_pins.npz"))


def pin_case(pins, name):
    pts = (pins[f"{name}_pts"].astype(np.float64) * float(pins["unit"])).astype(np.float32)
    core = np.zeros(len(pts), bool)
    core[pins[f"{name}_core"]] = True
    return pts, float(pins[f"{name}_eps"]), int(pins[f"{name}_min_samples"]), pins[f"{name}_labels"].astype(np.int64), core


def test_pins_cover_the_rules(pins):
    names = set(str(n) for n in pins["cases"])
    assert {"blobs600", "blobs10", "duplicates", "min_samples_1", "min_samples_gt_n", "far_extent", "n1"} <= names
    assert sum(n.startswith("border_") for n in names) >= 3
    # the border point carries the smaller of the two labels in every index order
    for n in names:
        if n.startswith("border_"):
            pts, _, _, labels, core = pin_case(pins, n)
            mid = int(np.nonzero(~core)[0][0])
            assert labels[mid] == 0 and set(labels.tolist()) == {0, 1}


@pytest.mark.parametrize("name", ["blobs600", "blobs10", "border_border_first", "border_border_last", "border_b_first",
                                  "border_mixed", "duplicates", "min_samples_1", "min_samples_gt_n", "far_extent", "n1"])
def test_restatement_equals_sklearn_pins(pins, name):
    pts, eps, ms, labels, core = pin_case(pins, name)
    got, got_core = dbscan_reference(pts, eps, ms)
    np.testing.assert_array_equal(got_core, core)
    np.testing.assert_array_equal(got, labels)


@pytest.mark.parametrize("seed,ms", [(1, 600), (2, 10), (3, 1)])
def test_restatement_equals_live_sklearn(seed, ms):
    sk = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(seed)
    pts = lattice_blobs(rng, 12000, spread=0.3, extent=3.0)
    db = sk.DBSCAN(eps=0.35, min_samples=ms).fit(pts)
    got, got_core = dbscan_reference(pts, 0.35, ms)
    core = np.zeros(len(pts), bool)
    core[db.core_sample_indices_] = True
    np.testing.assert_array_equal(got_core, core)
    np.testing.assert_array_equal(got, db.labels_)


def test_dbscan_validates_like_sklearn():
    from goi_hyperplane_amd.cluster import DBSCAN, dbscan
    x = np.zeros((4, 3), np.float32)
    for eps in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="'eps' parameter of DBSCAN must be a float in the range"):
            DBSCAN(eps=eps).fit(x)
        with pytest.raises(ValueError, match="'eps' parameter"):
            dbscan(torch.zeros(4, 3), eps, 5)
    for ms in (0, -3, 2.5):
        with pytest.raises(ValueError, match="'min_samples' parameter of DBSCAN must be an int in the range"):
            DBSCAN(min_samples=ms).fit(x)
    with pytest.raises(TypeError, match="float32"):
        DBSCAN().fit(x.astype(np.float64))
    with pytest.raises(TypeError, match="float32"):
        dbscan(torch.zeros(4, 3, dtype=torch.float64), 0.5, 5)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        dbscan(torch.zeros(4, 2), 0.5, 5)
    with pytest.raises(TypeError):
        DBSCAN().fit([[0.0, 0.0, 0.0]])


def test_dbscan_refuses_cpu_tensors():
    """A CPU tensor is an error, not a quiet fall-back to a host implementation."""
    from goi_hyperplane_amd.cluster import DBSCAN, dbscan
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dbscan(torch.zeros(10, 3), 0.5, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DBSCAN().fit(torch.zeros(10, 3))


def test_group_points_is_exported():
    from goi_hyperplane_amd import semantic
    import inspect
    sig = inspect.signature(semantic.group_points)
    assert list(sig.parameters)[:8] == ["pc", "selected", "viewpoint_camera", "bg_color", "mlp", "lut", "score_fn", "res_mask"]
    assert sig.parameters["eps"].default == 0.35 and sig.parameters["min_samples"].default == 600
    assert sig.parameters["keep_ratio"].default == 0.7
