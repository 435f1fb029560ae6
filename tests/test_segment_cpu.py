"""The restatement of goi_hyperplane_amd.segment (tests/segment_reference.py) against independent routes, on EVERY case of
tests/segment_cases.py, and the case table against the list it has to cover.  No GPU.

  1. the partition equals scipy.sparse.csgraph.connected_components of the symmetrised join matrix; root is each component's
     minimum id; size equals the bincount; labels are dense, in ascending root order, over the components of size >= min_size;
  2. the gate equals a float64 evaluation wherever the float64 value is not within 1 ulp(fp32) of tau, and is symmetric;
  3. the hand-made cases (ties, mutual pairs, labels, rows, min_size) land where they are stated to;
  4. the table covers every bullet, every P, k and S;
  5. the module checks its arguments before it looks for a device."""
from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import segment_cases as sc
from tests import segment_reference as ref


def _used_join(c, join):
    used = c["join"] if c["join"] is not None else join
    ok = ref.valid_edges(c["idx"])
    return ok if used is None else ok & (np.asarray(used) != 0)


@pytest.mark.parametrize("name", sc.names())
def test_partition_equals_scipy_connected_components(name):
    c = sc.case(name)
    idx = c["idx"]
    P = idx.shape[0]
    join, root, size, label, count = sc.reference(name)
    kept = np.ones(P, bool) if c["rows"] is None else np.asarray(c["rows"]) != 0
    i, m = np.nonzero(_used_join(c, join))
    j = idx[i, m].astype(np.int64)
    both = kept[i] & kept[j]
    A = sp.coo_matrix((np.ones(int(both.sum()), np.int8), (i[both], j[both])), shape=(P, P)).tocsr()
    A = A + A.T  # symmetrised: an edge one endpoint lists unites both
    n, comp = connected_components(A, directed=False) if P else (0, np.zeros(0, np.int32))
    groups = {}
    for row in np.flatnonzero(kept):
        groups.setdefault(int(comp[row]), []).append(int(row))
    want = {frozenset(g) for g in groups.values()}
    assert ref.partition(root) == want
    # root: the minimum id; -1 and size 0 outside `rows`
    assert root.dtype == size.dtype == label.dtype == np.int32
    assert np.all(root[~kept] == -1) and np.all(size[~kept] == 0) and np.all(label[~kept] == -1)
    for g in want:
        members = sorted(g)
        assert np.all(root[members] == members[0]) and np.all(size[members] == len(members))
    assert np.array_equal(size[kept], np.bincount(root[kept], minlength=P)[root[kept]] if P else size[kept])
    # labels: dense ranks in ascending root over the kept components
    big = sorted(min(g) for g in want if len(g) >= c["min_size"])
    assert count == len(big)
    rank = {r: n for n, r in enumerate(big)}
    assert np.array_equal(label, np.array([rank.get(int(r), -1) if r >= 0 else -1 for r in root], np.int32).reshape(P))
    if "expect_parts" in c:
        assert want == {frozenset(g) for g in c["expect_parts"]}
    if "expect_labels" in c:
        assert [int(label[min(g)]) for g in c["expect_parts"]] == c["expect_labels"]


@pytest.mark.parametrize("name", sc.names())
def test_gate_equals_a_float64_evaluation_away_from_tau(name):
    c = sc.case(name)
    if not c["gate"]:
        assert sc.reference(name)[0] is None
        return
    join = sc.reference(name)[0]
    idx, tau = c["idx"], np.float32(c["tau"])
    assert join.dtype == np.uint8 and join.shape == idx.shape and set(np.unique(join)) <= {0, 1}
    args = sc.gate_args(c)
    others = ref.edges(idx, **{**args, "features": None})  # every clause but the feature gate
    assert np.all(join <= others) and np.all(others <= ref.valid_edges(idx))
    if "expect_join" in c:
        assert np.array_equal(join, np.array(c["expect_join"], np.uint8))
    if c["f"] is None:
        assert np.array_equal(join, others)
        return
    d64 = ref.feature_dist2(c["f"], idx, np.float64)
    d32 = ref.feature_dist2(c["f"], idx, np.float32)
    with np.errstate(invalid="ignore"):
        far = np.isnan(d64) | np.isinf(tau) | (np.abs(d64 - np.float64(tau)) > np.spacing(tau))
        want = others & (d64 <= np.float64(tau))
    print(f"{name}: {int(join.sum())} of {int(others.sum())} edges join; {int((~far).sum())} within 1 ulp of tau; "
          f"max |d32 - d64| / d64 = {np.nanmax(np.abs(d32 - d64) / np.maximum(d64, 1e-300), initial=0):.3e}")
    assert np.array_equal(join[far], want[far].astype(np.uint8))
    # symmetric bit for bit: where j lists i back, both entries carry the same d
    P, k = idx.shape
    i, m = np.nonzero(ref.valid_edges(idx))
    j = idx[i, m].astype(np.int64)
    back = idx[j] == i[:, None]
    e, mb = np.nonzero(back)
    assert np.array_equal(d32[i[e], m[e]].view(np.uint32), d32[j[e], mb].view(np.uint32))


def test_ties_land_on_the_stated_side():
    nine = ref.feature_dist2(sc.case("tie_tau_joins")["f"], sc.case("tie_tau_joins")["idx"])
    assert np.all(nine == 9) and sc.case("tie_tau_below")["tau"] < 9 == sc.case("tie_tau_joins")["tau"]
    assert np.float32(sc.case("tie_tau_below")["tau"]) == np.nextafter(np.float32(9), np.float32(0))
    assert sc.reference("tie_tau_joins")[0].all() and not sc.reference("tie_tau_below")[0].any()
    assert sc.reference("tie_dist2_joins")[0].all() and not sc.reference("tie_dist2_below")[0].any()
    # a NaN feature: no edge of that row joins, from either side, although tau = +inf joins every other edge
    c = sc.case("nan_feature_tau_inf_P63_k8_S16")
    join = sc.reference(c["name"])[0]
    touches = (np.arange(63)[:, None] == 7) | (c["idx"] == 7)
    assert not join[touches].any() and join[~touches].all() and touches.sum() > 8
    assert sc.reference(c["name"])[1][7] == 7 and sc.reference(c["name"])[2][7] == 1
    assert sc.reference("knn_P257_k3_S3")[0].all()


def test_the_case_table_covers_the_list():
    cs = sc.cases()
    covered = set().union(*(c["tags"] for c in cs))
    assert covered == set(sc.TAGS), set(sc.TAGS) - covered
    assert {c["idx"].shape[0] for c in cs} >= sc.P_SET
    assert {c["idx"].shape[1] for c in cs} >= sc.K_SET
    assert {c["f"].shape[1] for c in cs if c["f"] is not None} >= sc.S_SET
    by_tag = {t: [c for c in cs if t in c["tags"]] for t in sc.TAGS}
    idx_of = lambda t: by_tag[t][0]["idx"]  # noqa: E731
    assert any((c["idx"] == -1).all(axis=1).any() for c in by_tag["empty_rows"])
    assert any(((c["idx"] == -1).any(axis=1) & (c["idx"][:, 0] >= 0)).any() for c in by_tag["tails"])
    P = idx_of("out_of_range").shape[0]
    assert (idx_of("out_of_range") >= P).any() and (idx_of("out_of_range") < -1).any()
    assert (idx_of("self_edges")[:, 0] == np.arange(idx_of("self_edges").shape[0])).all()
    assert (idx_of("duplicates")[:, 0] == idx_of("duplicates")[:, 1]).all()
    assert idx_of("star").shape == (5000, 1) and (idx_of("star")[1:] == 0).all() and by_tag["no_join"][0]["gate"] is False
    for t in ("path_ascending", "path_descending", "path_shuffled"):
        assert idx_of(t).shape == (4999, 1) and sc.reference(by_tag[t][0]["name"])[2].max() == 4999
    assert (np.diff(np.flatnonzero(idx_of("path_ascending")[:, 0] >= 0)) == 1).all() and idx_of("path_ascending")[0, 0] == 1
    assert idx_of("path_descending")[4998, 0] == 4997
    bridge = idx_of("directed_bridge")
    assert bridge[5, 3] == 60 and not (bridge[40:] < 40)[bridge[40:] >= 0].any()  # nobody in the second blob lists the first
    assert {c["mutual"] for c in by_tag["mutual_on"]} == {True} and {c["mutual"] for c in by_tag["mutual_off"]} == {False}
    assert {"pairs_mutual_on", "pairs_mutual_off"} <= set(sc.names())
    art = by_tag["rows_articulation"][0]
    assert not art["rows"][2] and art["join"].all()
    assert sc.reference("line_whole")[4] == 1 and sc.reference(art["name"])[4] == 2  # removing the row splits the component
    assert any(c["rows"] is not None for c in by_tag["knn_cloud"]) and any(c["labels"] is not None for c in by_tag["knn_cloud"])
    assert any(c["max_dist2"] is not None for c in by_tag["knn_cloud"])
    sizes = sorted(len(g) for g in sc.SIZES_PARTS)
    assert by_tag["min_size_equal"][0]["min_size"] in sizes and by_tag["min_size_above"][0]["min_size"] - 1 in sizes
    assert by_tag["min_size_above_all"][0]["min_size"] > max(sizes) and sc.reference("sizes_min6")[4] == 0
    assert (sc.reference("sizes_min6")[3] == -1).all()
    # the gate decides something on the clouds: neither every edge nor none
    for name in ("knn_P5000_k8_S16", "knn_P257_k8_S4", "knn_P64_k16_S17"):
        join = sc.reference(name)[0]
        assert 0.05 < join.mean() < 0.95, (name, join.mean())
    assert 1 < sc.reference("knn_P5000_k8_S16")[4] < 5000


def test_the_module_is_exported_and_checks_its_arguments_before_any_device():
    import torch

    import goi_hyperplane_amd
    from goi_hyperplane_amd import segment
    assert goi_hyperplane_amd.segment is segment and "segment" in goi_hyperplane_amd.__all__
    idx = torch.zeros((4, 2), dtype=torch.int32)
    f = torch.zeros((4, 3))
    for call in (lambda: segment.edges(idx, f, 1.0), lambda: segment.components(idx),
                 lambda: segment.select(segment.Segments(*[torch.zeros(4, dtype=torch.int32)] * 5), torch.zeros(1, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for call, exc, text in (
            (lambda: segment.edges(idx.long()), TypeError, "idx must be int32"),
            (lambda: segment.edges(idx[0]), ValueError, r"idx must have shape \(P, k\)"),
            (lambda: segment.edges(idx, torch.zeros((4, 33))), ValueError, "1 <= S <= 32"),
            (lambda: segment.edges(idx, torch.zeros((5, 3))), ValueError, "features must have shape"),
            (lambda: segment.edges(idx, f, float("nan")), ValueError, "tau is NaN"),
            (lambda: segment.edges(idx, f, 1.0, max_dist2=1.0), ValueError, "max_dist2 needs dist2"),
            (lambda: segment.edges(idx, f, 1.0, dist2=torch.zeros((4, 3))), ValueError, "dist2 must have idx's shape"),
            (lambda: segment.edges(idx, f, 1.0, labels=torch.zeros(4, dtype=torch.int32)), TypeError, "labels must be int64"),
            (lambda: segment.edges(idx, f, 1.0, rows=torch.zeros(5, dtype=torch.bool)), ValueError, "rows must have shape"),
            (lambda: segment.components(idx, join=torch.zeros((4, 3), dtype=torch.uint8)), ValueError, "join must have idx's shape"),
            (lambda: segment.components(idx, min_size=0), ValueError, "min_size"),
            (lambda: segment.components(idx, min_size=1.5), TypeError, "min_size must be an int"),
            (lambda: segment.select(None, idx), TypeError, "segments must be"),
    ):
        with pytest.raises(exc, match=text):
            call()
