"""The k-NN graph on the GPU (csrc/knn.hip: goi_knn_graph, goi_knn_majority through goi_hyperplane_amd.knn) against its numpy
restatement (tests/knn_graph_reference.py).  Bar: array_equal on the ids and on the bits of the distances, everywhere."""
import functools

import numpy as np
import pytest
import torch

from tests import knn_graph_reference as ref
from tests.test_knn_cpu import clouds

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4, 5, 8, 9, 16]  # every KCAP boundary (4, 8, 16) from both sides


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def gpu_graph(pts, k, selection=None):
    from goi_hyperplane_amd import knn
    return host(knn.graph(dev(pts), k, None if selection is None else dev(selection)))


def gpu_query(q, r, k, qm=None, rm=None):
    from goi_hyperplane_amd import knn
    return host(knn.query(dev(q), dev(r), k, None if qm is None else dev(qm), None if rm is None else dev(rm)))


@functools.lru_cache(maxsize=None)
def cloud_rows(name):
    pts = clouds()[name][:3000]
    return pts, ref.knn_rows(pts, pts, 16, exclude_self=True)  # the rows for k < 16 are its prefixes


@functools.lru_cache(maxsize=None)
def ragged_rows(P):
    pts = np.random.default_rng(P).standard_normal((P, 3)).astype(np.float32)
    return pts, ref.knn_rows(pts, pts, 16, exclude_self=True)


@pytest.mark.parametrize("name", list(clouds()))
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_clouds_match_the_reference_bit_for_bit(name, k):
    pts, (i, d) = cloud_rows(name)
    assert same(gpu_graph(pts, k), (i[:, :k], d[:, :k])), name


@pytest.mark.parametrize("P", [0, 1, 2, 3, 4, 5, 16, 17, 63, 64, 65, 255, 256, 257, 513, 1025])
@pytest.mark.parametrize("k", KS)
def test_ragged_sizes_and_padding(P, k):
    pts, (i, d) = ragged_rows(P)
    got = gpu_graph(pts, k)
    assert got[0].shape == (P, k) and got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert same(got, (i[:, :k], d[:, :k]))
    if P <= k:
        assert np.all(got[0][:, max(P - 1, 0):] == -1) and np.all(np.isposinf(got[1][:, max(P - 1, 0):]))


@pytest.mark.parametrize("P", [4, 5, 257, 1025, 20000])
def test_k3_reproduces_distCUDA2(P):
    from simple_knn._C import distCUDA2
    pts = np.random.default_rng(P + 1).standard_normal((P, 3)).astype(np.float32)
    _, d = gpu_graph(pts, 3)
    assert np.array_equal(((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3), distCUDA2(dev(pts)).cpu().numpy())


def test_more_candidate_boxes_than_one_trip_tests():
    """66 000 points = 258 boxes: the second trip of the box loop.  Distances against distCUDA2, ids by recomputing theirs."""
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(11)
    pts = rng.standard_normal((66_000, 3)).astype(np.float32)
    i, d = gpu_graph(pts, 3)
    assert np.array_equal(((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3), distCUDA2(dev(pts)).cpu().numpy())
    assert np.all(i >= 0) and not np.any(i == np.arange(len(pts))[:, None])
    for j in range(3):
        again = np.array([ref.dist2_matrix(pts[a:a + 1], pts[b:b + 1])[0, 0] for a, b in zip(range(0, 66_000, 97), i[::97, j])])
        assert np.array_equal(again, d[::97, j])
    q = (rng.standard_normal((300, 3)) * 2).astype(np.float32)
    assert same(gpu_query(q, pts, 5), ref.knn_rows(q, pts, 5))


@pytest.mark.parametrize("k", [1, 4, 16])
def test_identical_points_take_the_lowest_other_ids(k):
    pts = np.full((600, 3), 0.375, np.float32)
    i, d = gpu_graph(pts, k)
    want = np.array([[j for j in range(k + 1) if j != a][:k] for a in range(600)], np.int32)
    assert np.array_equal(i, want) and np.all(d == 0)


def test_input_order_invariance():
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((5000, 3)).astype(np.float32)
    _, d9 = ref.knn_rows(pts, pts, 9, exclude_self=True)
    assert np.all(d9[:, 1:] > d9[:, :-1]), "the cloud of this test must be tie-free"
    perm = rng.permutation(len(pts))
    ia, da = gpu_graph(pts, 8)
    ib, db = gpu_graph(pts[perm], 8)
    assert np.array_equal(db, da[perm])
    assert np.array_equal(perm[ib], ia[perm])


@pytest.mark.parametrize("Pq,Pr,k", [(1, 1, 1), (5, 3, 2), (300, 77, 8), (77, 300, 16), (1025, 513, 3), (64, 2, 4), (257, 1, 5),
                                      (3, 1025, 9), (7, 0, 3)])
def test_bipartite_ragged(Pq, Pr, k):
    rng = np.random.default_rng(Pq * 31 + Pr)
    q = rng.standard_normal((Pq, 3)).astype(np.float32)
    r = (rng.standard_normal((Pr, 3)) * 1.5 + 0.25).astype(np.float32)
    got = gpu_query(q, r, k)
    assert same(got, ref.knn_rows(q, r, k))
    if Pr < k:
        assert np.all(got[0][:, Pr:] == -1) and np.all(np.isposinf(got[1][:, Pr:]))


def test_bipartite_queries_outside_the_references_and_on_them():
    rng = np.random.default_rng(8)
    r = rng.random((1500, 3)).astype(np.float32)
    far = (rng.standard_normal((200, 3)) * 50 + [1000, -400, 30]).astype(np.float32)
    on = r[rng.choice(1500, 300, replace=False)]  # coincident with a reference: it counts, with distance 0
    q = np.concatenate([far, on, (rng.random((100, 3)) * 3 - 1).astype(np.float32)])[rng.permutation(600)]
    for k in (1, 6, 16):
        got = gpu_query(q, r, k)
        assert same(got, ref.knn_rows(q, r, k))
    hit = np.all(q[:, None, :] == r[None, :, :], axis=2).any(1)
    assert hit.sum() == 300 and np.all(got[1][hit, 0] == 0) and np.all(got[1][~hit, 0] > 0)
    same_tensor = gpu_query(r, r, 4)  # queries ARE the references and nothing is excluded: every row starts with itself
    assert same(same_tensor, ref.knn_rows(r, r, 4)) and np.array_equal(same_tensor[0][:, 0], np.arange(1500))


def masks_of(P, rng):
    one = np.zeros(P, bool)
    one[P // 3] = True
    return {"none": np.zeros(P, bool), "one": one, "tenth": rng.random(P) < 0.1, "all": np.ones(P, bool)}


@pytest.mark.parametrize("qkind", ["none", "one", "tenth", "all"])
@pytest.mark.parametrize("rkind", ["none", "one", "tenth", "all"])
def test_masks_equal_the_index_selected_arrays(qkind, rkind):
    rng = np.random.default_rng(21)
    q = rng.standard_normal((1300, 3)).astype(np.float32)
    r = rng.standard_normal((2100, 3)).astype(np.float32)
    r[:50] += 40  # outliers that are masked out in most cases must not matter
    qm, rm = masks_of(1300, rng)[qkind], masks_of(2100, rng)[rkind]
    k = 5
    i, d = gpu_query(q, r, k, qm, rm)
    si, sd = ref.knn_rows(q[qm], r[rm], k)
    ids = np.flatnonzero(rm)
    want_i = np.full((1300, k), -1, np.int32)
    want_d = np.full((1300, k), np.inf, np.float32)
    want_i[qm] = np.where(si >= 0, ids[np.maximum(si, 0)] if len(ids) else -1, -1)
    want_d[qm] = sd
    assert same((i, d), (want_i, want_d))
    assert np.all(i[~qm] == -1) and np.all(np.isposinf(d[~qm]))


@pytest.mark.parametrize("kind", ["none", "one", "tenth", "all"])
def test_selection_of_graph(kind):
    rng = np.random.default_rng(22)
    pts = rng.standard_normal((2500, 3)).astype(np.float32)
    sel = masks_of(2500, rng)[kind]
    k = 8
    i, d = gpu_graph(pts, k, sel)
    si, sd = ref.knn_rows(pts[sel], pts[sel], k, exclude_self=True)
    ids = np.flatnonzero(sel)
    want_i = np.full((2500, k), -1, np.int32)
    want_d = np.full((2500, k), np.inf, np.float32)
    want_i[sel] = np.where(si >= 0, ids[np.maximum(si, 0)] if len(ids) else -1, -1)
    want_d[sel] = sd
    assert same((i, d), (want_i, want_d))
    assert same((i, d), ref.knn_rows(pts, pts, k, query_keep=sel, ref_keep=sel, exclude_self=True))


@pytest.mark.parametrize("qkind,rkind", [("tenth", None), (None, "tenth"), ("tenth", "all"), ("one", None), ("tenth", "tenth2")])
def test_exclude_self_with_different_masks(qkind, rkind):
    """goi_knn_graph(P, x, qm, P, x, rm, k, exclude_self = 1) with two DIFFERENT masks: the queries get their own Morton sort, and
    the reference left out of row i is still reference i (by id), no other."""
    from goi_hyperplane_amd import knn
    rng = np.random.default_rng(23)
    pts = rng.standard_normal((2300, 3)).astype(np.float32)
    pts[100:140] = pts[60:100]  # coincident pairs: the twin stays, at distance 0, only the query itself goes
    kinds = dict(masks_of(2300, rng), tenth2=rng.random(2300) < 0.1)
    qm, rm = kinds.get(qkind), kinds.get(rkind)
    x = dev(pts)
    got = host(knn._graph(x, None if qm is None else dev(qm).view(torch.uint8), x, None if rm is None else dev(rm).view(torch.uint8),
                          6, True))
    assert same(got, ref.knn_rows(pts, pts, 6, query_keep=qm, ref_keep=rm, exclude_self=True))
    assert not np.any(got[0] == np.arange(2300)[:, None])


@functools.lru_cache(maxsize=None)
def two_blobs():
    rng = np.random.default_rng(30)
    a = rng.standard_normal((900, 3)) * 0.5
    b = rng.standard_normal((700, 3)) * 0.5 + [4, 0, 0]
    far = rng.standard_normal((40, 3)) * 0.2 + [0, 60, 0]  # unlabelled, far from every label
    pts = np.concatenate([a, b, far]).astype(np.float32)
    truth = np.concatenate([np.full(900, 3), np.full(700, 7), np.full(40, -1)]).astype(np.int64)
    labels = np.where(rng.random(len(pts)) < 0.25, truth, -1)
    order = rng.permutation(len(pts))
    return pts[order], labels[order]


def test_majority_and_complete_labels_against_the_reference():
    from goi_hyperplane_amd import knn
    pts, labels = two_blobs()
    idx, dist2 = knn.query(dev(pts), dev(pts), 8, dev(labels < 0), dev(labels >= 0))
    for cut in (None, 0.05, np.inf):
        lab, cnt = knn.majority_labels(idx, dev(labels), dist2, cut)
        rl, rc = ref.majority_labels(idx.cpu().numpy(), labels, dist2.cpu().numpy(), cut)
        assert np.array_equal(lab.cpu().numpy(), rl) and np.array_equal(cnt.cpu().numpy(), rc)
        assert lab.dtype == torch.int64 and cnt.dtype == torch.int32
    lab, _ = knn.majority_labels(idx, dev(labels))
    assert np.array_equal(lab.cpu().numpy(), ref.majority_labels(idx.cpu().numpy(), labels)[0])
    for k, cut, sel in ((8, None, None), (3, 4.0, None), (16, None, np.random.default_rng(1).random(len(pts)) < 0.5), (8, 0.01, None)):
        got = knn.complete_labels(dev(pts), dev(labels), k=k, max_dist2=cut, selection=None if sel is None else dev(sel))
        got = got.cpu().numpy()
        assert np.array_equal(got, ref.complete_labels(pts, labels, k, cut, sel))
        assert np.array_equal(got[labels >= 0], labels[labels >= 0]), "labelled rows are unchanged"
    far = pts[:, 1] > 30
    done = knn.complete_labels(dev(pts), dev(labels), k=8, max_dist2=4.0).cpu().numpy()
    assert np.all(done[far] == -1) and np.all(done[~far] >= 0), "the cut leaves the far queries unlabelled"
    assert np.all(knn.complete_labels(dev(pts), dev(labels), k=8).cpu().numpy() >= 0)
    full = np.abs(labels)
    assert np.array_equal(knn.complete_labels(dev(pts), dev(full)).cpu().numpy(), full)
    none = np.full(len(pts), -1, np.int64)
    assert np.array_equal(knn.complete_labels(dev(pts), dev(none)).cpu().numpy(), none)
    off = np.zeros(len(pts), bool)
    assert np.array_equal(knn.complete_labels(dev(pts), dev(labels), selection=dev(off)).cpu().numpy(), labels)


def test_majority_tie_goes_to_the_lowest_class():
    from goi_hyperplane_amd import knn
    labels = np.array([5, 2, 2, 5, -1, 9, 1 << 40], np.int64)  # values, not bins: any int64 >= 0
    idx = np.array([[0, 1, 2, 3], [0, 3, 1, 4], [4, 4, -1, -1], [5, -1, -1, -1], [1, 0, 3, 5], [6, 6, 0, 0]], np.int32)
    dist2 = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [1, 1, np.inf, np.inf], [7, np.inf, np.inf, np.inf], [1, 2, 2.5, 3], [0, 0, 0, 0]],
                     np.float32)
    lab, cnt = knn.majority_labels(dev(idx), dev(labels))
    assert lab.tolist() == [2, 5, -1, 9, 5, 5] and cnt.tolist() == [2, 2, 0, 1, 2, 2]
    lab, cnt = knn.majority_labels(dev(idx), dev(labels), dev(dist2), 2.0)
    assert lab.tolist() == [2, 5, -1, -1, 2, 5] and cnt.tolist() == [1, 2, 0, 0, 1, 2]


def test_statistical_outliers_are_exactly_the_planted_points():
    from goi_hyperplane_amd import knn
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    extent = 9.0
    planted = np.array([[100, 0, 0], [0, -100, 0], [0, 0, 100], [-100, -100, 0], [100, 100, 100]], np.float32) * extent
    rng = np.random.default_rng(2)
    pts = np.concatenate([g, planted])[rng.permutation(1005)]
    is_planted = np.abs(pts).max(1) > 50
    got = knn.statistical_outliers(dev(pts), k=16, ratio=2.0).cpu().numpy()
    assert got.dtype == bool and np.array_equal(got, is_planted) and got.sum() == 5
    assert np.array_equal(got, ref.statistical_outliers(pts, 16, 2.0))
    sel = ~is_planted | (pts[:, 0] > 50)  # two of the five stay in
    got = knn.statistical_outliers(dev(pts), k=16, ratio=2.0, selection=dev(sel)).cpu().numpy()
    assert np.array_equal(got, is_planted & sel) and got.sum() == 2
    md = knn.mean_distance(dev(np.array([[1, 4, np.inf], [np.inf, np.inf, np.inf], [9, 9, 9]], np.float32))).cpu().numpy()
    assert np.array_equal(md, np.array([1.5, np.inf, 3], np.float32))


def test_two_runs_give_identical_bits():
    from goi_hyperplane_amd import knn
    pts, labels = two_blobs()
    p, lab = dev(pts), dev(labels)
    sel = dev(np.random.default_rng(4).random(len(pts)) < 0.7)
    calls = {
        "graph": lambda: knn.graph(p, 16, sel),
        "query": lambda: knn.query(p[:500].contiguous(), p, 7, None, sel),
        "majority_labels": lambda: knn.majority_labels(*knn.query(p, p, 8, None, lab >= 0)[:1], lab),
        "complete_labels": lambda: (knn.complete_labels(p, lab, k=8, max_dist2=2.0),),
        "mean_distance": lambda: (knn.mean_distance(knn.graph(p, 5)[1]),),
        "statistical_outliers": lambda: (knn.statistical_outliers(p, 8, 1.0),),
    }
    for name, call in calls.items():
        a, b = call(), call()
        assert all(torch.equal(x, y) and (not x.is_floating_point() or torch.equal(x.view(torch.int32), y.view(torch.int32)))
                   for x, y in zip(a, b)), name


def test_refusals():
    from goi_hyperplane_amd import knn
    p = torch.zeros(8, 3, device="cuda")
    lab = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.graph(torch.zeros(8, 3), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.query(p, torch.zeros(8, 3), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.complete_labels(p, torch.zeros(8, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        knn.graph(p, 3, torch.ones(8, dtype=torch.bool))
    with pytest.raises(TypeError):
        knn.graph(p.double(), 3)
    with pytest.raises(TypeError):
        knn.query(p, p.half(), 3)
    with pytest.raises(TypeError):
        knn.complete_labels(p, lab.int())
    with pytest.raises(TypeError):
        knn.majority_labels(torch.zeros(8, 3, dtype=torch.int64, device="cuda"), lab)
    with pytest.raises(TypeError):
        knn.graph(p, 3, torch.ones(8, device="cuda"))
    with pytest.raises(TypeError):
        knn.mean_distance(p.double())
    for k in (0, 17):
        with pytest.raises(ValueError, match="1 <= k <= 16"):
            knn.graph(p, k)
        with pytest.raises(ValueError, match="1 <= k <= 16"):
            knn.query(p, p, k)
        with pytest.raises(ValueError, match="1 <= k <= 16"):
            knn.complete_labels(p, lab, k=k)
