"""goi_hyperplane_amd.instance on the GPU against its numpy restatement (tests/instance_reference.py) on the cases of
tests/instance_cases.py:
  1. members, n and hits integer-equal, every float output bit-equal; inputs untouched; a second call gives the same bits;
  2. an instance's bits depend on its own member sequence alone: relabelling, appended rows, a larger K, other instances;
  3. members= reuse and an int capacity do not synchronise the host; capacity=None gives the same result;
  4. vote / rows_of / select against the restatement: ties, -1 rows, dropped components, each of the eight bits;
  5. end to end: a noisy per-Gaussian hit on two touching balls becomes exactly one ball.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from goi_hyperplane_amd import instance, segment
from tests import instance_cases as ic
from tests import instance_reference as ref

pytestmark = pytest.mark.gpu
FLOATS = ("wsum", "centroid", "lo", "hi", "cov", "feature")
KEYS = ("n", "hits") + FLOATS
INPUTS = ("label", "xyz", "features", "weight", "hit")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def up(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(torch.device("cuda:0"))  # (a copy: the cases are read-only)


def down(st):
    return {key: None if getattr(st, key) is None else getattr(st, key).cpu().numpy() for key in KEYS}


def same_bits(a, b):
    """bit-equal; a NaN equals a NaN (its payload is not part of the contract)"""
    if a is None or b is None:
        return a is None and b is None
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))))


def run(c, K=None):
    """the case through the module: (the device inputs, Members, InstanceStats)"""
    t = {key: up(c[key]) for key in INPUTS}
    m = instance.members(t["label"], c["K"] if K is None else K)
    return t, m, instance.stats(t["label"], t["xyz"], t["features"], t["weight"], t["hit"], members=m)


@functools.lru_cache(maxsize=None)
def on_device(name):
    return run(ic.case(name))


def by_hand(label, K, xyz, f=None, w=None, hit=None):
    """arrays through the module and through the restatement: (got, want) dicts"""
    st = instance.stats(up(label), up(xyz), up(f), up(w), up(hit), capacity=K)
    ptr, rows = ref.members(label, K)
    return down(st), ref.stats(ptr, rows, xyz, f, w, hit)


# ---- 1. against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.names())
def test_every_output_equals_the_restatement(dev, name):
    c = ic.case(name)
    t, m, st = on_device(name)
    want_ptr, want_rows, want = ic.reference(name)
    K, P = c["K"], c["label"].shape[0]
    assert m.K == K and m.ptr.dtype == m.rows.dtype == torch.int32 and tuple(m.ptr.shape) == (K + 1,) and tuple(m.rows.shape) == (P,)
    assert np.array_equal(m.ptr.cpu().numpy(), want_ptr) and np.array_equal(m.rows.cpu().numpy(), want_rows)
    got = down(st)
    assert st.members is m and (st.feature is None) == (c["features"] is None)
    for key in KEYS:
        assert same_bits(got[key], want[key]), key
    assert st.n.dtype == st.hits.dtype == torch.int32 and tuple(st.hits.shape) == (K, 8) and tuple(st.cov.shape) == (K, 6)
    for key in INPUTS:  # the inputs are untouched
        assert c[key] is None or np.array_equal(t[key].cpu().numpy(), c[key], equal_nan=c[key].dtype.kind == "f"), key
    again = run(c)  # a second call, other buffers: the same bits
    assert torch.equal(again[1].ptr, m.ptr) and torch.equal(again[1].rows, m.rows)
    second = down(again[2])
    for key in KEYS:
        assert same_bits(second[key], got[key]), key


def test_twins_give_identical_bits(dev):
    a, b = down(on_device("twins")[2]), down(on_device("twins_K3")[2])
    for key in KEYS:
        assert a[key][2].tobytes() == a[key][7].tobytes() == b[key][1].tobytes(), key


# ---- 2. an instance's bits are its own ---------------------------------------------------------------------------------------------
def test_relabelling_the_instances_permutes_the_rows_bit_for_bit(dev):
    c = ic.case("all_sizes_S16")
    K = c["K"]
    perm = np.random.default_rng(3).permutation(K)
    inside = (c["label"] >= 0) & (c["label"] < K)
    relabelled = dict(c, label=np.where(inside, perm[np.clip(c["label"], 0, K - 1)], c["label"]).astype(np.int32))
    base, moved = down(on_device("all_sizes_S16")[2]), down(run(relabelled)[2])
    for key in KEYS:
        assert same_bits(moved[key][perm], base[key]), key


def test_appended_rows_and_a_larger_K_leave_every_instance_alone(dev):
    c = ic.case("mid_sizes_S17")
    K, P = c["K"], c["label"].shape[0]
    base = down(on_device("mid_sizes_S17")[2])
    wider = down(run(c, K=K + 40)[2])  # raising K alone: trailing empty instances
    rng = np.random.default_rng(4)
    extra = 1500  # rows of three other instances (one of them large), and rows in none
    more = dict(c, K=K + 3, label=np.r_[c["label"], rng.choice([K, K + 1, K + 2, -1], extra, p=[0.6, 0.2, 0.1, 0.1])].astype(np.int32),
                xyz=np.r_[c["xyz"], rng.standard_normal((extra, 3)).astype(np.float32)],
                features=np.r_[c["features"], rng.standard_normal((extra, 17)).astype(np.float32)],
                weight=np.r_[c["weight"], rng.random(extra).astype(np.float32)],
                hit=np.r_[c["hit"], rng.integers(0, 256, extra).astype(np.uint8)])
    grown = down(run(more)[2])
    assert grown["n"][K] > 512
    for key in KEYS:
        assert same_bits(wider[key][:K], base[key]) and same_bits(grown[key][:K], base[key]), key
    assert not wider["n"][K:].any() and np.all(wider["lo"][K:] == np.inf) and np.all(wider["hi"][K:] == -np.inf)


def test_a_large_instance_alone_and_among_3000_singletons(dev):
    rng = np.random.default_rng(6)
    n, singles = 5000, 3000
    xyz, f, w, h = ic.fields(n, 7, S=32, weight="positive", hit="patterns", centre=2.0)
    alone, _ = by_hand(np.zeros(n, np.int32), 1, xyz, f, w, h)
    P = n + singles
    at = np.sort(rng.choice(P, n, replace=False))  # the large instance's rows, in the same order, spread over the array
    label = np.zeros(P, np.int32)
    rest = np.setdiff1d(np.arange(P), at)
    label[rest] = 1 + rng.permutation(singles)
    x2, f2, w2, h2 = ic.fields(P, 8, S=32, weight="positive", hit="patterns")
    x2[at], f2[at], w2[at], h2[at] = xyz, f, w, h
    crowd, want = by_hand(label, singles + 1, x2, f2, w2, h2)
    for key in KEYS:
        assert same_bits(crowd[key][:1], alone[key]), key
        assert same_bits(crowd[key], want[key]), key


# ---- 3. no host synchronisation -----------------------------------------------------------------------------------------------------
def test_members_reuse_and_an_int_capacity_do_not_synchronise(dev):
    c = ic.case("all_sizes_S16")
    t = {key: up(c[key]) for key in INPUTS}
    seg = segment.Segments(t["label"], t["label"], t["label"], torch.tensor([c["K"]], dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev))
    hit = t["hit"] > 127
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # nothing here synchronises the host
    try:
        m = instance.members(seg, capacity=c["K"])
        a = instance.stats(seg, t["xyz"], t["features"], t["weight"], t["hit"], members=m)
        b = instance.stats(t["label"], t["xyz"], t["features"], t["weight"], t["hit"], capacity=c["K"])
        keep = instance.vote(a, 0.5, 1, bit=7)
        rows = instance.rows_of(seg, keep)
        picked = instance.select(seg, hit, 0.5, capacity=c["K"])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    free = instance.stats(seg, t["xyz"], t["features"], t["weight"], t["hit"])  # capacity=None: reads seg.count back
    assert free.members.K == c["K"]
    da, want = down(a), ic.reference("all_sizes_S16")[2]
    for other in (b, free):
        do = down(other)
        for key in KEYS:
            assert same_bits(do[key], da[key]) and same_bits(da[key], want[key]), key
    assert torch.equal(picked, rows) and rows.dtype == torch.bool and tuple(rows.shape) == tuple(t["label"].shape)
    assert np.array_equal(rows.cpu().numpy(), ref.select(c["label"], c["K"], c["hit"] > 127, 0.5))


def test_capacity_none_of_a_bare_label_array(dev):
    c = ic.case("mid_sizes_plain")
    st = instance.stats(up(c["label"]), up(c["xyz"]), hit=up(c["hit"]))
    assert st.members.K == int(c["label"].max()) + 1 == c["K"]
    got, want = down(st), ic.reference("mid_sizes_plain")[2]
    for key in KEYS:
        assert same_bits(got[key], want[key]), key
    empty = instance.stats(torch.full((5,), -1, dtype=torch.int32, device=dev), torch.zeros(5, 3, device=dev))
    assert empty.members.K == 0 and empty.n.numel() == 0 and empty.members.rows.cpu().tolist() == [-1] * 5


# ---- 4. vote, rows_of, select -------------------------------------------------------------------------------------------------------
def test_vote_for_each_bit_and_fraction(dev):
    c = ic.case("all_sizes_S16")
    _, _, st = on_device("all_sizes_S16")
    _, _, want = ic.reference("all_sizes_S16")
    for bit in range(8):
        for fraction, min_hits in ((0.5, 1), (0.25, 1), (0.51, 3), (0.0, 0), (1, 1)):
            got = instance.vote(st, fraction, min_hits, bit=bit)
            assert got.dtype == torch.bool and tuple(got.shape) == (c["K"],)
            assert np.array_equal(got.cpu().numpy(), ref.vote(want["n"], want["hits"], fraction, min_hits, bit)), (bit, fraction)
    with pytest.raises(ValueError, match="bit"):
        instance.vote(st, bit=8)
    with pytest.raises(ValueError, match="min_hits"):
        instance.vote(st, min_hits=-1)


def test_select_at_exact_ties_with_outside_rows(dev):
    sizes, counts = (10, 10, 10, 4, 0, 7, 300), (5, 4, 6, 2, 0, 7, 150)  # 5 / 10, 2 / 4 and 150 / 300 tie at 0.5; 7 / 10 at 0.7
    label = ic.partition(sizes, 12, outside=(-1,) * 15 + (len(sizes), ic.INT_MIN))
    hit = np.zeros(label.shape[0], bool)
    for k, n_hit in enumerate(counts):
        hit[np.flatnonzero(label == k)[:n_hit]] = True
    hit[label < 0] = True  # hits on rows in no instance count for nothing
    K = len(sizes)
    d_label, d_hit = up(label), up(hit)
    for fraction, min_hits, kept in ((0.5, 1, [0, 2, 3, 5, 6]), (0.7, 1, [5]), (0.4, 1, [0, 1, 2, 3, 5, 6]), (0.5, 6, [2, 5, 6]),
                                     (0.5001, 1, [2, 5])):
        got = instance.select(d_label, d_hit, fraction, min_hits, capacity=K).cpu().numpy()
        assert np.array_equal(got, ref.select(label, K, hit, fraction, min_hits)), fraction
        assert np.array_equal(got, np.isin(label, kept)), fraction
    st = instance.stats(d_label, None, hit=d_hit, capacity=K)
    assert st.n.cpu().tolist() == list(sizes) and st.hits[:, 0].cpu().tolist() == list(counts) and not st.hits[:, 1:].any()
    assert not st.centroid.any() and not st.cov.any() and st.feature is None
    # a capacity that is too small degrades: the instances above it are in no instance
    small = instance.select(d_label, d_hit, 0.5, capacity=3).cpu().numpy()
    assert np.array_equal(small, np.isin(label, [0, 2]))
    keep = torch.tensor([True, False, True], device=dev)
    assert np.array_equal(instance.rows_of(d_label, keep).cpu().numpy(), np.isin(label, [0, 2]))
    assert instance.rows_of(d_label, torch.zeros(0, dtype=torch.bool, device=dev)).sum().item() == 0


def test_select_over_components_that_min_size_dropped(dev):
    from tests import segment_cases as sc
    c = sc.case("sizes_min3")  # components {3}, {0, 9} dropped; {1, 4, 6} and {2, 5, 7, 8, 10} kept
    seg = segment.components(up(c["idx"]), None, None, 3)
    every = torch.ones(11, dtype=torch.bool, device=dev)
    assert np.flatnonzero(instance.select(seg, every).cpu().numpy()).tolist() == [1, 2, 4, 5, 6, 7, 8, 10]
    two = torch.zeros(11, dtype=torch.bool, device=dev)
    two[[1, 4, 3, 0, 9, 2]] = True  # 2 of 3, and 1 of 5; the dropped rows' hits count for nothing
    assert np.flatnonzero(instance.select(seg, two).cpu().numpy()).tolist() == [1, 4, 6]
    assert np.flatnonzero(instance.select(seg, two, 0.2).cpu().numpy()).tolist() == [1, 2, 4, 5, 6, 7, 8, 10]
    st = instance.stats(seg, None, hit=two)
    assert st.members.K == 2 and st.n.cpu().tolist() == [3, 5] and st.members.rows.cpu().tolist() == [1, 4, 6, 2, 5, 7, 8, 10, -1, -1, -1]


# ---- 5. end to end: a speckled prompt mask on two balls that touch ------------------------------------------------------------------
def test_a_noisy_hit_on_two_touching_balls_selects_exactly_one_ball(dev):
    from goi_hyperplane_amd import cluster
    from goi_hyperplane_amd.render import GaussianSet
    from goi_hyperplane_amd.scene import make_scene
    from goi_hyperplane_amd.semantic import LinearSVM, SemanticModel, select_gaussians, select_instances, svm_score_fn
    P, S = 2000, 16
    rng = np.random.default_rng(5)
    scene = make_scene(P, S=S, sh_degree=1, seed=3, log_scale_mean=-3.0)
    u = rng.standard_normal((P, 3))
    inside = u / np.linalg.norm(u, axis=1, keepdims=True) * (0.5 * rng.random((P, 1)) ** (1 / 3))  # uniform in a ball of radius 0.5
    ball = (np.arange(P) >= P // 2).astype(np.int64)  # ball A: rows 0 .. 999 around (-0.5, 0, 0); ball B around (+0.5, 0, 0)
    scene.means3D = (inside + np.stack([ball - 0.5, 0 * ball, 0 * ball], 1)).astype(np.float32)
    scene.semantics = (np.eye(S)[ball] + 0.01 * rng.standard_normal((P, S))).astype(np.float32)  # e0 or e1, plus noise
    pc = GaussianSet.from_scene(scene, dev)
    xyz, sem = pc.get_xyz.detach(), pc._semantics.detach()
    # positions alone cannot tell the balls apart: one DBSCAN cluster at the graph's own scale
    whole = segment.instances(xyz, None, k=8)
    eps = float(whole.graph[1][:, -1].max().sqrt())
    assert len(set(cluster.dbscan(xyz, eps, 4).cpu().tolist()) - {-1}) == 1
    seg = segment.instances(xyz, sem, k=8, tau=0.5)
    assert seg.count.cpu().tolist() == [2] and np.array_equal(seg.label.cpu().numpy(), ball)
    # a deterministic noisy per-Gaussian hit: 70 % of A's rows, 10 % of B's
    hit = np.zeros(P, bool)
    hit[rng.permutation(P // 2)[:700]] = True
    hit[P // 2 + rng.permutation(P // 2)[:100]] = True
    got = instance.select(seg, up(hit), min_fraction=0.5).cpu().numpy()
    assert np.array_equal(got, ball == 0), "the noisy hit must become exactly ball A"
    assert (hit != (ball == 0))[: P // 2].mean() == 0.3 and (hit != (ball == 0))[P // 2:].mean() == 0.1  # the raw hit is wrong there
    # the ball's own centroid and box, within the derived bounds
    st = instance.stats(seg, xyz, sem, hit=up(hit))
    assert st.n.cpu().tolist() == [1000, 1000] and st.hits[:, 0].cpu().tolist() == [700, 100]
    pos, f = scene.means3D, scene.semantics
    ptr, rows = ref.members(ball.astype(np.int32), 2)
    ex = ref.exact(ptr, rows, pos, f, None)
    got_st = down(st)
    for k in range(2):
        mine = pos[ball == k]
        assert np.array_equal(got_st["lo"][k], mine.min(0)) and np.array_equal(got_st["hi"][k], mine.max(0))
        for a in range(3):
            assert abs(float(got_st["centroid"][k, a]) - float(ex[k]["centroid"][a])) <= ref.centroid_bound(1000, ex[k]["centroid"][a],
                                                                                                          ex[k]["absd"][a])
        for q, (a, b) in enumerate(ref.PAIRS):
            assert abs(float(got_st["cov"][k, q]) - float(ex[k]["cov"][q])) <= ref.cov_bound(1000, ex[k]["cov"][q], ex[k]["absdd"][q],
                                                                                            ex[k]["absd"][a], ex[k]["absd"][b])
        for ch in range(S):
            assert abs(float(got_st["feature"][k, ch]) - float(ex[k]["feature"][ch])) <= ref.mean_bound(1000, ex[k]["feature"][ch],
                                                                                                       ex[k]["absf"][ch])
    assert abs(got_st["centroid"][0, 0] + 0.5) < 0.05 and abs(got_st["centroid"][1, 0] - 0.5) < 0.05
    # the prompt path: select_instances is instance.select of select_gaussians
    torch.manual_seed(8)
    mlp = SemanticModel(dim_in=S, dim_out=300, num_layer=1, use_bias=True, device=dev)
    pos_code = torch.rand(300, device=dev) < 0.3
    un = torch.nn.functional.normalize(torch.randn(256, device=dev), dim=0)
    lut = torch.randn(300, 256, device=dev) * 0.1 + 0.2 * (2 * pos_code.float() - 1)[:, None] * un[None]
    svm = LinearSVM().to(dev)
    svm.weight_set(un.reshape(1, -1))
    score_fn = svm_score_fn(svm)
    per_gaussian = select_gaussians(pc, mlp, lut, score_fn, 0.5)
    for fraction in (0.5, 0.05):
        objects = select_instances(pc, mlp, lut, score_fn, 0.5, seg, min_fraction=fraction)
        assert objects.dtype == torch.bool and tuple(objects.shape) == (P,)
        assert torch.equal(objects, instance.select(seg, per_gaussian, fraction))
        assert torch.equal(objects, select_instances(pc, mlp, lut, score_fn, 0.5, seg, min_fraction=fraction, capacity=2))
        assert np.array_equal(objects.cpu().numpy(), ref.select(ball.astype(np.int32), 2, per_gaussian.cpu().numpy(), fraction))
