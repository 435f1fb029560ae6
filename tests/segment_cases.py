"""The named cases the CPU and GPU tests of goi_hyperplane_amd.segment share (tests/test_segment_cpu.py, tests/test_gpu_segment.py).

A case is a dict: name, idx [P,k] int32, the arguments of the gate -- f [P,S] float32 or None, tau, dist2 [P,k] or None,
max_dist2 or None, labels int64 [P] or None, rows bool [P] or None, mutual -- and of the partition -- gate (False: components is
called WITHOUT a join), join (None: what the gate gives; an array: that one instead, for the rows case), min_size -- plus `tags`,
the bullets of the case list it covers, and for a few hand-made ones `expect_join` / `expect_parts`.  xyz [P,3] where the graph is
that of a cloud.  Built once per process from fixed seeds, never modified.  The shapes are the smallest at which the kernels can
still go wrong: a lane per edge and per row in workgroups of 256 and waves of 64 (P = 0, 1, 2, 63, 64, 65, 257, 5000), rows read
as 16-byte words or float by float (S = 4, 16, 32 against 1, 3, 17), one giant component (the star), long parent chains (the
paths)."""
from __future__ import annotations

import functools

import numpy as np

from tests import knn_graph_reference as kref

# every bullet of the case list: test_segment_cpu.py asserts that the table covers them all
TAGS = ("knn_cloud", "tails", "empty_rows", "out_of_range", "self_edges", "duplicates", "star", "path_ascending", "path_descending",
        "path_shuffled", "directed_bridge", "mutual_on", "mutual_off", "rows_articulation", "labels_equal", "labels_differ",
        "labels_minus_one", "tie_tau_joins", "tie_tau_below", "tie_dist2_joins", "tie_dist2_below", "nan_feature", "tau_inf",
        "min_size_equal", "min_size_above", "min_size_above_all", "order", "no_join")
P_SET, K_SET, S_SET = {0, 1, 2, 63, 64, 65, 257, 5000}, {1, 3, 8, 16}, {1, 3, 4, 16, 17, 32}


def _case(name, idx, tags, f=None, tau=np.inf, dist2=None, max_dist2=None, labels=None, rows=None, mutual=False, gate=True,
          join=None, min_size=1, **extra):
    idx = np.ascontiguousarray(idx, np.int32)
    assert idx.ndim == 2 and set(tags) <= set(TAGS)
    return dict(name=name, idx=idx, tags=frozenset(tags), f=f, tau=float(tau), dist2=dist2, max_dist2=max_dist2, labels=labels,
                rows=rows, mutual=mutual, gate=gate, join=join, min_size=min_size, **extra)


def cloud(P, seed, S):
    """a clustered cloud (the shape of tools/knn_time.py's) whose features follow the clusters: a vector per centre plus 0.1
    noise, so that an edge inside a blob has d around 0.02 S and one between two blobs around 2 S"""
    rng = np.random.default_rng(seed)
    nc = max(P // 40, 2)
    which = rng.integers(0, nc, P)
    xyz = (rng.standard_normal((nc, 3))[which] * 5 + 0.3 * rng.standard_normal((P, 3))).astype(np.float32)
    f = (rng.standard_normal((nc, S))[which] + 0.1 * rng.standard_normal((P, S))).astype(np.float32)
    return xyz, f, which.astype(np.int64)


def _knn_case(P, k, S, seed, tags=(), tau=None, cut=False, with_labels=False, with_rows=False, **kw):
    rng = np.random.default_rng(seed + 1000)
    xyz, f, which = cloud(P, seed, S)
    idx, dist2 = kref.knn_rows(xyz, xyz, k, exclude_self=True)
    labels = rows = None
    if with_labels:
        labels = which % 3
        labels[rng.random(P) < 0.1] = -1
    if with_rows:
        rows = rng.random(P) < 0.8
    return _case(f"knn_P{P}_k{k}_S{S}", idx, ("knn_cloud",) + tuple(tags), f=f, tau=0.03 * S if tau is None else tau,
                 dist2=dist2 if cut else None, max_dist2=float(np.median(dist2[np.isfinite(dist2)])) if cut else None,
                 labels=labels, rows=rows, xyz=xyz, **kw)


def _random_case(name, P, k, S, seed, tags, edit, **kw):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, P, (P, k)).astype(np.int32)
    edit(rng, idx)
    f = rng.integers(0, 3, (P, S)).astype(np.float32) + (0.1 * rng.standard_normal((P, S))).astype(np.float32)
    return _case(name, idx, tags, f=f, tau=1.0 * S, **kw)


def _tails(rng, idx):  # -1 tails of random length, and whole -1 rows
    P, k = idx.shape
    length = rng.integers(0, k + 1, P)
    length[rng.random(P) < 0.1] = 0
    idx[np.arange(k)[None, :] >= length[:, None]] = -1


def _out_of_range(rng, idx):  # ids >= P (and negative ones other than -1) that never join
    P, k = idx.shape
    bad = rng.random((P, k)) < 0.25
    idx[bad] = rng.choice(np.array([P, P + 5, 2 ** 31 - 1, -7, -2 ** 31], np.int64), int(bad.sum())).astype(np.int32)


def _self_edges(rng, idx):
    idx[:, 0] = np.arange(idx.shape[0])


def _duplicates(rng, idx):
    idx[:, 1::2] = idx[:, 0::2][:, :idx[:, 1::2].shape[1]]


def _path(order):
    """k = 1: row order[t] lists order[t + 1], the last row lists nobody"""
    idx = np.full((len(order), 1), -1, np.int32)
    idx[order[:-1], 0] = order[1:]
    return idx


def _blobs_and_bridge():
    """two rings of 40 rows (every row lists its next three), and ONE edge between them, in row 5's last slot: 5 -> 60; row 60
    does not list row 5"""
    idx = np.full((80, 4), -1, np.int32)
    for base in (0, 40):
        i = np.arange(40)
        for s in range(3):
            idx[base + i, s] = base + (i + s + 1) % 40
    idx[5, 3] = 60
    return idx


def _sizes_graph():
    """chains (k = 1, each row lists the next of its chain) of sizes 1, 2, 3, 5 over interleaved ids, so that dense labels in
    ascending ROOT order are not the order of first appearance of anything else: {3}, {0, 9}, {1, 6, 4}, {2, 10, 5, 8, 7}"""
    idx = np.full((11, 1), -1, np.int32)
    for chain in ([3], [9, 0], [6, 1, 4], [10, 2, 5, 8, 7]):
        idx[chain[:-1], 0] = chain[1:]
    return idx


SIZES_PARTS = [{3}, {0, 9}, {1, 4, 6}, {2, 5, 7, 8, 10}]


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(99)
    tie_f = np.array([[0, 0, 0], [1, 2, 2]], np.float32)  # e = (1, 2, 2): d = 1 + 4 + 4 = 9 exactly
    tie_idx = np.array([[1], [0]], np.int32)
    below9 = float(np.nextafter(np.float32(9), np.float32(0)))
    nine = np.full((2, 1), 9, np.float32)
    xyz63, f63, _ = cloud(63, 21, 16)
    f_nan = f63.copy()
    f_nan[7, 2] = np.nan
    idx63 = kref.knn_rows(xyz63, xyz63, 8, exclude_self=True)[0]
    line = np.array([[1, -1], [0, 2], [1, 3], [2, 4], [3, -1]], np.int32)  # 0 - 1 - 2 - 3 - 4, both endpoints list every edge
    pairs = np.array([[1], [0], [3], [-1]], np.int32)  # 0 <-> 1 list each other; 2 -> 3 only
    lab_idx = np.array([[1], [-1], [3], [-1], [5], [-1], [7], [-1], [9], [-1]], np.int32)
    lab = np.array([3, 3, 1, 2, -1, 2, 2, -1, -1, -1], np.int64)
    shuffled = rng.permutation(4999)
    out = [
        _case("knn_P0_k3_S4", np.zeros((0, 3), np.int32), ("knn_cloud",), f=np.zeros((0, 4), np.float32), tau=1.0),
        _knn_case(1, 1, 1, 1, tags=("empty_rows",)),               # one point: its row is all -1
        _knn_case(2, 3, 3, 2, tags=("tails",)),                    # one neighbour each, -1 tails
        _knn_case(63, 8, 16, 3),
        _knn_case(64, 16, 17, 4),
        _knn_case(65, 3, 32, 5, cut=True, mutual=True, tags=("mutual_on",)),
        _knn_case(257, 8, 4, 6, with_labels=True, with_rows=True, min_size=3),
        _knn_case(5000, 8, 16, 7, min_size=5),
        _knn_case(5000, 16, 1, 8, mutual=True, cut=True, tags=("mutual_on",)),
        _knn_case(257, 3, 3, 9, tau=np.inf, tags=("tau_inf",)),
        _random_case("tails_P257_k8_S17", 257, 8, 17, 10, ("tails", "empty_rows"), _tails),
        _random_case("out_of_range_P65_k3_S16", 65, 3, 16, 11, ("out_of_range",), _out_of_range),
        _random_case("self_edges_P64_k3_S32", 64, 3, 32, 12, ("self_edges",), _self_edges),
        _random_case("duplicates_P63_k8_S3", 63, 8, 3, 13, ("duplicates",), _duplicates),
        _random_case("random_P257_k16_S1_mutual", 257, 16, 1, 14, ("mutual_on",), lambda r, i: None, mutual=True),
        # partition shapes (no features: every valid edge joins; the first without a join array at all)
        _case("star_P5000_k1", np.r_[-1, np.zeros(4999, np.int64)].reshape(5000, 1), ("star", "no_join"), gate=False,
              expect_parts=[set(range(5000))]),
        _case("star_P5000_k1_gated", np.r_[-1, np.zeros(4999, np.int64)].reshape(5000, 1), ("star",),
              expect_parts=[set(range(5000))]),
        _case("path_ascending_P4999", _path(np.arange(4999)), ("path_ascending",), expect_parts=[set(range(4999))]),
        _case("path_descending_P4999", _path(np.arange(4999)[::-1]), ("path_descending",), expect_parts=[set(range(4999))]),
        _case("path_shuffled_P4999", _path(shuffled), ("path_shuffled",), expect_parts=[set(range(4999))]),
        _case("blobs_and_bridge", _blobs_and_bridge(), ("directed_bridge", "mutual_off"), expect_parts=[set(range(80))]),
        _case("blobs_and_bridge_mutual", _blobs_and_bridge(), ("mutual_on",), mutual=True,  # (no ring edge is mutual either)
              expect_parts=[{i} for i in range(80)]),
        _case("pairs_mutual_off", pairs, ("mutual_off",), expect_join=[[1], [1], [1], [0]], expect_parts=[{0, 1}, {2, 3}]),
        _case("pairs_mutual_on", pairs, ("mutual_on",), mutual=True, expect_join=[[1], [1], [0], [0]],
              expect_parts=[{0, 1}, {2}, {3}]),
        # rows: zero at the articulation row of a line; the join array says 1 for every edge all the same
        _case("rows_articulation", line, ("rows_articulation",), rows=np.array([1, 1, 0, 1, 1], bool),
              join=np.ones((5, 2), np.uint8), expect_parts=[{0, 1}, {3, 4}]),
        _case("rows_articulation_gated", line, ("rows_articulation",), rows=np.array([1, 1, 0, 1, 1], bool),
              expect_join=[[1, 0], [1, 0], [0, 0], [0, 1], [1, 0]], expect_parts=[{0, 1}, {3, 4}]),
        _case("line_whole", line, ("mutual_on",), mutual=True, expect_parts=[{0, 1, 2, 3, 4}]),
        _case("labels", lab_idx, ("labels_equal", "labels_differ", "labels_minus_one"), labels=lab,
              expect_join=[[1], [0], [0], [0], [0], [0], [0], [0], [0], [0]],
              expect_parts=[{0, 1}] + [{i} for i in range(2, 10)]),
        # threshold ties
        _case("tie_tau_joins", tie_idx, ("tie_tau_joins",), f=tie_f, tau=9.0, expect_join=[[1], [1]], expect_parts=[{0, 1}]),
        _case("tie_tau_below", tie_idx, ("tie_tau_below",), f=tie_f, tau=below9, expect_join=[[0], [0]], expect_parts=[{0}, {1}]),
        _case("tie_dist2_joins", tie_idx, ("tie_dist2_joins",), dist2=nine, max_dist2=9.0, expect_join=[[1], [1]],
              expect_parts=[{0, 1}]),
        _case("tie_dist2_below", tie_idx, ("tie_dist2_below",), dist2=nine, max_dist2=below9, expect_join=[[0], [0]],
              expect_parts=[{0}, {1}]),
        # special values: a NaN feature on row 7 -- no edge of row 7 joins, whichever side lists it -- under tau = +inf
        _case("nan_feature_tau_inf_P63_k8_S16", idx63, ("nan_feature", "tau_inf", "knn_cloud"), f=f_nan, tau=np.inf),
        # min_size against components of 1, 2, 3 and 5 rows; ascending-root labels
        _case("sizes_min1", _sizes_graph(), ("order",), min_size=1, expect_parts=SIZES_PARTS, expect_labels=[3, 0, 1, 2]),
        _case("sizes_min3", _sizes_graph(), ("min_size_equal", "order"), min_size=3, expect_parts=SIZES_PARTS,
              expect_labels=[-1, -1, 0, 1]),
        _case("sizes_min4", _sizes_graph(), ("min_size_above",), min_size=4, expect_parts=SIZES_PARTS, expect_labels=[-1, -1, -1, 0]),
        _case("sizes_min6", _sizes_graph(), ("min_size_above_all",), min_size=6, expect_parts=SIZES_PARTS,
              expect_labels=[-1, -1, -1, -1]),
    ]
    for c in out:
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def gate_args(c):
    """the keyword arguments of edges() -- the restatement's and the module's alike"""
    return dict(features=c["f"], tau=c["tau"], dist2=c["dist2"], max_dist2=c["max_dist2"], labels=c["labels"], rows=c["rows"],
                mutual=c["mutual"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(join uint8 [P,k] or None, root, size, label, count) of a case by the restatement, computed once and shared"""
    from tests import segment_reference as ref
    c = case(name)
    join = ref.edges(c["idx"], **gate_args(c)) if c["gate"] else None
    used = c["join"] if c["join"] is not None else join
    root, size, label, count = ref.components(c["idx"], used, c["rows"], c["min_size"])
    for a in (join, root, size, label):
        if a is not None:
            a.setflags(write=False)
    return join, root, size, label, count
