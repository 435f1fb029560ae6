"""The named cases the CPU and GPU tests of goi_hyperplane_amd.smooth share (tests/test_smooth_cpu.py, tests/test_gpu_smooth.py).

A case is a dict: name, f [P,S] float32, idx [P,k] int32, weight [P,k] float32 or None, rows [P] bool or None, and -- for the
graphs of a cloud -- xyz [P,3] and dist2 [P,k].  Built once per process from fixed seeds, never modified.  The shapes are the
smallest at which the kernels can still go wrong: a workgroup works on 16 rows at a time with a quarter wave each (P = 1, 2, 63,
64, 65, 257, 1000: one lane group, a part of a wave, a wave's and a workgroup's tails), a lane holds channels l and l + 16
(S = 1, 3, 16, 17, 32), a list goes through in batches of 16 entries, four at a time (k = 1, 3, 8, 16; in-lists of 0 .. 4999).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import knn_graph_reference as kref


def cloud(P, seed):
    """a clustered cloud: a few centres, tight blobs (the shape of tools/knn_time.py's cloud)"""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((max(P // 40, 2), 3)) * 5
    return (c[rng.integers(0, len(c), P)] + 0.3 * rng.standard_normal((P, 3))).astype(np.float32)


def _features(rng, P, S):
    return rng.standard_normal((P, S)).astype(np.float32)


def _weights(rng, P, k, kind):
    if kind is None:
        return None
    w = rng.random((P, k)).astype(np.float32)
    if kind == "zeros":
        w[rng.random((P, k)) < 0.3] = 0.0
    return w


def _rows(rng, P, kind):
    if kind is None:
        return None
    return np.zeros(P, bool) if kind == "none" else rng.random(P) < 0.5


def _knn_case(P, S, k, seed, weight=None, rows=None):
    rng = np.random.default_rng(seed)
    xyz = cloud(P, seed)
    idx, dist2 = kref.knn_rows(xyz, xyz, k, exclude_self=True)
    if weight == "gaussian":
        w = np.where(np.isfinite(dist2), np.exp(-dist2.astype(np.float64) / (2 * 0.3 ** 2)), 0.0).astype(np.float32)
    else:
        w = _weights(rng, P, k, weight)
    return dict(name=f"knn_P{P}_S{S}_k{k}", f=_features(rng, P, S), idx=idx.astype(np.int32), weight=w, rows=_rows(rng, P, rows),
                xyz=xyz, dist2=dist2)


def _random_case(name, P, S, k, seed, weight=None, rows=None, edit=None):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, P, (P, k)).astype(np.int32)
    if edit:
        edit(rng, idx)
    return dict(name=name, f=_features(rng, P, S), idx=idx, weight=_weights(rng, P, k, weight), rows=_rows(rng, P, rows))


def _tails(rng, idx):  # -1 tails of random length, and whole -1 rows
    P, k = idx.shape
    length = rng.integers(0, k + 1, P)
    length[rng.random(P) < 0.1] = 0
    idx[np.arange(k)[None, :] >= length[:, None]] = -1


def _out_of_range(rng, idx):  # ids >= P (and negative ones other than -1) that must be skipped
    P, k = idx.shape
    bad = rng.random((P, k)) < 0.25
    idx[bad] = rng.choice(np.array([P, P + 5, 2 ** 31 - 1, -7], np.int64), int(bad.sum())).astype(np.int32)


def _self_edges(rng, idx):
    idx[:, 0] = np.arange(idx.shape[0])


def _duplicates(rng, idx):
    idx[:, 1::2] = idx[:, 0::2][:, :idx[:, 1::2].shape[1]]


def _star(rng, idx):  # every other row points at row 0, which points nowhere: an in-list of P - 1
    idx[:] = 0
    idx[0] = -1


def _two_hubs(rng, idx):
    idx[:, 0] = 0
    idx[:, 1] = 1


def _few_targets(rng, idx):  # only the first 50 rows are ever pointed at: every other row has in-degree 0
    idx[:] = rng.integers(0, 50, idx.shape)


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _knn_case(1, 1, 1, 1),                                   # one point: its row is all -1, N_E = 0
        _knn_case(2, 3, 3, 2),                                   # one neighbour each, -1 tails
        _knn_case(63, 16, 8, 3),
        _knn_case(64, 17, 16, 4),
        _knn_case(65, 32, 3, 5, weight="random"),
        _knn_case(257, 3, 8, 6, weight="gaussian", rows="half"),
        _knn_case(1000, 16, 16, 7, weight="zeros", rows="half"),
        _knn_case(1000, 32, 1, 8),
        _random_case("tails_P257_S17_k8", 257, 17, 8, 9, weight="random", edit=_tails),
        _random_case("ids_out_of_range_P65_S16_k3", 65, 16, 3, 10, edit=_out_of_range),
        _random_case("self_edges_P64_S32_k3", 64, 32, 3, 11, weight="random", edit=_self_edges),
        _random_case("duplicates_P63_S3_k8", 63, 3, 8, 12, weight="random", edit=_duplicates),
        _random_case("star_P5000_S16_k1", 5000, 16, 1, 13, edit=_star),
        _random_case("star_weighted_P5000_S3_k1", 5000, 3, 1, 14, weight="zeros", rows="half", edit=_star),
        _random_case("two_hubs_P1000_S17_k16", 1000, 17, 16, 15, weight="random", edit=_two_hubs),
        _random_case("in_degree_0_P257_S1_k3", 257, 1, 3, 16, edit=_few_targets),
        _random_case("rows_all_zero_P65_S16_k3", 65, 16, 3, 17, weight="random", rows="none"),
        _random_case("random_P1000_S1_k16", 1000, 1, 16, 18, weight="zeros", rows="half", edit=_tails),
        _random_case("random_P2_S32_k8", 2, 32, 8, 19, weight="random"),
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


@functools.lru_cache(maxsize=None)
def transposed(name):
    from tests import smooth_reference as ref
    return ref.transpose(case(name)["idx"])


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(L, dL/df, N_E) of a case by the restatement in `dtype`, computed once and shared"""
    from tests import smooth_reference as ref
    c = case(name)
    L, g, ne = ref.loss_and_grad(c["f"], c["idx"], c["weight"], c["rows"], dtype, transposed(name))
    g.setflags(write=False)
    return L, g, ne


@functools.lru_cache(maxsize=None)
def gradient_bound(name):
    from tests import smooth_reference as ref
    c = case(name)
    return ref.grad_bound(c["f"], c["idx"], c["weight"], c["rows"], transposed(name))


def literal_loss(f, idx, weight, rows):
    """the formula as written, on a float64 torch tensor: differentiable"""
    import torch
    from tests import smooth_reference as ref
    cnt = ref.counting_mask(idx, rows)
    i, m = np.nonzero(cnt)
    if len(i) == 0:
        return f.sum() * 0
    j = torch.from_numpy(idx[i, m].astype(np.int64))
    w = torch.ones(len(i), dtype=torch.float64) if weight is None else torch.from_numpy(weight[i, m].astype(np.float64))
    return (w * ((f[torch.from_numpy(i)] - f[j]) ** 2).sum(dim=1)).sum() / len(i)


@functools.lru_cache(maxsize=None)
def autograd64(name):
    """(L, dL/df) of a case by torch autograd in float64 on the CPU, from the literal formula"""
    import torch
    c = case(name)
    f = torch.from_numpy(c["f"].astype(np.float64)).requires_grad_(True)
    L = literal_loss(f, c["idx"], c["weight"], c["rows"])
    L.backward()
    return float(L.detach()), f.grad.numpy()


SMALL = ("knn_P1_S1_k1", "knn_P2_S3_k3", "knn_P63_S16_k8", "ids_out_of_range_P65_S16_k3", "duplicates_P63_S3_k8", "random_P2_S32_k8")
