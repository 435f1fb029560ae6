"""The named cases the CPU and GPU tests of goi_hyperplane_amd.instance share (tests/test_instance_cpu.py,
tests/test_gpu_instance.py).

A case is a dict: name, label int32 [P], K, xyz float32 [P,3], features float32 [P,S] or None, weight float32 [P] or None, hit
uint8 / bool [P] or None, and `tags`, the bullets of the case list it covers.  Built once per process from fixed seeds, never
modified, all with P <= 20000.  The shapes are the smallest at which the kernels can still go wrong: a quarter wave walks a chunk
of 256 members in batches of 16, four at a time (sizes 0, 1, 3, 4, 5 around the batch of four; 255, 256, 257 around one chunk and
around the threshold between inst_small_k and the slot path; 511, 512, 513 around two chunks; 5000 = 20 chunks); the slot path
exists only for P > 256 (cases on both sides); lane l holds channels l and l + 16 (S = 1, 3, 16, 17, 32)."""
from __future__ import annotations

import functools

import numpy as np

TAGS = ("size_0", "size_1", "size_3", "size_4", "size_5", "size_255", "size_256", "size_257", "size_511", "size_512", "size_513",
        "size_5000", "interleaved", "K_1", "K_equals_P", "K_larger", "K_smaller", "label_minus_one", "label_int_min", "P_0", "K_0",
        "S_1", "S_3", "S_16", "S_17", "S_32", "no_features", "weight_absent", "weight_positive", "weight_zero_instance",
        "weight_zero_pivot", "hit_all_patterns", "hit_bool", "hit_absent", "far_pivot", "nan_position", "twins", "real_partition",
        "P_at_most_256")
ALL_SIZES = (1, 3, 0, 4, 5000, 5, 255, 256, 0, 257, 511, 512, 513)  # the size of instance k (two empty ones inside)
MID_SIZES = (3, 0, 257, 1, 4, 5, 255, 256, 513)
INT_MIN = -2 ** 31


def partition(sizes, seed, outside=()):
    """label int32 [P]: instance k has sizes[k] rows, plus one row per entry of `outside` (labels in no instance), the rows
    shuffled so that every instance's members are spread over the array"""
    rng = np.random.default_rng(seed)
    label = np.concatenate([np.full(s, k, np.int64) for k, s in enumerate(sizes)] + [np.asarray(outside, np.int64)])
    return rng.permutation(label).astype(np.int32)


def fields(P, seed, S=None, weight=None, hit=None, centre=0.0, extent=1.0):
    rng = np.random.default_rng(seed)
    xyz = (centre + extent * rng.standard_normal((P, 3))).astype(np.float32)
    f = None if S is None else rng.standard_normal((P, S)).astype(np.float32)
    w = None
    if weight == "positive":
        w = (0.05 + rng.random(P)).astype(np.float32)
    h = None
    if hit == "patterns":
        h = rng.permutation(np.arange(P) % 256).astype(np.uint8)
    elif hit == "bool":
        h = rng.random(P) < 0.4
    return xyz, f, w, h


def _case(name, label, K, tags, xyz, features=None, weight=None, hit=None):
    assert set(tags) <= set(TAGS) and label.shape[0] <= 20000
    return dict(name=name, label=label, K=int(K), tags=frozenset(tags), xyz=xyz, features=features, weight=weight, hit=hit)


def _sizes_tags(sizes):
    return tuple(f"size_{s}" for s in sizes if f"size_{s}" in TAGS) + ("interleaved",)


TWIN_N = 600  # members of a twin: three chunks


def _twins():
    """Two cases that share ONE instance's member values: in `twins` instances 2 and 7 (of K = 9) hold the same 600 (position,
    feature, weight, hit) values in the same order at different row ids; in `twins_K3` the same values are instance 1 of K = 3
    among other rows.  All three must give identical bits."""
    rng = np.random.default_rng(77)
    vx, vf, vw, vh = fields(TWIN_N, 78, S=16, weight="positive", hit="patterns", centre=3.0)
    out = []
    for name, sizes, twins, seed in (("twins", (5, 40, TWIN_N, 300, 2, 0, 17, TWIN_N, 90), (2, 7), 79),
                                     ("twins_K3", (700, TWIN_N, 33), (1,), 80)):
        label = partition(sizes, seed, outside=(-1,) * 20)
        P = label.shape[0]
        xyz, f, w, h = fields(P, seed + 100, S=16, weight="positive", hit="patterns", centre=3.0)
        for k in twins:
            at = np.flatnonzero(label == k)  # ascending row id: the member order
            xyz[at], f[at], w[at], h[at] = vx, vf, vw, vh
        out.append(_case(name, label, len(sizes), ("twins", "S_16", "weight_positive", "hit_all_patterns", "label_minus_one"),
                         xyz, f, w, h))
    del rng
    return out


def _real_partition():
    """segment_cases' clustered cloud of 5000 points through the restated segment.components (min_size = 5: dropped rows are -1)"""
    from tests import segment_cases as sc
    c = sc.case("knn_P5000_k8_S16")
    _, _, _, label, count = sc.reference("knn_P5000_k8_S16")
    rng = np.random.default_rng(5)
    return _case("real_partition_P5000", np.array(label, np.int32), count, ("real_partition", "S_16", "label_minus_one", "hit_bool",
                                                                           "weight_absent"),
                 np.array(c["xyz"]), np.array(c["f"]), None, rng.random(5000) < 0.3)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # every size class in one label array, S = 16, weights, eight hit bits; rows of -1, INT32_MIN and of a label >= K among them
    K = len(ALL_SIZES)
    label = partition(ALL_SIZES, 1, outside=(-1,) * 30 + (INT_MIN,) * 7 + (K, K + 3, 2 ** 31 - 1))
    xyz, f, w, h = fields(label.shape[0], 2, S=16, weight="positive", hit="patterns")
    out.append(_case("all_sizes_S16", label, K, _sizes_tags(ALL_SIZES) + ("S_16", "weight_positive", "hit_all_patterns",
                                                                        "label_minus_one", "label_int_min", "K_smaller"),
                     xyz, f, w, h))
    # the channel counts, on the middle sizes
    mid = partition(MID_SIZES, 3, outside=(-1, -1, INT_MIN))
    Pm, Km = mid.shape[0], len(MID_SIZES)
    for S in (1, 3, 17, 32):
        xyz, f, w, h = fields(Pm, 10 + S, S=S, weight="positive", hit="patterns")
        out.append(_case(f"mid_sizes_S{S}", mid, Km, _sizes_tags(MID_SIZES) + (f"S_{S}", "weight_positive", "hit_all_patterns"),
                         xyz, f, w, h))
    xyz, f, w, h = fields(Pm, 20, hit="bool")
    out.append(_case("mid_sizes_plain", mid, Km, _sizes_tags(MID_SIZES) + ("no_features", "weight_absent", "hit_bool"),
                     xyz, None, None, h))
    xyz, f, w, h = fields(Pm, 21, S=3)
    out.append(_case("mid_sizes_no_hit", mid, Km, ("S_3", "weight_absent", "hit_absent"), xyz, f, None, None))
    # K against the labels in use
    out.append(_case("K_larger", mid, Km + 5, ("K_larger", "S_3"), *fields(Pm, 22, S=3, weight="positive", hit="bool")))
    out.append(_case("K_smaller", mid, 4, ("K_smaller", "S_3"), *fields(Pm, 23, S=3, weight="positive", hit="bool")))
    one = np.where(np.arange(700) % 7 == 3, -1, 0).astype(np.int32)
    out.append(_case("K_1", one, 1, ("K_1", "label_minus_one", "S_17"), *fields(700, 24, S=17, weight="positive", hit="patterns")))
    out.append(_case("K_equals_P_singletons", np.random.default_rng(25).permutation(300).astype(np.int32), 300,
                     ("K_equals_P", "size_1", "S_16"), *fields(300, 26, S=16, weight="positive", hit="patterns")))
    out.append(_case("small_P200", partition((60, 0, 100, 1, 30), 27, outside=(-1,) * 9), 5, ("P_at_most_256", "S_32"),
                     *fields(200, 28, S=32, weight="positive", hit="patterns")))
    # empty calls
    out.append(_case("P_0", np.zeros(0, np.int32), 3, ("P_0", "size_0", "S_16"), *fields(0, 29, S=16, weight="positive", hit="bool")))
    out.append(_case("K_0", partition((4, 6), 30), 0, ("K_0", "S_3"), *fields(10, 31, S=3, weight="positive", hit="bool")))
    # weights: an instance whose weights are all zero (the 257 one and a singleton), and a zero on pivot rows
    xyz, f, w, h = fields(Pm, 32, S=16, weight="positive", hit="patterns")
    w[(mid == 2) | (mid == 3)] = 0.0
    for k in (4, 7, 8):
        w[np.flatnonzero(mid == k)[0]] = 0.0
    out.append(_case("zero_weights", mid, Km, ("weight_zero_instance", "weight_zero_pivot", "S_16"), xyz, f, w, h))
    # the pivot: a scene 1000 units from the origin, 0.01 across
    out.append(_case("far_pivot", mid, Km, ("far_pivot", "S_3"), *fields(Pm, 33, S=3, weight="positive", hit="bool", centre=1000.0,
                                                                          extent=0.01)))
    # one NaN position (not a pivot row): lo / hi skip it, the sums of that axis are NaN
    xyz, f, w, h = fields(Pm, 34, S=3, weight="positive", hit="bool")
    xyz[np.flatnonzero(mid == 8)[100], 1] = np.nan
    xyz[np.flatnonzero(mid == 6)[5], 2] = -0.0
    out.append(_case("nan_position", mid, Km, ("nan_position", "S_3"), xyz, f, w, h))
    out.extend(_twins())
    out.append(_real_partition())
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
def reference(name):
    """(ptr, rows, the stats dict) of a case by the restatement, computed once and shared, read-only"""
    from tests import instance_reference as ref
    c = case(name)
    ptr, rows = ref.members(c["label"], c["K"])
    st = ref.stats(ptr, rows, c["xyz"], c["features"], c["weight"], c["hit"])
    for a in (ptr, rows) + tuple(v for v in st.values() if v is not None):
        a.setflags(write=False)
    return ptr, rows, st
