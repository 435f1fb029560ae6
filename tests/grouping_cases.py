"""The cases of goi_hyperplane_amd.grouping's tests (tests/test_grouping_cpu.py, tests/test_gpu_grouping.py): the smallest maps
at which the kernels of csrc/grouping.hip can go wrong.  Every case is a dict(name, tags, feat float32 [S,H,W], labels int32 [H,W],
K, kw) with kw the keyword arguments of grouping.loss_terms; the arrays are read-only and built once.

The constants the implementation introduces, and the cases on both sides of each:
  * a workgroup of 256 threads, a wave of 64 columns: W in {1, 9, 53, 63, 64, 65, 256, 511}
  * grp_sums_k's strips: rows = ceil(H * ceil(W / 64) / 2048) is 1 up to (256, 256), 2 at (257, 511), 3 at (2100, 65)
  * grp_grad_k's 512 workgroups: H * W <= 131072 up to (256, 256), above it at (257, 511) and (2100, 65)
  * the LDS tables of 61440 bytes: the sums' K (S + 1) * 8 and the gradient's K (8 + 12 S); at S = 32 the last K that fits is 232
    and 156, at S = 1 it is 3840 and 3072 -- each with its successor -- and K = 4096 at S = 3 is beyond both.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import grouping_reference as ref

INT_MIN = -2 ** 31
TAGS = ("hw_1x1", "hw_1x63", "hw_1x64", "hw_1x65", "hw_7x9", "hw_16x16", "hw_37x53", "hw_129x65", "hw_256x256", "strip_rows_2",
        "strip_rows_3", "grad_blocks_capped", "S1", "S3", "S16", "S17", "S32", "K0", "K1", "K2", "K5", "K300_mostly_empty",
        "K_above_both_tables", "sums_table_last", "sums_table_first_without", "grad_table_last", "grad_table_first_without",
        "uniform", "half_plane", "checkerboard", "voronoi", "random64", "all_ignored", "one_pixel_mask", "ignored_minus1",
        "ignored_K", "ignored_int_min", "twin_masks_d0", "exactly_margin", "beyond_margin", "offset_1000", "all_zero", "max_abs_enough",
        "max_abs_exceeded", "balance_pixel", "balance_mask", "w_inter_0")


def _voronoi(H, W, ids, rng):
    """every pixel takes the id of the nearest of len(ids) random sites"""
    sites = rng.random((len(ids), 2)) * (H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - sites[:, 0]) ** 2 + (xx[..., None] - sites[:, 1]) ** 2
    return np.asarray(ids, np.int32)[d.argmin(-1)]


def _features(S, labels, K, rng, offset=0.0):
    """unit-ish noise about a per-mask centre; the centres are about one margin apart, so that some pairs pull and some do not"""
    H, W = labels.shape
    centres = rng.standard_normal((max(K, 1) + 1, S)) * (0.8 / np.sqrt(S))
    inside = (labels >= 0) & (labels < K)
    c = centres[np.where(inside, labels, K)]  # (ignored pixels share the spare centre)
    f = c + 0.5 * rng.standard_normal((H, W, S)) / np.sqrt(S) + offset
    return np.ascontiguousarray(f.transpose(2, 0, 1)).astype(np.float32)


def _case(name, tags, feat, labels, K, **kw):
    feat, labels = np.ascontiguousarray(feat, np.float32), np.ascontiguousarray(labels, np.int32)
    feat.setflags(write=False)
    labels.setflags(write=False)
    return dict(name=name, tags=set(tags), feat=feat, labels=labels, K=K, kw=kw)


def _sprinkle(labels, K, rng, values, share=0.1):
    out = labels.copy()
    at = rng.random(labels.shape) < share
    out[at] = rng.choice(np.asarray(values, np.int64), int(at.sum())).astype(np.int32)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(11)
    out = []

    def add(name, tags, S, labels, K, feat=None, offset=0.0, **kw):
        labels = np.asarray(labels, np.int32)
        out.append(_case(name, tags, _features(S, labels, K, rng, offset) if feat is None else feat, labels, K, **kw))

    add("one_pixel", ["hw_1x1", "S1", "K1", "uniform"], 1, np.zeros((1, 1)), 1)
    add("row63_half", ["hw_1x63", "S3", "K2", "half_plane"], 3, (np.arange(63) >= 20)[None, :], 2)
    add("row64_checker", ["hw_1x64", "S16", "checkerboard"], 16, (np.arange(64) & 1)[None, :], 2, balance="mask")
    add("row65_cells", ["hw_1x65", "S17", "K5", "voronoi"], 17, _voronoi(1, 65, range(5), rng), 5)
    small = _sprinkle(_voronoi(7, 9, range(5), rng), 5, rng, [-1, 5, INT_MIN], 0.25)
    small[0, :3] = (-1, 5, INT_MIN)
    add("small_ignored", ["hw_7x9", "S32", "ignored_minus1", "ignored_K", "ignored_int_min", "balance_pixel"], 32, small, 5)
    add("K0", ["hw_16x16", "K0"], 16, _voronoi(16, 16, range(4), rng), 0)
    add("all_ignored", ["all_ignored"], 3, rng.choice([-1, 5, 77, INT_MIN], (16, 16)), 5)
    cells = _voronoi(37, 53, np.sort(rng.choice(300, 12, replace=False)), rng)
    add("odd_K300", ["hw_37x53", "K300_mostly_empty", "balance_mask"], 16, cells, 300, balance="mask")
    add("tall_random64", ["hw_129x65", "random64"], 17, rng.integers(0, 64, (129, 65)), 64)
    add("tall_checker", ["checkerboard"], 3, (np.add.outer(np.arange(129), np.arange(65)) & 1), 2)
    big = _voronoi(256, 256, range(40), rng)
    big[big == 39] = 38
    big[100, 200] = 39  # a mask of exactly one pixel
    add("big_cells", ["hw_256x256", "one_pixel_mask", "voronoi"], 16, big, 40)
    add("big_uniform", ["uniform"], 16, np.zeros((256, 256)), 1)
    add("strips_2", ["strip_rows_2", "grad_blocks_capped"], 1, _voronoi(257, 511, range(7), rng), 7)
    add("strips_3", ["strip_rows_3", "half_plane"], 1, np.repeat((np.arange(2100) >= 777)[:, None] * 2, 65, 1), 3)
    # two masks of the same multiset of pixel values (eighths: every sum is exact in any order), a third far away
    vals = rng.integers(-8, 9, (64, 3)) / 8.0
    lab = np.full((16, 16), 2)
    lab.reshape(-1)[:64], lab.reshape(-1)[64:128] = 0, 1
    f = np.zeros((256, 3))
    f[:64], f[64:128], f[128:] = vals, vals[rng.permutation(64)], vals[rng.integers(0, 64, 128)] + (4.0, 0, 0)
    add("twins", ["twin_masks_d0", "beyond_margin"], 3, lab, 3, feat=f.T.reshape(3, 16, 16))
    # means exactly one margin apart along the first axis, and a third mask five margins away
    lab = np.repeat(np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])[None, :], 7, 0)
    f = np.zeros((7, 9, 3))
    f[..., 0] = np.array([0, 0, 0, 1, 1, 1, 5, 5, 5])
    f[..., 1] = np.where(np.arange(7)[:, None] % 2 == 0, 0.25, -0.25) * (np.arange(7)[:, None] < 6)  # (mean 0 on every mask)
    add("at_margin", ["exactly_margin", "beyond_margin"], 3, lab, 3, feat=f.transpose(2, 0, 1))
    five = _voronoi(37, 53, range(5), rng)
    add("offset_1000", ["offset_1000"], 16, five, 5, offset=1000.0)
    add("zeros", ["all_zero"], 3, _voronoi(16, 16, range(2), rng), 2, feat=np.zeros((3, 16, 16)))
    f5 = _features(16, five, 5, rng)
    add("max_abs_enough", ["max_abs_enough"], 16, five, 5, feat=f5, max_abs=8.0)
    add("max_abs_exceeded", ["max_abs_exceeded"], 16, five, 5, feat=f5, max_abs=0.25)
    add("w_inter_0", ["w_inter_0"], 16, five, 5, feat=f5, w_inter=0.0, w_intra=0.5, margin=2.0)
    add("margin_2_mask", ["balance_mask"], 16, five, 5, feat=f5, margin=2.0, w_inter=3.0, balance="mask")
    for K, tag in ((232, "sums_table_last"), (233, "sums_table_first_without"), (156, "grad_table_last"), (157, "grad_table_first_without")):
        add(f"S32_K{K}", [tag], 32, rng.integers(K - 40, K, (7, 9)), K)
    for K, tag in ((3840, "sums_table_last"), (3841, "sums_table_first_without"), (3072, "grad_table_last"),
                   (3073, "grad_table_first_without")):
        add(f"S1_K{K}", [tag], 1, rng.choice(np.r_[0, K - 1, rng.integers(0, K, 6)], (16, 16)), K)
    add("S3_K4096", ["K_above_both_tables"], 3, rng.choice(np.r_[4095, rng.integers(0, 4096, 20)], (16, 16)), 4096)
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def names():
    return [c["name"] for c in cases()]


def case(name):
    return next(c for c in cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """ref.terms of the case: computed once, shared, never written to"""
    c = case(name)
    return ref.terms(c["feat"], c["labels"], c["K"], **c["kw"])


@functools.lru_cache(maxsize=None)
def twin(name):
    c = case(name)
    return ref.twin(c["feat"], c["labels"], c["K"], **{k: v for k, v in c["kw"].items() if k != "max_abs"})
