"""Writes tests/golden/ref_pca_pins.npz: sklearn's own PCA(3) on a few float32 inputs (needs scikit-learn >= 1.5; the
pins were made with 1.7.2).  The reference's PCA stage IS this call (gui/main_edit.py:1841-1870 visual_latent,
utils/visual_latent.py:32-40), and the machines the GPU tests run on may not have scikit-learn.

Per case `name`:
    name_x            the float32 input rows [n, S]
    name_mean, name_components, name_explained_variance, name_transform
                      sklearn's fit on the SAME numbers as float64: mean_, components_, explained_variance_, fit_transform
    name_err32        [mean, components, explained variance (relative to the largest), transform]: the largest distance
                      of sklearn's fit on the float32 input itself from the float64 one -- the yardstick for the
                      tolerance of a float32 implementation

    python tests/golden/make_pca_golden.py
"""
import os
import sys

import numpy as np
from sklearn.decomposition import PCA

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.pca_reference import sample  # noqa: E402

CASES = {"s3": (3, 300, 101, 0.0), "s10": (10, 500, 102, 0.0), "s16": (16, 1000, 103, 0.0), "s17": (17, 900, 104, 0.0),
         "s32": (32, 1500, 105, 0.0), "s16_offset": (16, 1000, 103, 100.0)}


def main():
    out = {}
    for name, (S, n, seed, offset) in CASES.items():
        x = sample(S, n, seed, offset)
        p64 = PCA(n_components=3, svd_solver="covariance_eigh")
        t64 = p64.fit_transform(x.astype(np.float64))
        p32 = PCA(n_components=3, svd_solver="covariance_eigh")
        t32 = p32.fit_transform(x)
        assert p32.components_.dtype == np.float32
        out[name + "_x"] = x
        out[name + "_mean"] = p64.mean_
        out[name + "_components"] = p64.components_
        out[name + "_explained_variance"] = p64.explained_variance_
        out[name + "_transform"] = t64
        out[name + "_err32"] = np.array([
            np.abs(p32.mean_ - p64.mean_).max(),
            np.abs(p32.components_ - p64.components_).max(),
            np.abs(p32.explained_variance_ - p64.explained_variance_).max() / p64.explained_variance_[0],
            np.abs(t32 - t64).max()])
        print(name, out[name + "_err32"])
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_pca_pins.npz"), **out)


if __name__ == "__main__":
    main()
