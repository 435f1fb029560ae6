"""The mask stage of the camera sweeps without a GPU.

The dilation's reference is the clipped-window definition (tests/mask_reference.py) checked here against
scipy.ndimage.binary_dilation(m, np.ones((k, k)), iterations=n) with its default border_value=0, which is documented as
the same operation: cv2 (the reference's cv2.dilate(m, np.ones((k, k)), iterations=n) >= 0.5) is not a dependency of this
project, so the dilation cannot be pinned to cv2 itself.  cv2's default border value for dilation never contributes, and
a k x k rectangle iterated n times is one rectangle of side n (k - 1) + 1, which is the window above.

The metric formulas (masks.segmentation_metrics, the host-side helper on counts) are checked bit for bit against the
reference's own calculate_iou / calculate_mean_pixel_accuracy / calculate_mean_precision pinned in
tests/golden/ref_mask_metric_pins.npz (tests/golden/make_mask_golden.py), NaN and 0 included; the camera filter
(semantic.relevant_keep) against the reference's removal loop; and the public entry points validate their arguments and
refuse CPU tensors."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.mask_reference import confusion_reference, dilate_reference, metrics_reference, relevant_reference

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def pins():
    return np.load(os.path.join(GOLD, "ref_mask_metric_pins.npz"))


def pin_masks(pins, name):
    shape = tuple(int(v) for v in pins[f"{name}_shape"])
    n = shape[0] * shape[1]
    unpack = lambda a: np.unpackbits(a, count=n).astype(bool).reshape(shape)  # noqa: E731
    return unpack(pins[f"{name}_pred"]), unpack(pins[f"{name}_gt"])


def scipy_dilate(m, k, n):
    return ndimage.binary_dilation(m, structure=np.ones((k, k), bool), iterations=n, border_value=0)


@pytest.mark.parametrize("shape", [(64, 64), (1, 65), (37, 1), (63, 129), (100, 97)])
@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
@pytest.mark.parametrize("k,n", [(1, 1), (3, 1), (3, 5), (5, 2), (7, 3)])
def test_dilate_reference_equals_scipy(shape, density, k, n):
    rng = np.random.default_rng(hash((shape, density, k, n)) % 2 ** 32)
    m = rng.random(shape) < density
    assert np.array_equal(dilate_reference(m, n * (k - 1) // 2), scipy_dilate(m, k, n))


@pytest.mark.parametrize("where", ["corners", "edges", "empty", "full"])
def test_dilate_reference_borders(where):
    H, W = 41, 70
    m = np.zeros((H, W), bool)
    if where == "corners":
        m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    elif where == "edges":
        m[0, 33] = m[20, W - 1] = m[H - 1, 5] = m[7, 0] = True
    elif where == "full":
        m[:] = True
    for k, n in ((3, 5), (3, 1), (9, 2)):
        assert np.array_equal(dilate_reference(m, n * (k - 1) // 2), scipy_dilate(m, k, n))


def test_pins_cover_the_cases(pins):
    names = set(str(n) for n in pins["cases"])
    assert {"empty_gt", "empty_pred", "both_empty", "both_full", "disjoint", "single_pixel", "random_512_sparse",
            "random_512_dense", "big_counts"} <= names
    c = confusion_reference(*pin_masks(pins, "big_counts"))
    assert c[3] > 2 ** 24 and np.float32(c[3]) != c[3]  # the float32 rounding of a count is exercised
    assert np.isnan(pins["both_empty_iou"]) and np.isnan(pins["empty_pred_mp"]) and float(pins["empty_gt_iou"]) == 0.0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_metrics_match_the_pins_bit_for_bit(pins):
    from goi_hyperplane_amd.masks import segmentation_metrics
    names = [str(n) for n in pins["cases"]]
    counts = np.stack([confusion_reference(*pin_masks(pins, n)) for n in names])
    m = segmentation_metrics(torch.from_numpy(counts))
    assert m.iou.dtype == torch.float64 and m.mpa.dtype == torch.float32 and m.mp.dtype == torch.float32
    for i, n in enumerate(names):
        want = (pins[f"{n}_iou"], pins[f"{n}_mpa"], pins[f"{n}_mp"])
        assert same(m.iou[i].numpy(), want[0]), (n, "iou", m.iou[i], want[0])
        assert same(m.mpa[i].numpy(), want[1]), (n, "mpa", m.mpa[i], want[1])
        assert same(m.mp[i].numpy(), want[2]), (n, "mp", m.mp[i], want[2])
        iou, mpa, mp = metrics_reference(counts[i])  # the numpy restatement agrees too
        assert same(np.float64(iou), want[0]) and same(mpa, want[1]) and same(mp, want[2]), n


def test_metrics_take_array_likes():
    from goi_hyperplane_amd.masks import segmentation_metrics
    m = segmentation_metrics([[3, 1, 2, 10]])
    assert float(m.iou[0]) == 3 / 6 and m.mpa.shape == (1,)


@pytest.mark.parametrize("counts,ratio", [
    ([0, 0, 0, 0], 0.1),                           # no camera sees the prompt
    ([7, 7, 7], 0.1),                              # all equal
    ([1000, 100, 99, 101, 0, 1000], 0.1),          # at the 10 % boundary
    ([0, 5, 0, 1, 0], 0.0),                        # min_ratio 0: zero-count cameras still go
    ([30000001, 3000000, 2999999, 3000001, 3000002, 0], 0.1),  # float32 rounding of max * ratio and of the counts
    ([16777217, 1677721, 1677722, 1677723], 0.1),
    ([262144, 1, 26214, 26215], 0.1),
    ([10, 9, 1], 1.0),
])
def test_filter_matches_the_reference_loop(counts, ratio):
    from goi_hyperplane_amd.semantic import relevant_keep
    keep = relevant_keep(torch.tensor(counts, dtype=torch.int64), ratio)
    assert keep.dtype == torch.bool
    assert torch.nonzero(keep).reshape(-1).tolist() == relevant_reference(counts, ratio)


def test_dilate_arguments_are_validated():
    from goi_hyperplane_amd import masks
    m = torch.zeros(4, 4, dtype=torch.bool)
    for k, n in ((2, 1), (4, 3), (0, 1), (-1, 1), (3, 0), (3, -2), (3, 64), (129, 1), (3.5, 1)):
        with pytest.raises(ValueError):
            masks.dilate(m, kernel_size=k, iterations=n)
    assert masks.radius(3, 5) == 5 and masks.radius(1, 9) == 0 and masks.radius(3, 63) == 63 and masks.radius(127, 1) == 63


def test_cpu_tensors_are_refused():
    from goi_hyperplane_amd import masks
    m = torch.zeros(2, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masks.dilate(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masks.pack(torch.zeros(8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masks.confusion(m, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masks.unpack(torch.zeros(2, 8, 1, dtype=torch.int64), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masks.dilate_packed(torch.zeros(2, 8, 1, dtype=torch.int64), 8, 5)


def test_sweeps_refuse_bad_camera_sets():
    from goi_hyperplane_amd.scene import make_camera
    from goi_hyperplane_amd.semantic import evaluate_cameras, relevant_cameras

    class Cam:
        def __init__(self, w, h):
            c = make_camera(w, h)
            self.image_width, self.image_height = c.image_width, c.image_height

    with pytest.raises(ValueError, match="one frame size"):
        relevant_cameras([Cam(64, 48), Cam(64, 40)], None, None, None, None, 0.5, None)
    with pytest.raises(ValueError, match="one frame size"):
        evaluate_cameras([Cam(64, 48), Cam(32, 48)], torch.zeros(2, 48, 64), None, None, None, None, 0.5, None)
    with pytest.raises(ValueError, match="empty"):
        relevant_cameras([], None, None, None, None, 0.5, None)
    with pytest.raises(ValueError):
        relevant_cameras([Cam(64, 48)], None, None, None, None, 0.5, None, kernel_size=2)
