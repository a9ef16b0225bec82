"""CPU: the host restatement of SemSegEvaluator's Boundary IoU counters (odise_amd/sem_boundary.py) is the evaluator's definition -
`radius` 3x3 erosions behind a one-pixel ring of zeros, pinned here against scipy.ndimage - and the library's radius formula is Python's."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy import ndimage

import __graft_entry__ as entry
from odise_amd import _lib
from odise_amd import sem_boundary as S


def blocky(rng, h, w, K, cell=(5, 7)):
    """A label map of constant rectangles with values in 0..K (K = ignore)."""
    small = rng.integers(0, K + 1, (h // cell[0] + 1, w // cell[1] + 1))
    return np.kron(small, np.ones(cell, np.int64))[:h, :w].astype(np.int32)


def literal_boundary(m, r):
    """_mask_to_boundary as written: zero ring, r erosions whose own border never wins a minimum (cval = 255), ring dropped."""
    p = np.pad(m.astype(np.uint8), 1, constant_values=0)
    for _ in range(r):
        p = ndimage.minimum_filter(p, size=3, mode="constant", cval=255)
    return m - p[1:-1, 1:-1].astype(m.dtype)


@pytest.mark.parametrize("h,w", [(5, 7), (33, 1), (1, 1), (67, 131)])
@pytest.mark.parametrize("K", [1, 20, 150, 254])
def test_closed_form_is_the_repeated_erosion(h, w, K):
    rng = np.random.default_rng(1000 * K + h)
    m = blocky(rng, h, w, K)
    for r in (1, 2, 5, 9):
        got = S.mask_to_boundary(m, r)
        np.testing.assert_array_equal(got, literal_boundary(m, r), err_msg=f"r={r}")
        assert got.min() >= 0 and got.max() <= K
    np.testing.assert_array_equal(S.mask_to_boundary(m), literal_boundary(m, S.boundary_radius(h, w)))


def test_boundary_confusion_counts_label_differences():
    rng = np.random.default_rng(5)
    K, h, w = 20, 67, 131
    pred, gt = blocky(rng, h, w, K - 1), blocky(rng, h, w, K)
    gt[rng.random((h, w)) < 0.05] = 255       # outside [0, K]: the ignore label
    g = np.where(gt == 255, K, gt)
    r = S.boundary_radius(h, w)
    bp, bg = literal_boundary(pred, r), literal_boundary(g, r)
    ref = np.zeros((K + 1, K + 1), np.int64)
    np.add.at(ref, (bp.reshape(-1), bg.reshape(-1)), 1)
    got = S.boundary_confusion(pred, gt, K)
    assert got.dtype == np.int64 and got.sum() == h * w
    np.testing.assert_array_equal(got, ref)
    with pytest.raises(ValueError):
        S.boundary_confusion(pred, gt, 255)


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _lib.load()


def python_radius(h, w):
    return max(1, int(round(0.02 * math.sqrt(h * h + w * w))))


def test_library_radius_is_the_python_formula(lib):
    for h in range(1, 65):
        for w in range(1, 65):
            assert lib.odise_hip_boundary_radius(h, w) == python_radius(h, w) == S.boundary_radius(h, w), (h, w)
    expect = {(480, 640): 16, (512, 683): 17, (1024, 1024): 29, (1280, 1280): 36, (1024, 2560): 55}
    for (h, w), r in expect.items():
        assert lib.odise_hip_boundary_radius(h, w) == python_radius(h, w) == r, (h, w)


def test_library_radius_refuses_an_empty_picture(lib):
    assert lib.odise_hip_boundary_radius(0, 5) < 0
    assert b"boundary_radius" in lib.odise_hip_last_error()
    assert lib.odise_hip_boundary_radius(5, -1) < 0
    with pytest.raises(ValueError):
        S.boundary_radius(0, 5)


def test_prototypes_of_the_boundary_entry_points(lib):
    protos = _lib.header_prototypes()
    assert [len(protos[n]) for n in ("odise_hip_boundary_radius", "odise_hip_label_boundary", "odise_hip_semantic_boundary_confusion")] == [2, 7, 9]
    assert len(lib.odise_hip_semantic_boundary_confusion.argtypes) == 9
    # refused before anything is touched: no context needed to see the class limit
    assert lib.odise_hip_label_boundary(None, None, 255, 4, 4, 0, None) == -1
    assert b"255" in lib.odise_hip_last_error()
