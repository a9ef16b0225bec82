"""The host reference of the polygon rasterisation (odise_amd/coco_poly.py): the literal restatement of maskApi.c rleFrPoly against hand
cases and against the parity formulation the device uses, the union, annToRLE's three forms, and the packing of polygon ground truth."""
import ctypes as C

import numpy as np
import pytest

import inst_cases as IC
import poly_cases as PC
from odise_amd import _lib
from odise_amd import coco_poly as P
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE


def _decode(counts, h, w):
    assert int(np.sum(counts)) == h * w
    return IE.decode_runs(counts, h, w)


@pytest.mark.parametrize("name", sorted(PC.HAND))
def test_hand_cases(name):
    poly, rows = PC.HAND[name]
    want = np.array([[int(c) for c in r] for r in rows], np.uint8)
    np.testing.assert_array_equal(_decode(P.polygon_counts(poly, 5, 6), 5, 6), want)
    np.testing.assert_array_equal(P.polygon_mask(poly, 5, 6), want)


def _check_set(anns, h, w):
    nonempty = 0
    for polys in anns:
        union = np.zeros((h, w), np.uint8)
        parts = []
        for p in polys:
            cnts = P.polygon_counts(p, h, w)
            mask = P.polygon_mask(p, h, w)
            np.testing.assert_array_equal(_decode(cnts, h, w), mask)         # the mask is the parity of the crossings
            np.testing.assert_array_equal(cnts, R.mask_counts(mask))         # and the counts are canonical
            union |= mask
            parts.append(cnts)
        np.testing.assert_array_equal(P.merge_counts(parts, h, w), R.mask_counts(union))
        np.testing.assert_array_equal(P.annotation_to_counts(polys, h, w), R.mask_counts(union))
        nonempty += int(union.any())
    return nonempty


@pytest.mark.parametrize("h,w", PC.SIZES)
def test_literal_and_parity_formulations_agree_on_the_case_set(h, w):
    anns = PC.annotations(h, w)
    nonempty = _check_set(anns, h, w)
    assert nonempty >= len(anns) // 3
    s = PC.shapes(h, w)
    assert P.polygon_mask(s["around"], h, w).all() and not P.polygon_mask(s["beside"], h, w).any()
    assert not P.polygon_mask(s["in_a_pixel"], h, w).any()
    if h > 1 and w > 1:
        np.testing.assert_array_equal(P.polygon_mask(s["rect_int"], h, w), P.polygon_mask(s["rect_int_cw"], h, w))
        np.testing.assert_array_equal(P.polygon_mask(s["collinear_repeated"], h, w), P.polygon_mask(s["rect_int"], h, w))


def test_literal_and_parity_formulations_agree_on_random_polygons():
    h, w = PC.RANDOM_HW
    anns = PC.random_annotations()
    assert len(anns) == PC.RANDOM_N and _check_set(anns, h, w) > PC.RANDOM_N // 2


def test_the_long_edge_and_the_circle_exceed_one_block_stride():
    x, y, k = P._scaled(PC.long_edge(96, 80))
    assert max(max(abs(x[j + 1] - x[j]), abs(y[j + 1] - y[j])) + 1 for j in range(k)) > 1024
    x, y, k = P._scaled(PC.circle(96, 80))
    assert k == 1500 and any(x[j] == x[j + 1] and y[j] == y[j + 1] for j in range(k))
    disc = P.polygon_mask(PC.circle(96, 80), 96, 80)
    assert abs(int(disc.sum()) - np.pi * 28 * 28) < 60


def test_an_fma_sensitive_edge_is_in_the_set():
    edges = PC.fma_edges()
    assert len(edges) >= 1
    for dx, dy, t, ys in edges:
        s = -float(dy) / dx
        assert PC._v_separate(ys, s, t) != PC._v_fused(ys, s, t)
    polys = PC.fma_polygons()
    assert all([p] in PC.annotations(64, 64) for p in polys)


def test_rect_polygons_decode_to_the_rects_of_inst_cases():
    for box in ((10, 31, 10, 30), (0, 40, 0, 40), (5, 6, 5, 6), (50, 90, 40, 80), (0, 96, 0, 80)):
        np.testing.assert_array_equal(P.polygon_mask(PC.rect_poly(*box), IC.H, IC.W), IC.rect(*box))


def test_annotation_to_counts_takes_the_three_forms():
    h, w = 70, 45
    polys = PC.annotations(h, w)[-3]
    cnts = P.annotation_to_counts(polys, h, w)
    assert len(polys) == 3 and len(cnts) > 3
    np.testing.assert_array_equal(P.annotation_to_counts({"size": [h, w], "counts": [int(c) for c in cnts]}, h, w), cnts)
    np.testing.assert_array_equal(P.annotation_to_counts({"size": [h, w], "counts": R.counts_to_string(cnts)}, h, w), cnts)
    np.testing.assert_array_equal(P.annotation_to_counts({"size": [h, w], "counts": R.counts_to_string(cnts).encode()}, h, w), cnts)
    np.testing.assert_array_equal(P.annotation_to_counts([], h, w), [h * w])


@pytest.mark.parametrize("bad", [[1, 2, 3, 4, 5], [1, 2, 3, 4], [], [0, 0, 1, 1, 2, 2, 3], [0, 0, 1, float("nan"), 2, 2], [0, 0, 1e9, 1, 2, 2]])
def test_malformed_polygons_raise_on_the_host(bad):
    with pytest.raises(ValueError):
        P.annotation_to_counts([bad], 10, 10)
    with pytest.raises(ValueError):
        IE.gt_rows([{"category_id": 0, "segmentation": [bad]}], {0: 0}, polygons=True, hw=(10, 10))
    with pytest.raises(ValueError):
        P.pack_polygons([[bad]])


def test_gt_rows_packs_polygons_and_keeps_its_default():
    h, w = IC.H, IC.W
    crowd = IC.ann(IC.rect(0, 40, 0, 40), category=1, iscrowd=1)
    two = [PC.rect_poly(10, 30, 10, 20), PC.rect_poly(10, 30, 40, 50)]
    anns = [{"category_id": 7, "iscrowd": 0, "area": 400.0, "segmentation": [PC.rect_poly(10, 30, 10, 30)]}, crowd,
            {"category_id": 7, "segmentation": two},                            # no area: the pixels of the union, 400 (small)
            {"category_id": 1, "iscrowd": 0, "area": 5000.0, "segmentation": []}]
    rows, runs, offs, xy, poly_offs, gt_polys = IE.gt_rows(anns, {7: 0, 1: 1}, polygons=True, hw=(h, w))
    crowd_counts = IE.annotation_counts(crowd["segmentation"])
    np.testing.assert_array_equal(offs, [0, 0, len(crowd_counts), len(crowd_counts), len(crowd_counts)])
    np.testing.assert_array_equal(runs, crowd_counts)
    np.testing.assert_array_equal(gt_polys, [0, 1, 1, 3, 3])
    np.testing.assert_array_equal(poly_offs, [0, 4, 8, 12])
    np.testing.assert_array_equal(xy, np.concatenate([PC.rect_poly(10, 30, 10, 30)] + two).astype(np.float64))
    assert xy.dtype == np.float64 and poly_offs.dtype == np.int64 and gt_polys.dtype == np.int32 and runs.dtype == np.uint32
    np.testing.assert_array_equal(rows, [[0, 0, 0b1100], [1, 1, 0b1010], [0, 0, 0b1100], [1, 0, 0b1010]])
    with pytest.raises(ValueError, match="RLE"):
        IE.gt_rows(anns, {7: 0, 1: 1})
    with pytest.raises(ValueError, match="h, w"):
        IE.gt_rows(anns, {7: 0, 1: 1}, polygons=True)
    plain = IE.gt_rows([crowd], {1: 0})
    assert len(plain) == 3
    both = IE.gt_rows([crowd], {1: 0}, polygons=True, hw=(h, w))
    assert len(both) == 6 and both[3].size == 0 and list(both[4]) == [0] and list(both[5]) == [0, 0]
    for a, b in zip(plain, both):
        np.testing.assert_array_equal(a, b)
    assert IE.FLAG_BAD_POLYGON == 8 and IE.flag_names(8) == [IE.FLAG_NAMES[8]] and len(IE.flag_names(15)) == 4


def test_the_library_exports_the_polygon_entries():
    import __graft_entry__ as entry
    entry.build()
    lib = _lib.load()
    assert {"odise_hip_polygon_rle", "odise_hip_instance_eval_poly"} <= set(_lib.header_symbols())
    protos = _lib.header_prototypes()
    assert len(protos["odise_hip_polygon_rle"]) == 13 and len(protos["odise_hip_instance_eval_poly"]) == 3
    assert lib.odise_hip_sizeof_inst_poly_gt() == C.sizeof(_lib.InstPolyGt)
    assert lib.odise_hip_polygon_rle(None, None, None, None, 0, 0, 1, 1, None, 0, None, None, None) != 0      # a null context is an error
    assert lib.odise_hip_instance_eval_poly(None, None, None) != 0
