"""CPU: the host restatement of the bbox side of instance evaluation (odise_amd/instance_eval.py mask_boxes / box_iou / gt_boxes and
image_rows(iou_type="bbox")), against hand-worked values and detectron2's own formulation; instances_to_coco_json with boxes; the
ctypes mirrors of the two new descriptors.  Integers and exact doubles throughout: every comparison is ==."""
import ctypes as C
import os

import numpy as np
import pytest

import inst_bbox_cases as BC
import inst_cases as IC
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- mask_boxes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 130), (130, 1), (63, 5), (64, 5), (65, 5), (200, 300)])
def test_mask_boxes_equal_the_detectron2_formulation(h, w):
    ms = IC.mask_set(h, w)
    got = IE.mask_boxes(ms)
    assert got.dtype == np.float32 and got.shape == (len(ms), 4)
    np.testing.assert_array_equal(got, BC.torch_boxes(ms))
    np.testing.assert_array_equal(IE.mask_boxes(ms.astype(np.float32) * np.float32(0.75)), got)   # any nonzero value is a pixel
    # the set begins: zeros, ones, one pixel at (0, 0), (0, w-1), (h-1, 0), (h-1, w-1)
    want = [[0, 0, 0, 0], [0, 0, w, h], [0, 0, 1, 1], [w - 1, 0, w, 1], [0, h - 1, 1, h], [w - 1, h - 1, w, h]]
    np.testing.assert_array_equal(got[:6], np.asarray(want, np.float32))


def test_mask_boxes_by_hand():
    m = np.zeros((4, 70, 9), np.uint8)
    m[1, 63, 2] = 1
    m[2, 64, 8] = 1
    m[3, 0, 8] = m[3, 69, 0] = 1                                            # opposite corners: the whole picture
    np.testing.assert_array_equal(IE.mask_boxes(m), np.asarray([[0, 0, 0, 0], [2, 63, 3, 64], [8, 64, 9, 65], [0, 0, 9, 70]], np.float32))
    assert IE.mask_boxes(np.zeros((0, 5, 5), np.uint8)).shape == (0, 4)
    np.testing.assert_array_equal(IE.xyxy_to_xywh([[2, 63, 3, 64], [0, 0, 9, 70]]), [[2, 63, 1, 1], [0, 0, 9, 70]])


# ---- box_iou ------------------------------------------------------------------------------------------------------------------------------
def test_box_iou_by_hand():
    dt = [[0, 0, 10, 10], [20, 20, 4, 4], [2, 2, 4, 4], [10, 3, 8, 3]]
    gt = [[0, 0, 10, 10],                 # the first detection itself
          [10, 0, 5, 10],                 # touches the first detection's right edge: w == 0
          [100, 100, 1, 1],               # disjoint from everything
          [0, 0, 10, 10],                 # the same box as a crowd
          [10.5, 3.25, 7.75, 2.5]]        # fractional
    got = IE.box_iou(dt, gt, [0, 0, 0, 1, 0])
    want = np.zeros((4, 5))
    want[0, 0] = 1.0
    want[2, 0] = 16.0 / 100.0             # containment: 16 / (16 + 100 - 16)
    want[0, 3] = 1.0
    want[2, 3] = 1.0                      # crowd: inter / area_d = 16 / 16
    want[3, 1] = 15.0 / (24.0 + 50.0 - 15.0)   # x 10..15, y 3..6
    # fractional: x from max(10, 10.5) to min(18, 18.25) = 7.5, y from 3.25 to min(6, 5.75) = 2.5; 18.75 / (24 + 19.375 - 18.75)
    want[3, 4] = 18.75 / (24.0 + 19.375 - 18.75)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (got, want)
    assert IE.box_iou(np.zeros((0, 4)), gt).shape == (0, 5) and IE.box_iou(dt, np.zeros((0, 4))).shape == (4, 0)


def test_box_iou_is_one_rounded_operation_at_a_time():
    """Random fractional boxes against the expression written out in numpy doubles, every operation rounded on its own."""
    g = np.random.default_rng(12)
    dt = np.concatenate([g.random((4000, 2)) * 50, g.random((4000, 2)) * 40 + 0.1], 1)
    gt = dt + g.random((4000, 4)) * 3
    got = IE.box_iou(dt, gt[:1])[:, 0]
    for k in range(0, 4000, 97):
        D, G = dt[k], gt[0]
        w = min(np.float64(D[0]) + D[2], np.float64(G[0]) + G[2]) - max(D[0], G[0])
        h = min(np.float64(D[1]) + D[3], np.float64(G[1]) + G[3]) - max(D[1], G[1])
        want = 0.0 if w <= 0 or h <= 0 else (w * h) / ((D[2] * D[3] + G[2] * G[3]) - w * h)
        assert got[k] == want, k


def test_gt_boxes():
    anns = BC.with_bbox([IC.ann(IC.rect(3, 9, 4, 20)), IC.ann(IC.rect(0, 96, 0, 80))])
    np.testing.assert_array_equal(IE.gt_boxes(anns), [[4, 3, 16, 6], [0, 0, 80, 96]])
    assert IE.gt_boxes([]).shape == (0, 4) and IE.gt_boxes(anns).dtype == np.float64
    with pytest.raises(ValueError, match="bbox"):
        IE.gt_boxes([anns[0], IC.ann(IC.rect(1, 2, 1, 2))])


# ---- image_rows ---------------------------------------------------------------------------------------------------------------------------
def test_bbox_and_segm_matching_part_ways_on_the_ells():
    c = BC.ell_case()
    np.testing.assert_array_equal(IE.mask_boxes(c["masks"]), [[10, 10, 30, 30]] * 2)
    bbox, n, f, _, _ = BC.want_rows(c, 3, 2, "bbox")
    segm, _, f2, _, _ = BC.want_rows(c, 3, 2, "segm")
    assert n == 2 and f == 0 and f2 == 0
    assert [IC.bits(r["matched"], 0) for r in bbox] == [[1] * 10, [0] * 10]       # rank 0 (the upper L) takes the ground truth's box
    assert [IC.bits(r["matched"], 0) for r in segm] == [[0] * 10, [1] * 10]       # its mask is the lower L's
    assert list(bbox["area"]) == [400, 400] and list(segm["area"]) == [144, 144]
    assert list(bbox["score"]) == list(segm["score"]) and list(bbox["image"]) == [3, 3]


@pytest.mark.parametrize("name", sorted(IC.matching_cases()))
def test_bbox_rows_of_rectangles_are_the_segm_rows(name):
    """Every mask of the matching cases is a rectangle, so its box is itself: the pixel counts of rleIou and the products of bbIou are the same
    integers, and the crowd / ignore / tie rules must give the same rows in both tasks."""
    c = BC.bbox_case(IC.matching_cases()[name])
    bbox, n, f, _, _ = BC.want_rows(c, 5, len(c["masks"]), "bbox")
    segm = BC.want_rows(c, 5, len(c["masks"]), "segm")[0]
    assert f == 0 and n == len(c["masks"]) and bbox["matched"].any()
    assert bbox.tobytes() == segm.tobytes()


def test_bbox_rows_flag_a_box_that_is_not_finite():
    c = BC.bbox_case(IC.matching_cases()["areas"])
    c["annotations"][0]["bbox"][2] = float("nan")
    rows, n, f, _, _ = BC.want_rows(c, 0, 2, "bbox")
    assert f == IE.FLAG_BAD_GT and n == 0 and not rows.view(np.uint8).any()
    assert BC.want_rows(c, 0, 2, "segm")[2] == 0                            # the segm task does not look at the boxes


def test_default_image_rows_are_the_bytes_they_were():
    """tests/golden/inst_rows_random_case_segm.bin: image_rows of IC.random_case() (image 17) as the tree before the bbox task computed it."""
    c = IC.random_case()
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    rows, f = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, 17, num_categories=c["K"])
    with open(os.path.join(GOLDEN, "inst_rows_random_case_segm.bin"), "rb") as fh:
        want = fh.read()
    assert f == 0 and rows.tobytes() == want
    bbox, fb = IE.image_rows(c["masks"], c["scores"], c["classes"], None, table, 17, num_categories=c["K"], iou_type="bbox",
                             gt_boxes=IE.gt_boxes(BC.with_bbox(c["annotations"])))
    assert fb == 0 and bbox.tobytes() != want and (bbox["matched"] != 0).any()


# ---- instances_to_coco_json ---------------------------------------------------------------------------------------------------------------
def test_instances_to_coco_json_with_and_without_boxes():
    masks = np.stack([IC.rect(3, 9, 4, 20), IC.rect(0, 0, 0, 0)])
    inst = {"pred_masks": masks, "scores": np.asarray([.75, .5], np.float32), "pred_classes": np.asarray([4, 1])}
    plain = R.instances_to_coco_json(inst, 7)
    assert [r["bbox"] for r in plain] == [[0.0, 0.0, 0.0, 0.0]] * 2
    boxed = R.instances_to_coco_json(inst, 7, boxes=IE.mask_boxes(masks))
    assert [r["bbox"] for r in boxed] == [[4.0, 3.0, 16.0, 6.0], [0.0, 0.0, 0.0, 0.0]]
    assert all(type(v) is float for r in boxed for v in r["bbox"])
    for a, b in zip(plain, boxed):
        assert {k: v for k, v in a.items() if k != "bbox"} == {k: v for k, v in b.items() if k != "bbox"}
    assert boxed[0]["image_id"] == 7 and boxed[0]["category_id"] == 4 and boxed[0]["score"] == 0.75


# ---- the descriptors ----------------------------------------------------------------------------------------------------------------------
def test_descriptor_mirrors_match_the_library():
    import __graft_entry__ as entry
    from odise_amd import _lib
    entry.build()
    lib = _lib.load()
    assert lib.odise_hip_sizeof_inst_boxes_desc() == C.sizeof(_lib.InstBoxesDesc)
    assert lib.odise_hip_sizeof_inst_bbox_task() == C.sizeof(_lib.InstBboxTask)
    for name in ("odise_hip_instance_boxes", "odise_hip_box_iou", "odise_hip_instance_eval_bbox"):
        assert name in _lib.header_symbols() and hasattr(lib, name)
    # null context: refused before anything is touched
    assert lib.odise_hip_instance_boxes(None, None) != 0 and lib.odise_hip_box_iou(None, None, 1, None, 1, None, None) != 0
    assert lib.odise_hip_instance_eval_bbox(None, None, None, None) != 0
