"""CPU: the host restatement of the segm evaluation (odise_amd/instance_eval.py) pinned by closed forms - run decoding, rleIou, the rules
of COCOeval.evaluateImg one by one, COCOeval.accumulate / summarize on cases whose AP can be worked out by hand."""
import math

import numpy as np
import pytest

import inst_cases as IC
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE


def _rows(c, image=0):
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"])
    assert flags == 0
    return rows, table


# ---- run decoding -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 130), (130, 1), (63, 5), (64, 5), (65, 5), (200, 300)])
def test_decode_runs_inverts_mask_counts(h, w):
    for k, m in enumerate(IC.mask_set(h, w)):
        cnts = R.mask_counts(m)
        np.testing.assert_array_equal(IE.decode_runs(cnts, h, w), m, err_msg=f"mask {k}")
        np.testing.assert_array_equal(IE.decode_runs(IC.with_zero_runs(cnts, k), h, w), m, err_msg=f"mask {k} with zero-length runs")


def test_zero_length_runs_in_the_middle_decode_as_written():
    # 2 zeros, 3 ones, NO zeros, 2 ones, 5 zeros over a 3 x 4 mask (column-major)
    m = IE.decode_runs([2, 3, 0, 2, 5], 3, 4)
    np.testing.assert_array_equal(m.ravel(order="F"), [0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
    # a leading zero-length run of zeros: the mask starts with a one
    np.testing.assert_array_equal(IE.decode_runs([0, 1, 11], 3, 4).ravel(order="F"), [1] + [0] * 11)


def test_annotation_counts_takes_compressed_and_uncompressed_rle():
    m = IC.blobs(40, 30, 1)
    a, b = IC.ann(m, compressed=True), IC.ann(m, compressed=False)
    assert isinstance(a["segmentation"]["counts"], str) and isinstance(b["segmentation"]["counts"], list)
    np.testing.assert_array_equal(IE.annotation_counts(a["segmentation"]), IE.annotation_counts(b["segmentation"]))
    a["segmentation"]["counts"] = a["segmentation"]["counts"].encode()
    np.testing.assert_array_equal(IE.decode_runs(IE.annotation_counts(a["segmentation"]), 40, 30), m)
    with pytest.raises(ValueError):
        IE.gt_rows([{"category_id": 0, "segmentation": [[0, 0, 1, 1, 2, 2]]}], {0: 0})


# ---- IoU ----------------------------------------------------------------------------------------------------------------------------------
def test_iou_closed_forms():
    ms = IC.mask_set(20, 17)[1:]                                            # without the empty mask
    iou = IE.mask_iou(ms, [R.mask_counts(m) for m in ms])
    np.testing.assert_array_equal(np.diag(iou), np.ones(len(ms)))          # identical masks
    assert iou[1, 2] == 0.0 and iou[2, 3] == 0.0                            # two corners: disjoint
    d = IC.rect(0, 2, 0, 2, 4, 4)                                           # hand-counted 4 x 4: 4 pixels against 6, 2 in common
    g = np.zeros((4, 4), np.uint8)
    g[1, 0:3] = 1
    g[2, 0:3] = 1
    assert IE.mask_iou(d[None], [R.mask_counts(g)])[0, 0] == 2 / 8
    assert IE.mask_iou(d[None], [R.mask_counts(g)], [1])[0, 0] == 2 / 4     # crowd: inter / area_d
    assert IE.mask_iou(np.zeros((1, 4, 4)), [R.mask_counts(g)], [1])[0, 0] == 0.0   # an empty detection divides nothing


# ---- matching -----------------------------------------------------------------------------------------------------------------------------
CASES = IC.matching_cases()


def test_higher_score_takes_the_ground_truth_where_its_iou_reaches():
    rows, _ = _rows(CASES["two_on_one"])
    assert list(rows["score"]) == [np.float32(.9), np.float32(.8)] and list(rows["area"]) == [272, 380]
    assert IC.bits(rows["matched"][0], 0) == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0]          # .6476
    assert IC.bits(rows["matched"][1], 0) == [0, 0, 0, 1, 1, 1, 1, 1, 1, 0]          # .9048, where the first left it
    assert IC.bits(rows["ignored"][0], 0) == [0] * 10 and IC.bits(rows["ignored"][1], 1) == [0] * 10
    # the ground truth (420 pixels) is ignored in the medium range: matches are ignored, the unmatched small detection too
    assert IC.bits(rows["ignored"][0], 2) == [1] * 10 and IC.bits(rows["ignored"][1], 2) == [1] * 10


def test_equal_iou_moves_to_the_later_ground_truth():
    rows, _ = _rows(CASES["equal_iou"])
    assert IC.bits(rows["matched"][0], 0) == [1] + [0] * 9                            # .5454
    assert IC.bits(rows["matched"][1], 0) == [0, 1, 1, 1, 1, 1, 1, 1, 1, 0]           # its ground truth is taken at t = .5


def test_crowd_match_is_ignored_and_the_crowd_stays_available():
    rows, _ = _rows(CASES["crowd"])
    for k in range(2):
        for a in range(4):
            assert IC.bits(rows["matched"][k], a) == [1] * 10 and IC.bits(rows["ignored"][k], a) == [1] * 10


def test_regular_match_is_not_displaced_by_an_ignored_one_of_higher_iou():
    rows, _ = _rows(CASES["break"])
    assert IC.bits(rows["matched"][0], 0) == [1] * 10
    assert IC.bits(rows["ignored"][0], 0) == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1]           # .7692 holds up to t = .75


def test_area_ranges():
    rows, table = _rows(CASES["areas"])
    assert table[0, 2] == 0b1100                                                      # 900: outside medium and large
    for a, ig in enumerate((0, 0, 1, 1)):
        assert IC.bits(rows["matched"][0], a) == [1] * 10 and IC.bits(rows["ignored"][0], a) == [ig] * 10
    for a, ig in enumerate((0, 1, 0, 1)):                                             # 1600 unmatched: false positive in all and medium
        assert IC.bits(rows["matched"][1], a) == [0] * 10 and IC.bits(rows["ignored"][1], a) == [ig] * 10
    np.testing.assert_array_equal(IE.npig(table, 1), [[1, 1, 0, 0]])


def test_a_picture_without_ground_truth_or_without_detections():
    c = IC.random_case(seed=9, n=25, n_gt=0)
    rows, _ = _rows(c)
    assert len(rows) == 25 and not rows["matched"].any()
    assert IC.bits(rows["ignored"][0], 0) == [0] * 10                                 # a false positive in the range "all"
    none = IC.case([np.zeros((IC.H, IC.W))], [0.], [0], CASES["areas"]["annotations"])
    none["masks"], none["scores"], none["classes"] = none["masks"][:0], none["scores"][:0], none["classes"][:0]
    assert len(_rows(none)[0]) == 0


def test_iou_exactly_on_the_threshold_matches():
    rows, _ = _rows(CASES["on_half"])
    assert IC.bits(rows["matched"][0], 0) == [1] + [0] * 9


def test_ties_keep_table_order_and_flags_empty_the_picture():
    c = IC.random_case()
    rows, _ = _rows(c)
    order = np.argsort(-c["scores"], kind="mergesort")
    np.testing.assert_array_equal(rows["score"], c["scores"][order])
    np.testing.assert_array_equal(rows["category"], c["classes"][order])
    assert len(np.unique(c["scores"])) < len(c["scores"])
    assert rows["matched"].any() and rows["ignored"].any() and (rows["matched"] & ~rows["ignored"]).any()
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    assert {int(v) for v in table[:, 2]} >= {0b1100, 0b1010, 0b0110} and table[:, 1].any()     # small, medium, large and crowds
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    bad = [np.r_[counts[0], 1]] + counts[1:]
    assert IE.image_rows(c["masks"], c["scores"], c["classes"], bad, table)[1] == IE.FLAG_BAD_RUNS
    assert IE.image_rows(c["masks"], c["scores"], c["classes"] + 3, counts, table, num_categories=c["K"])[1] == IE.FLAG_BAD_CLASS
    t2 = table.copy()
    t2[3, 1] = 2
    rows2, f2 = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, t2, num_categories=c["K"])
    assert f2 == IE.FLAG_BAD_GT and len(rows2) == 0


# ---- AP closed forms ----------------------------------------------------------------------------------------------------------------------
S = 128


def _picture(dets, gts, image, K):
    """dets: (mask, score, class), gts: (mask, class) -> rows, npig"""
    anns = [IC.ann(m, category=c) for m, c in gts]
    table, runs, offs = IE.gt_rows(anns, {k: k for k in range(K)})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    masks = np.stack([d[0] for d in dets]) if dets else np.zeros((0, S, S), np.uint8)
    rows, flags = IE.image_rows(masks, [d[1] for d in dets], [d[2] for d in dets], counts, table, image, num_categories=K)
    assert flags == 0
    return rows, IE.npig(table, K)


def _r(y0, y1, x0, x1):
    return IC.rect(y0, y1, x0, x1, S, S)


def test_perfect_predictions_score_100_everywhere():
    gts = [(_r(0, 10, 0, 10), 0), (_r(20, 60, 20, 60), 1), (_r(0, 100, 28, 128), 0)]         # 100 small, 1600 medium, 10000 large
    rows, n = _picture([(m, .9 - .1 * i, c) for i, (m, c) in enumerate(gts)], gts, 0, 2)
    p, r = IE.accumulate(rows, n, 2)
    # precision is tp / (fp + tp + np.spacing(1)): one ulp below 1 where it is perfect
    np.testing.assert_allclose(IE.summarize(p, r)[[0, 1, 2, 3, 4, 5, 8, 9, 10, 11]], np.ones(10), rtol=1e-12, atol=0)
    res = IE.results(p, r, ["a", "b"])
    assert sorted(res) == sorted(["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b"])
    for k, v in res.items():
        assert v == pytest.approx(100.0, abs=1e-9), k


def test_one_detection_of_iou_062():
    g = _r(0, 10, 0, 10)
    d = g.copy()
    d.ravel()[np.flatnonzero(d.ravel())[62:]] = 0                                            # 62 of its 100 pixels
    rows, n = _picture([(d, .9, 0)], [(g, 0)], 0, 1)
    res = IE.results(*IE.accumulate(rows, n, 1), ["a"])
    assert res["AP50"] == pytest.approx(100.0, abs=1e-9) and res["AP75"] == 0.0
    assert res["AP"] == pytest.approx(30.0, abs=1e-9) and res["APs"] == pytest.approx(30.0, abs=1e-9)
    assert math.isnan(res["APm"]) and math.isnan(res["APl"])


def test_false_positive_above_and_below_the_true_positive():
    g = _r(0, 10, 0, 10)
    for fp_score, want in ((.95, 50.0), (.5, 100.0)):
        rows, n = _picture([(g, .9, 0), (_r(50, 60, 50, 60), fp_score, 0)], [(g, 0)], 0, 1)
        res = IE.results(*IE.accumulate(rows, n, 1), ["a"])
        assert res["AP50"] == pytest.approx(want, abs=1e-9), (fp_score, res)


def test_missing_detections_score_zero_and_a_category_without_ground_truth_stays_out():
    g = _r(0, 10, 0, 10)
    rows, n = _picture([(g, .9, 0), (_r(50, 60, 50, 60), .8, 2)], [(g, 0), (_r(30, 40, 30, 40), 1)], 0, 3)
    p, r = IE.accumulate(rows, n, 3)
    res = IE.results(p, r, ["a", "b", "c"])
    assert res["AP-a"] == pytest.approx(100.0, abs=1e-9) and res["AP-b"] == 0.0 and math.isnan(res["AP-c"])
    assert (p[:, :, 2] == -1).all() and (r[:, 2] == -1).all()
    assert res["AP"] == pytest.approx(50.0, abs=1e-9)                                                                  # the mean of a and b only


def test_accumulate_does_not_depend_on_the_order_of_the_pictures():
    g = np.random.default_rng(0)
    pics = []
    for i in range(6):
        c = IC.random_case(seed=20 + i, n=30, n_gt=12, K=3)
        table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(3)})
        counts = [runs[offs[j]:offs[j + 1]] for j in range(len(table))]
        rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image=i, num_categories=3)
        assert flags == 0
        pics.append((rows, IE.npig(table, 3)))
    n = sum(p[1] for p in pics)
    want = IE.accumulate(np.concatenate([p[0] for p in pics]), n, 3)
    assert (want[0] > 0).any() and want[0].max() <= 1
    for _ in range(3):
        perm = g.permutation(6)
        got = IE.accumulate(np.concatenate([pics[i][0] for i in perm]), n, 3)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


# ---- struct size --------------------------------------------------------------------------------------------------------------------------
def test_row_and_descriptor_sizes_match_the_library():
    import ctypes as C

    import __graft_entry__ as entry
    from odise_amd import _lib
    entry.build()
    lib = _lib.load()
    assert IE.ROW_DTYPE.itemsize == 32 == lib.odise_hip_sizeof_inst_eval_row()
    assert lib.odise_hip_sizeof_inst_eval_desc() == C.sizeof(_lib.InstEvalDesc)
