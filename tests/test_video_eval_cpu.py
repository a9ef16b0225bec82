"""CPU: the numpy specification of video instance segmentation AP (odise_amd/video_eval.py) on hand-worked videos.  Every expected value
below is written out by hand from the rule (ytvoseval.py: sequence IoU, mean areas with the ranges [0, 1e10], [0, 128^2], [128^2, 256^2],
[256^2, 1e10], and evaluateImg's walk); none is computed by the code under test."""
import os
import subprocess
import sys

import numpy as np
import pytest

from odise_amd import instance_eval as IE
from odise_amd import video_eval as VE
from video_cases import STAT_NAMES, box, write_pair

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(ranges, thresholds):
    return sum(1 << (10 * a + t) for a in ranges for t in thresholds)


def table(*rows):
    return np.asarray(rows, np.int32).reshape(-1, 3)


def test_ranges_are_the_videos():
    assert VE.VIDEO_AREA_RNG == ((0, 1e10), (0, 16384), (16384, 65536), (65536, 1e10))
    assert VE.FLAG_SHARED_SLOT == 16 and set(VE.FLAG_NAMES) == {1, 2, 4, 8, 16}


def test_a_absent_ground_truth_frame_grows_the_union():
    # frame 0: d = 4x4 at (0,0), g = 4x4 at (2,2): they share 2x2 = 4.  frame 1: d = 3x3, g absent: the union grows by 9.
    d = [box(8, 8, 0, 4, 0, 4), box(8, 8, 0, 3, 0, 3)]
    g = [box(8, 8, 2, 6, 2, 6), None]
    c = VE.sequence_counts([d], [g])
    assert (int(c.inter[0, 0]), int(c.area_d[0]), int(c.area_g[0]), int(c.frames_d[0])) == (4, 25, 16, 2)
    iou = VE.sequence_iou([d], [g])
    assert iou.shape == (1, 1) and iou[0, 0] == 4 / 37            # (16 + 16 - 4) + 9
    assert c.avg_area()[0] == 12.5
    rows, flags = VE.video_rows([d], [.9], [0], [g], table((0, 0, 0)), video=7)
    assert flags == 0 and len(rows) == 1
    assert (rows["area"][0], rows["image"][0], rows["category"][0]) == (12, 7, 0)          # the mean, truncated
    assert rows["matched"][0] == 0 and rows["ignored"][0] == bits((2, 3), range(10))     # 4 / 37 < .5; 12.5 lies in [0, 128^2] only


def test_b_a_track_without_a_mask():
    d = [None, None, None]
    g = [box(8, 8, 0, 4, 0, 4)] * 3
    assert VE.sequence_iou([d], [g])[0, 0] == 0.0
    assert VE.avg_area([None, None, None]) == 0.0 and VE.avg_area([0, None]) == 0.0
    c = VE.sequence_counts([d], [g])
    assert c.avg_area()[0] == 0.0 and int(c.frames_d[0]) == 0 and int(c.area_g[0]) == 48
    rows, flags = VE.video_rows([d], [.5], [0], [g], table((0, 0, 0)))
    assert flags == 0 and rows["area"][0] == 0 and rows["matched"][0] == 0
    assert rows["ignored"][0] == bits((2, 3), range(10))           # area 0 lies inside [0, 1e10] and [0, 128^2], outside the other two
    # neither side has a mask anywhere: the denominator is 0 and the IoU is 0
    assert VE.sequence_iou([d], [[None, None, None]])[0, 0] == 0.0


def test_c_a_crowd_keeps_the_plain_iou_and_is_matched_twice():
    # one frame; the crowd covers columns 0..3 (32 pixels), both detections 7 of its 8 rows (28): iou = 28 / 32 = 0.875 for both,
    # where inter / area_d, the still-picture rule for a crowd, would give 1.0
    g = [[box(8, 8, 0, 8, 0, 4)]]
    d = [[box(8, 8, 0, 7, 0, 4)], [box(8, 8, 1, 8, 0, 4)]]
    iou = VE.sequence_iou(d, g)
    assert iou[0, 0] == 0.875 and iou[1, 0] == 0.875
    rows, flags = VE.video_rows(d, [.9, .8], [0, 0], g, table((0, 1, 0)))
    assert flags == 0
    for k in range(2):   # thresholds .5 .. .85 match the crowd (an ignored ground truth) in every range, both detections; .9 and .95 do not
        assert rows["matched"][k] == bits(range(4), range(8))
        assert rows["ignored"][k] == bits(range(4), range(8)) | bits((2, 3), (8, 9))     # unmatched there: area 28 outside ranges 2, 3


def test_d_the_ends_of_the_ranges_are_included():
    full128, full256 = np.ones((128, 128), bool), np.ones((256, 256), bool)
    for mask, inside_out in ((full128, (3,)), (full256, (1,))):     # 128^2 lies in ranges 0, 1, 2; 256^2 in ranges 0, 2, 3
        rows, flags = VE.video_rows([[mask]], [.5], [0], [], np.zeros((0, 3), np.int32))
        assert flags == 0 and rows["matched"][0] == 0 and rows["ignored"][0] == bits(inside_out, range(10))
        assert rows["area"][0] == mask.size
    # a mean that lands on the end exactly: 16386 and 16382 pixels
    b = full128.copy()
    b[0, :2] = False                                                 # 128 * 128 - 2
    big = np.ones((129, 128), bool)
    big[128, 2:] = False                                             # 128 * 128 + 2
    c = VE.sequence_counts([[big, np.pad(b, ((0, 1), (0, 0)))]], [])
    assert (int(c.area_d[0]), int(c.frames_d[0]), c.avg_area()[0]) == (32768, 2, 16384.0)
    assert [VE.area_outside(16384.0, r) for r in range(4)] == [False, False, False, True]
    assert [VE.area_outside(65536.0, r) for r in range(4)] == [False, True, False, False]
    # the ground truth's side: the annotation's own areas, floats from the file
    t = VE.gt_track_rows([{"category_id": 5, "iscrowd": 0, "areas": [16384.5, None, 16383.5]},
                          {"category_id": 5, "iscrowd": 1, "areas": [65536.0, 0, None]},
                          {"category_id": 5, "areas": [None]}], {5: 0})
    assert t.tolist() == [[0, 0, 8], [0, 1, 2], [0, 0, 4 | 8]]


def test_e_equal_iou_the_later_ground_truth_wins():
    # columns: g0 = 0..3, g1 = 2..5; d0 = 1..4 has 3 of 5 with both (0.6); d1 = 3..6 has 0.6 with g1 and 1 / 7 with g0.
    # d0 (higher score) moves on to g1 on the equal value, so nothing is left for d1; had d0 kept g0, d1 would match g1.
    col = lambda x0, x1: [box(8, 8, 0, 8, x0, x1)]
    d, g = [col(1, 5), col(3, 7)], [col(0, 4), col(2, 6)]
    iou = VE.sequence_iou(d, g)
    assert iou[0, 0] == iou[0, 1] == 24 / 40 and iou[1, 1] == 24 / 40 and iou[1, 0] == 8 / 56
    rows, flags = VE.video_rows(d, [.9, .8], [0, 0], g, table((0, 0, 0), (0, 0, 0)))
    assert flags == 0
    assert rows["matched"][0] & bits((0,), range(10)) in (bits((0,), (0, 1)), bits((0,), (0, 1, 2)))   # .5 and .55 for certain; .6 is the tie
    assert rows["matched"][1] == 0


def test_f_score_ties_keep_table_order():
    g = [[box(8, 8, 0, 8, 0, 4)]]
    exact, short = [box(8, 8, 0, 8, 0, 4)], [box(8, 8, 0, 7, 0, 4)]              # IoU 1 and 0.875, areas 32 and 28
    rows, _ = VE.video_rows([exact, short], [.7, .7], [0, 0], g, table((0, 0, 0)))
    assert rows["area"].tolist() == [32, 28]
    assert rows["matched"][0] == bits(range(4), range(10)) and rows["matched"][1] == 0
    rows, _ = VE.video_rows([short, exact], [.7, .7], [0, 0], g, table((0, 0, 0)))
    assert rows["area"].tolist() == [28, 32]
    assert rows["matched"][0] == bits(range(4), range(8))                        # the first in the table walks first and takes it up to .85
    assert rows["matched"][1] == bits(range(4), (8, 9))


def test_g_sequence_iou_against_a_literal_pixel_loop():
    rng = np.random.default_rng(20240607)
    T, h, w = 4, 9, 7

    def track():
        return [None if rng.random() < .3 else rng.random((h, w)) < .4 for _ in range(T)]
    dts, gts = [track() for _ in range(5)], [track() for _ in range(4)]
    got = VE.sequence_iou(dts, gts)
    for i, d in enumerate(dts):
        for j, g in enumerate(gts):
            inter = union = 0
            for f in range(T):
                for y in range(h):
                    for x in range(w):
                        a = d[f] is not None and bool(d[f][y, x])
                        b = g[f] is not None and bool(g[f][y, x])
                        inter += a and b
                        union += a or b
            assert got[i, j] == (inter / union if union else 0.0), (i, j)
    for i, d in enumerate(dts):
        areas = [None if m is None else int(m.sum()) for m in d]
        assert VE.sequence_counts(dts, gts).avg_area()[i] == VE.avg_area(areas)


def test_flags_and_shared_slots():
    c = VE.Counts(3, 2)
    m = np.stack([box(8, 8, 0, 4, 0, 4), box(8, 8, 2, 6, 2, 6), box(8, 8, 0, 8, 0, 8)])
    assert c.add_frame(m, [1, 1, 9], m[:1], [0]) == 16                           # two detections on track 1; slot 9 is no track
    assert c.area_d.tolist() == [0, 32, 0] and c.frames_d.tolist() == [0, 2, 0] and c.inter[1, 0] == 16 + 4 and c.area_g.tolist() == [16, 0]
    assert c.add_frame(m[:1], [0], m[:2], [1, 1]) == 16 and c.add_frame(m[:2], [0, 2], m[:2], [0, 1]) == 0
    rows, flags = VE.video_rows([[m[0]]], [.5], [3], [], np.zeros((0, 3), np.int32), num_categories=3)
    assert flags == 2 and len(rows) == 0
    rows, flags = VE.video_rows([[m[0]]], [.5], [0], [[m[0]]], table((0, 2, 0)), num_categories=3)
    assert flags == 4 and len(rows) == 0


# ---- the front door -------------------------------------------------------------------------------------------------------------------------
def _numbers(text):
    lines = [l.split() for l in text.strip().splitlines()]
    assert [l[0] for l in lines] == STAT_NAMES
    return [float(l[1]) for l in lines]


def test_h_cli_perfect_result(tmp_path):
    rp, gp = write_pair(tmp_path, True)
    r = subprocess.run([sys.executable, "-m", "odise_amd.video_eval", "--results", rp, "--gt", gp, "--device", "cpu"], cwd=REPO, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    s = _numbers(r.stdout)
    assert len(s) == 12
    assert s[0] == 1.0 and s[1] == 1.0 and s[2] == 1.0 and s[3] == 1.0           # every track is small: APs = AP
    assert s[4] == -1.0 and s[5] == -1.0                                          # no medium or large ground truth
    assert s[6] == 1.0 and s[8] == 1.0 and s[9] == 1.0 and s[10] == -1.0
    out = VE.evaluate_files(rp, gp, "cpu")
    # 1 / (1 + 2^-52) is one ulp below 1: COCO's own precision of a perfect result
    assert all(abs(out["results"][k] - 100.0) < 1e-9 for k in ("AP", "AP-cat", "AP-dog"))


def test_h_cli_empty_result(tmp_path, capsys):
    rp, gp = write_pair(tmp_path, False)
    assert VE.main(["--results", rp, "--gt", gp, "--device", "cpu"]) == 0
    s = _numbers(capsys.readouterr().out)
    assert s[0] == 0.0 and s[3] == 0.0 and s[8] == 0.0                            # ground truth without a detection: COCO's 0
    assert s[4] == -1.0 and s[5] == -1.0                                          # no ground truth in the range: COCO's -1


def test_more_than_100_tracks_are_walked_by_category():
    tracks = [{"category_id": 1 + (k % 3), "score": 1.0 - k / 1000, "segmentations": [None]} for k in range(330)]
    chunks = VE._chunks(tracks, {1: 0, 2: 1, 3: 2})
    assert [len(c) for c in chunks] == [100, 100, 100] and all(len({t["category_id"] for t in c}) == 1 for c in chunks)
    assert chunks[0][0] is tracks[0] and chunks[0][-1] is tracks[297]             # the 100 best of 110, in file order
    assert VE._chunks([], {}) == [[]]


def test_pack_segmentations_is_the_mask_part_of_gt_rows():
    from odise_amd import coco_rle
    m = box(12, 10, 2, 9, 1, 7)
    segs = [coco_rle.encode(m), {"size": [12, 10], "counts": coco_rle.mask_counts(m).tolist()}, [[1.0, 1.0, 8.5, 1.0, 8.5, 9.0], [0, 0, 3, 0, 3, 3, 0, 3]]]
    want = IE.gt_rows([{"category_id": 0, "area": 1.0, "segmentation": s} for s in segs], {0: 0}, polygons=True, hw=(12, 10))[1:]
    got = VE.pack_segmentations(segs, (12, 10))
    assert len(got) == 5 and all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert [a.size for a in VE.pack_segmentations([], (12, 10))] == [0, 1, 0, 1, 1]
    with pytest.raises(ValueError):
        VE.pack_segmentations([[[0, 0, 1, 1]]], (12, 10))


def test_a_crowded_video_is_walked_in_parts(tmp_path):
    rp, gp = write_pair(tmp_path, True, crowded=True)
    out = VE.evaluate_files(rp, gp, "cpu")
    s = out["stats"]
    assert len(s) == 12 and 0 < s[0] < 1 and s[8] < 1 and s[4] == -1          # video 30's track has no result: recall below 1
