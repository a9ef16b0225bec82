"""CPU: the LVIS specification (odise_amd/lvis_eval.py) against hand-worked pictures, each built to separate one clause of it."""
import numpy as np

from accum_cases import picture
from lvis_cases import ALL40, ann, bits, rect, rows_of, three_pictures, write_pair
from odise_amd import instance_eval as IE
from odise_amd import lvis_eval as LE

H, W = 40, 50
A = rect(H, W, 2, 12, 3, 13)        # 100 pixels
B = rect(H, W, 20, 30, 20, 40)      # 200 pixels, disjoint from A


def ap_of(rows, tables, K, freqs=None):
    npig = sum(LE.npig(t, K) for t in tables)
    p, r = LE.accumulate(np.concatenate(rows), npig, K)
    return LE.summarize(p, r, freqs or ["f"] * K), p, r


def test_a_detection_in_neither_list_vanishes_and_in_neg_it_is_a_false_positive():
    K = 2
    second, _, t1 = rows_of([(B, .5, 1)], [ann(B, 1)], K, image=1)            # category 1 has its object, found, in picture 1
    aps = []
    for score in (.9, .1):
        first, flags, t0 = rows_of([(A, .8, 0), (B, score, 1)], [ann(A, 0)], K)
        assert flags == 0 and len(first) == 1 and first["category"][0] == 0 and first["matched"][0] == ALL40
        aps.append(ap_of([first, second], [t0, t1], K)[0][0])
    assert aps[0] == aps[1] and np.isclose(aps[0], 1.0)                                        # 1 / (1 + 2^-52) in every cell
    first, flags, t0 = rows_of([(A, .8, 0), (B, .9, 1)], [ann(A, 0)], K, neg=[1])
    assert len(first) == 2 and first["category"].tolist() == [1, 0] and first["matched"][0] == 0
    assert bits(first["ignored"][0], 0) == 0 and bits(first["ignored"][0], 1) == 0            # 200 pixels: inside `all` and `small`
    s, p, _ = ap_of([first, second], [t0, t1], K)
    assert (p[:, :, 1, 0] == 1 / (2 + np.spacing(1))).all() and np.isclose(s[0], .75)         # the false positive ranks above the true one


def test_not_exhaustive_ignores_the_unmatched_detection_only():
    K = 1
    plain, _, _ = rows_of([(A, .9, 0), (B, .8, 0)], [ann(A, 0)], K)
    rows, flags, _ = rows_of([(A, .9, 0), (B, .8, 0)], [ann(A, 0)], K, nex=[0])
    assert flags == 0 and rows["matched"].tolist() == [ALL40, 0]
    assert rows["ignored"][1] == ALL40 and rows["ignored"][0] == plain["ignored"][0]
    assert bits(rows["ignored"][0], 0) == 0                                                    # the matched one is a true positive
    assert bits(plain["ignored"][1], 0) == 0 and bits(plain["ignored"][1], 3) == 0x3FF         # without the list: its area alone


def test_an_ignore_ground_truth_is_matched_once_at_its_plain_iou():
    K = 1
    g = ann(A, 0, ignore=1)
    rows, flags, table = rows_of([(A, .9, 0), (A, .8, 0)], [g], K)
    assert flags == 0 and table[0, 2] == LE.IGNORE_BITS and table[0, 1] == 0 and (LE.npig(table, K) == 0).all()
    assert rows["matched"].tolist() == [ALL40, 0] and rows["ignored"][0] == ALL40
    assert bits(rows["ignored"][1], 0) == 0 and bits(rows["ignored"][1], 1) == 0               # the second falls through: unmatched, by its area
    half = rect(H, W, 2, 12, 3, 8)                                                             # IoU 0.5 with A: plain IoU, not inter / area_d
    rows, _, _ = rows_of([(half, .9, 0)], [g], K)
    assert bits(rows["matched"][0], 0) == 0b1
    crowd, flags, _ = rows_of([(A, .9, 0)], [ann(A, 0, iscrowd=1)], K)
    assert flags == IE.FLAG_BAD_GT and len(crowd) == 0                                         # LVIS has no crowds


def test_the_cut_at_300_and_ties_in_table_order():
    K, n = 1, 303
    scores = np.linspace(1, .5, n).astype(np.float32)
    scores[299:302] = scores[299]                                                              # three tied at the cut: table index 299 stays
    dets = [(rect(20, 20, i // 20, i // 20 + 1, i % 20, i % 20 + (2 if i >= 300 else 1)), float(scores[i]), 0) for i in range(n)]
    assert LE.limit_dets(scores).tolist() == list(range(300))
    rows, flags, _ = rows_of(dets, [], K, neg=[0])
    assert flags == 0 and len(rows) == LE.MAX_DETS == 300 and (rows["area"] == 1).all() and (np.diff(rows["score"]) <= 0).all()
    back, _, _ = rows_of(dets[::-1], [], K, neg=[0])                                           # the other table order: of the tied three, 301 stays
    assert len(back) == 300 and back["area"][-2:].tolist() == [1, 2] and back["area"].sum() == 301


def test_the_area_range_ends_are_1024_and_9216():
    K, h, w = 1, 100, 100
    def sq(side, extra):
        m = rect(h, w, 0, side, 0, side)
        m[99, 99] = extra
        return m
    dets = [(sq(32, 0), .9, 0), (sq(32, 1), .8, 0), (sq(96, 0), .7, 0), (sq(96, 1), .6, 0)]
    rows, _, _ = rows_of(dets, [], K, neg=[0])
    assert rows["area"].tolist() == [1024, 1025, 9216, 9217] and (rows["matched"] == 0).all()
    out = [[bits(r["ignored"], a) == 0x3FF for a in range(4)] for r in rows]
    assert out == [[False, False, False, True], [False, True, False, True], [False, True, False, False], [False, True, True, False]]
    g = LE.gt_rows([ann(A, 0, area=1024.0), ann(A, 0, area=1024.5), ann(A, 0, area=9216.0), ann(A, 0, area=9216.5)], {0: 0})[0]
    assert g[:, 2].tolist() == [0b1000, 0b1010, 0b0010, 0b0110]


def test_on_equal_ious_the_later_ground_truth_wins():
    K = 1
    d1, g0, g1 = rect(H, W, 0, 10, 0, 4), rect(H, W, 0, 10, 0, 2), rect(H, W, 0, 10, 2, 4)     # IoU 0.5 with both
    rows, _, table = rows_of([(d1, .9, 0), (g1, .8, 0)], [ann(g0, 0), ann(g1, 0)], K)
    assert bits(rows["matched"][0], 0) == 0b1                                                  # d1 reaches t = 0.5 only
    assert bits(rows["matched"][1], 0) == 0x3FE                                                # there g1 is taken, by d1: the later one won
    lit = IE._walk(2, np.float32([.9, .8]), np.int64([0, 0]), table.astype(np.int64), IE.mask_iou(np.stack([d1, g1]), [
        IE.annotation_counts(ann(g0, 0)["segmentation"]), IE.annotation_counts(ann(g1, 0)["segmentation"])]), np.int64([40, 20]), None, 0, IE.IOU_THRS)
    assert lit.tobytes() == rows.tobytes()                                                     # the walk of instance_eval with no crowd


def test_accumulate_edges():
    K = 4
    g = np.random.default_rng(5)
    rows = picture(g, 0, g.integers(0, 2, 40))                                                 # categories 0 and 1 have rows
    npig = np.array([[5, 5, 0, 5], [3, 3, 3, 3], [2, 2, 2, 2], [0, 0, 0, 0]], np.int64)
    p, r = LE.accumulate(rows, npig, K)
    assert p.shape == (10, 101, K, 4) and r.shape == (10, K, 4)
    assert (p[:, :, 2] == 0).all() and (r[:, 2] == 0).all()                                    # ground truth and no detections
    assert (p[:, :, 0, 2] == -1).all() and (r[:, 0, 2] == -1).all() and (p[:, :, 3] == -1).all() and (p[:, :, 0, 0] > -1).all()
    s = LE.summarize(p, r, ["f", "f", "c", "c"])
    assert s[6] == -1 and s[7] == 0 and s[8] > 0                                               # no rare category; the common ones score 0
    assert LE.results(p, r, ["f", "f", "c", "c"])["APr"] == -100 and list(LE.results(p, r, ["f"] * 4)) == list(LE.STAT_NAMES[:9])
    assert LE.summarize(-np.ones_like(p), -np.ones_like(r), ["r"] * 4).tolist() == [-1] * 13


def test_accumulate_against_a_literal_second_implementation():
    g = np.random.default_rng(9)
    rows = np.concatenate([picture(g, i, np.zeros(57, np.int64)) for i in (2, 0, 1)])          # one category, ties across pictures
    n_pos = 61
    p, r = LE.accumulate(rows, [[n_pos] * 4], 1)
    srt = rows[np.argsort(rows["image"], kind="stable")]
    srt = srt[np.argsort(-srt["score"], kind="mergesort")]
    for a in range(4):
        for t in range(10):
            m, ig = (srt["matched"] >> np.uint64(10 * a + t)) & np.uint64(1), (srt["ignored"] >> np.uint64(10 * a + t)) & np.uint64(1)
            tp = fp = 0
            rc, pr = [], []
            for mm, ii in zip(m.tolist(), ig.tolist()):
                tp += int(mm and not ii)
                fp += int(not mm and not ii)
                rc.append(tp / n_pos)
                pr.append(tp / (fp + tp + np.spacing(1)))
            for ri, thr in enumerate(IE.REC_THRS):
                i = int(np.searchsorted(rc, thr, side="left"))
                assert p[t, ri, 0, a] == (max(pr[i:]) if i < len(pr) else 0.0)
            assert r[t, 0, a] == rc[-1]
    assert 0 < LE.summarize(p, r, ["c"])[0] < 1


def test_the_front_door_on_three_pictures(tmp_path, capsys):
    rp, gp = write_pair(tmp_path)
    out = LE.evaluate_files(rp, gp, "cpu")
    s = out["stats"]
    ap10, ap20, ap30 = 51 / 101, 1.0, .5           # one of two objects found; found; a false positive of another picture ranks above it
    assert np.isclose(s[0], (ap10 + ap20 + ap30) / 3) and np.isclose(s[6], ap30) and np.isclose(s[7], ap20) and np.isclose(s[8], ap10)
    assert np.isclose(s[9], (.5 + 1 + 1) / 3) and out["flags"] == 0
    assert out["results"] == {k: float(v * 100) for k, v in zip(LE.STAT_NAMES[:9], s[:9])}
    gt, res = three_pictures()
    assert any(r["category_id"] == 20 and r["image_id"] == 1 for r in res) and 20 not in gt["images"][0]["neg_category_ids"]
    assert LE.main(["--results", rp, "--gt", gp, "--device", "cpu"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split()[0] for ln in lines] == list(LE.STAT_NAMES) and float(lines[0].split()[1]) == round(float(s[0]), 6)
