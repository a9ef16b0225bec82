"""CPU: the host restatement of Boundary PQ (odise_amd/panoptic_quality.py segment_boundaries, image_boundary_stats, boundary_results) -
hand-drawn pictures against the literal repeated erosion and against numbers worked out by hand, the invariants that tie it to PQ, the
evaluator's record split, and the condition on the generated cases of tests/test_gpu_panoptic_boundary.py."""
import ctypes as C

import numpy as np
import pytest
from scipy.ndimage import binary_erosion

from odise_amd import _lib
from odise_amd import panoptic_quality as PQ
from pq_boundary_cases import boundary_case, dense_boundary_pairs, gpu_cases, must_fire, stream_cases
from pq_cases import Case, hand_cases


def literal_boundaries(pan, table, radius):
    """One mask per id, `radius` 3x3 erosions behind a ring of zeros, the mask minus its erosion."""
    pan = np.asarray(pan)
    out = np.zeros(pan.shape, np.uint8)
    for i in table:
        if i == 0:
            continue
        m = pan == i
        e = np.pad(m, radius)
        for _ in range(radius):
            e = binary_erosion(e, np.ones((3, 3), bool), border_value=0)
        out |= (m & ~e[radius:-radius, radius:-radius]).astype(np.uint8)
    return out


def drawn_pictures():
    line = np.zeros((9, 11), np.int64)
    line[4, 1:10] = 5                                   # a 1-pixel line: all of it is boundary
    edge = np.full((12, 12), 3, np.int64)
    edge[:8, :7] = 5                                    # touches the top and left edges: the pixels there are boundary pixels
    hole = np.full((15, 15), 5, np.int64)
    hole[4:11, 4:11] = 0
    hole[5:10, 5:10] = 7                                # a segment inside a hole of another, VOID between them
    yy, xx = np.mgrid[:8, :10]
    checker = np.where((yy + xx) % 2 == 0, 5, 7)        # every pixel is a boundary pixel
    absent = np.full((11, 13), 5, np.int64)
    absent[4:7, 5:9] = 99                               # 99 is in no table: a neighbour like any other, no boundary of its own
    return {"line": (line, [5]), "edge": (edge, [5, 3]), "hole": (hole, [5, 7]), "checker": (checker, [5, 7]), "absent": (absent, [5])}


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(drawn_pictures()))
def test_segment_boundaries_are_the_literal_erosion(name, radius):
    pan, table = drawn_pictures()[name]
    got = PQ.segment_boundaries(pan, table, radius)
    assert got.dtype == np.uint8 and np.array_equal(got, literal_boundaries(pan, table, radius))
    if name in ("line", "checker"):
        assert np.array_equal(got != 0, np.isin(pan, table))
    if name == "absent":
        assert not got[pan == 99].any() and got[3, 5] == 1 and got[0, 0] == 1 and got[2, 3] == (radius >= 2)
    if name == "edge" and radius == 1:
        assert got[0, 0] == 1 and got[0, 3] == 1 and got[3, 0] == 1 and got[3, 3] == 0 and got[7, 3] == 1 and got[11, 11] == 1 and got[9, 9] == 0


def test_segment_boundaries_first_row_counts_and_formula_radius():
    pan = np.full((40, 60), 5, np.int64)
    got = PQ.segment_boundaries(pan, [5, 0, 5])         # radius: round(0.02 * sqrt(40^2 + 60^2)) = 1
    assert got.sum() == 40 * 60 - 38 * 58
    assert np.array_equal(PQ.segment_boundaries(pan, [5], 20), np.ones((40, 60), np.uint8))     # 2r + 1 > min(H, W)


def pair_case(dx):
    """9 x 16: ground truth 5 = rows 1..7, columns 1..10 (7 x 10); prediction 9 = the same moved dx columns right; the rest is gt id 3
    (in the table, another category) and predicted id 8."""
    g = np.full((9, 16), 3, np.int64)
    p = np.full((9, 16), 8, np.int64)
    g[1:8, 1:11] = 5
    p[1:8, 1 + dx:11 + dx] = 9
    return Case(g, [(5, 1, 0, 70), (3, 2, 0, 9 * 16 - 70)], p, [(9, 1, 1), (8, 0, 2)], 3)


def test_hand_worked_pictures():
    # radius 1: B(5) = the ring of the 7 x 10 rectangle, 70 - 5 * 8 = 30 pixels, B(9) likewise.
    # dx = 1: inter 63, union 77, iou 9/11.  Rings: the rows 1 and 7 share columns 2..10 (9 + 9), the side columns do not meet, and each
    #   ring's side column crosses nothing of the other ring inside rows 2..6: inter_b 18, union_b 42, b_iou 3/7 -> demoted: fn, fp.
    #   The background pair (3, 8): inter 144 - 77 = 67, union 74 + 74 - 67 = 81; iou 67/81.  B(3) = the picture's outer ring (46) plus the
    #   ring around the rectangle (rows 0..8 x columns 0..11 minus the rectangle, minus the outer ring's share): counted by the literal
    #   erosion below rather than by hand; the category-1 numbers are the hand-made ones.
    for dx, (iou, b_iou) in {1: (63 / 77, 18 / 42), 0: (1.0, 1.0)}.items():
        case = pair_case(dx)
        tr = {}
        st, flags = PQ.image_boundary_stats(case.pan_gt, case.gt_rows, case.pan_pred, case.pred_rows, case.C, 1, trace=tr)
        assert flags == 0
        matched = min(iou, b_iou) > 0.5
        assert (st.tp[1], st.fp[1], st.fn[1]) == ((1, 0, 0) if matched else (0, 1, 1))
        assert st.iou[1] == (min(iou, b_iou) if matched else 0.0)
        ref, _ = case.stats()
        assert ref.tp[1] == 1 and ref.iou[1] == iou
    # a wide rectangle keeps its match at a lower value: 3 x 12 at radius 1 is all ring but 1 x 10; moved one column: inter 33, union 39;
    # rings 26 each; shared: rows 1 and 3 columns 2..12 (11 + 11), row 2: column 12 of B(5) meets no B(9) pixel (B(9) has 2 and 13) -> 22,
    # union_b 30, b_iou 11/15 < 11/13
    g = np.full((5, 16), 3, np.int64)
    p = np.full((5, 16), 8, np.int64)
    g[1:4, 1:13] = 5
    p[1:4, 2:14] = 9
    tr = {}
    st, _ = PQ.image_boundary_stats(g, [(5, 1, 0, 36), (3, 2, 0, 44)], p, [(9, 1, 1), (8, 0, 2)], 3, 1, trace=tr)
    assert (st.tp[1], st.fp[1], st.fn[1]) == (1, 0, 0) and st.iou[1] == 22 / 30 and tr["lowered"] >= 1
    # VOID below the predicted ring leaves union_b: ground truth 5 = columns 0..3 of one row, VOID right of it; prediction 9 = columns 0..5.
    # One row: every pixel is a boundary pixel.  inter_b 4, union_b 6 + 4 - 4 - 2 = 4 -> 1.0 = iou
    st, _ = PQ.image_boundary_stats([[5, 5, 5, 5, 0, 0]], [(5, 1, 0, 4)], [[9] * 6], [(9, 1, 1)], 3)
    assert (st.iou[1], st.tp[1]) == (1.0, 1)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_one_row_pictures_equal_pq(name):
    """2r + 1 > min(H, W): every pixel is a boundary pixel and the boundary counts are the mask counts; where the JSON area is the pixel
    count the records are byte-equal to image_stats, flags included."""
    case = hand_cases()[name]
    ref, ref_flags = case.stats()
    got, flags = PQ.image_boundary_stats(case.pan_gt, case.gt_rows, case.pan_pred, case.pred_rows, case.C)
    assert flags == ref_flags == case.flags
    if not name.startswith("json_area") and name != "two_matches_of_one_row":
        assert got.to_records().tobytes() == ref.to_records().tobytes()
    else:
        assert (got.tp <= ref.tp).all()      # |B(g)| is counted from the map: b_iou uses the pixel count where iou uses the JSON area


def test_degenerate_radius_on_a_blocky_picture_equals_pq_where_the_json_agrees():
    case = boundary_case(1, 67, 131, 37, 20)
    for i in range(len(case.gt_rows)):
        case.gt_rows[i, 3] = int((case.pan_gt == case.gt_rows[i, 0]).sum())
    ref, _ = case.stats()
    got, flags = PQ.image_boundary_stats(case.pan_gt, case.gt_rows, case.pan_pred, case.pred_rows, case.C, 34)     # 2r + 1 = 69 > H
    assert flags == 0 and ref.tp.sum() > 0 and got.to_records().tobytes() == ref.to_records().tobytes()


CASES = gpu_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_gpu_case_demotes_and_lowers_a_pair_and_keeps_the_invariants(name):
    case = CASES[name]
    if must_fire(case):
        tr = case.assert_boundary_rules_fire()
        assert tr["demoted"] >= 1 and tr["lowered"] >= 1
    else:   # only where the rule forbids such pairs: every pixel is a boundary pixel (1x1, 1x67), or a table without candidates
        assert 1 in case.pan_gt.shape or min(len(case.gt_rows), len(case.pred_rows)) == 0
        assert case.boundary_stats()[0].tp.sum() == case.stats()[0].tp.sum()
    ref, ref_flags = case.stats()
    got, flags = case.boundary_stats()
    assert flags == ref_flags == 0
    assert (got.tp <= ref.tp).all() and np.array_equal(got.tp + got.fn, ref.tp + ref.fn)
    # a second formulation of the matching (slot maps, sliding minima): the same pairs, and their sum in the same order
    pairs = dense_boundary_pairs(case)
    iou = np.zeros(case.C)
    for _, _, cat, v in pairs:
        iou[cat] += v
    assert np.array_equal(np.bincount([c for _, _, c, _ in pairs], minlength=case.C), got.tp) and iou.tobytes() == got.iou.tobytes()


def test_the_5x7_case_by_hand():
    """r = 1.  Left pair: inter 20, union 20 + 25 - 20 = 25; rings 14 and 16, 11 shared, union_b 19.  Right pair: inter 10, union 15; rings
    12 and 10, 7 shared, union_b 15."""
    case = CASES["size_5x7"]
    tr = {}
    got, _ = case.boundary_stats(tr)
    assert (tr["demoted"], tr["lowered"]) == (1, 1) and got.tp.sum() == 1 and got.iou.sum() == 11 / 19
    ref, _ = case.stats()
    assert ref.tp.sum() == 2 and sorted(ref.iou[ref.iou > 0].tolist()) in ([10 / 15, 20 / 25], [10 / 15 + 20 / 25])


def test_into_is_the_loop_and_not_the_sum_of_totals():
    cases = stream_cases()
    run = PQ.PQStats(6)
    for c in cases:
        c.boundary_stats(into=run)
    # the loop, written out from the second formulation: every matched pair of every picture, in ascending (gt id, pred id) order, onto
    # ONE running double per category
    loop = PQ.PQStats(6)
    for c in cases:
        for _, _, cat, v in dense_boundary_pairs(c):
            loop.tp[cat] += 1
            loop.iou[cat] += v
        one, _ = c.boundary_stats()
        loop.fp += one.fp
        loop.fn += one.fn
    assert np.array_equal(run.tp, loop.tp) and np.array_equal(run.fp, loop.fp) and np.array_equal(run.fn, loop.fn)
    assert run.iou.tobytes() == loop.iou.tobytes()
    totals = PQ.PQStats(6)
    for c in cases:
        totals += c.boundary_stats()[0]
    assert np.allclose(run.iou, totals.iou, rtol=1e-12) and run.iou.tobytes() != totals.iou.tobytes()
    again = PQ.PQStats(6)
    for c in cases:
        c.boundary_stats(into=again)
    assert again == run


def host_results() -> dict:
    """What `image_stats` and `image_boundary_stats` return for the one-row pictures of pq_cases.hand_cases (three flagged ones and the
    crowd rows among them), for every generated case above, and as running sums over the stream: the records as hex, flags, `trace`."""
    def entry(got, trace):
        return {"records": got[0].to_records().tobytes().hex(), "flags": int(got[1]), "trace": trace}
    out = {}
    for name, case in list(hand_cases().items()) + list(CASES.items()):
        tr, b_tr = {}, {}
        stats = case.stats(tr)
        radius = getattr(case, "radius", None)
        b_stats = PQ.image_boundary_stats(case.pan_gt, case.gt_rows, case.pan_pred, case.pred_rows, case.C, radius, trace=b_tr)
        out[name] = {"stats": entry(stats, tr), "boundary": entry(b_stats, b_tr)}
    run, b_run = PQ.PQStats(6), PQ.PQStats(6)
    for c in stream_cases():
        c.stats(into=run)
        c.boundary_stats(into=b_run)
    out["stream_into"] = {"stats": entry((run, 0), {}), "boundary": entry((b_run, 0), {})}
    return out


def test_both_functions_return_what_they_returned_before_they_shared_a_body():
    """tests/golden/pq_host_records.json holds `host_results()` of the two separate functions, written by json.dump of it at the commit
    before they became one body: the records byte for byte, the flags and the trace dicts (keys and values) are the same."""
    import json
    import pathlib
    golden = json.loads((pathlib.Path(__file__).parent / "golden" / "pq_host_records.json").read_text())
    got = host_results()
    assert sorted(got) == sorted(golden)
    assert any(golden[n]["stats"]["flags"] for n in golden) and golden["crowd"]["stats"]["trace"] == {"rejected": 0, "skipped_void": 0, "skipped_crowd": 1}
    for name in sorted(golden):
        for which in ("stats", "boundary"):
            assert got[name][which] == golden[name][which], (name, which)
        assert sorted(got[name]["boundary"]["trace"]) in ([], sorted(["rejected", "skipped_void", "skipped_crowd", "demoted", "lowered"]))
        assert sorted(got[name]["stats"]["trace"]) in ([], sorted(["rejected", "skipped_void", "skipped_crowd"]))


def test_boundary_results_by_hand():
    st = PQ.PQStats(3)
    st.iou[:], st.tp[:], st.fp[:], st.fn[:] = [1.5, 0.0, 0.6], [2, 0, 1], [1, 0, 0], [1, 2, 1]
    out = PQ.boundary_results(st, [True, True, False])
    # category 0: pq 1.5 / 3 = 0.5, sq 0.75, rq 2/3; category 1: 0, 0, 0; category 2: pq 0.6 / 1.5 = 0.4, sq 0.6, rq 2/3
    assert sorted(out) == sorted(["BPQ", "BSQ", "BRQ", "BPQ_th", "BSQ_th", "BRQ_th", "BPQ_st", "BSQ_st", "BRQ_st"])
    assert out["BPQ"] == 100 * (0.5 + 0.0 + 0.4) / 3 and out["BPQ_th"] == 100 * 0.25 and out["BPQ_st"] == 100 * 0.4
    assert out["BSQ_th"] == 100 * 0.375 and out["BRQ_st"] == 100 * (1 / 1.5)


class FakeArray:
    def __init__(self, host):
        self.host = host

    def view(self, shape, dtype, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return ("view", offset, n)

    def numpy(self):
        return self.host


def test_evaluator_record_split():
    """2C + 1 records: PQ, Boundary PQ, the flags; evaluate() sums the 2C as one PQStats and splits them again."""
    from odise_amd.panoptic_eval import HipPanopticEvaluator
    Cn = 3
    ev = HipPanopticEvaluator.__new__(HipPanopticEvaluator)
    ev.C, ev.isthing, ev.boundary, ev.n_records = Cn, [True, False, True], True, 2 * Cn
    host = np.zeros(2 * Cn + 1, PQ.STAT_DTYPE)
    host["iou"][:Cn], host["tp"][:Cn], host["fn"][:Cn] = [0.9, 0.0, 1.6], [1, 0, 2], [0, 1, 0]
    host["iou"][Cn:2 * Cn], host["tp"][Cn:2 * Cn], host["fn"][Cn:2 * Cn], host["fp"][Cn:2 * Cn] = [0.7, 0.0, 0.6], [1, 0, 1], [0, 1, 1], [0, 0, 1]
    ev._buf = FakeArray(host)
    out = ev.evaluate()
    assert ev.pq_stats == PQ.PQStats.from_records(host[:Cn]) and ev.boundary_stats == PQ.PQStats.from_records(host[Cn:2 * Cn])
    assert out == {**PQ.results(ev.pq_stats, ev.isthing), **PQ.boundary_results(ev.boundary_stats, ev.isthing)}
    assert out["PQ"] == 100 * ((0.9 + 0.0 + 1.6 / 2) / 3) and out["BPQ"] == 100 * ((0.7 + 0.0 + 0.6 / 2) / 3)
    host[2 * Cn:].view(np.int32)[0] = 2
    with pytest.raises(RuntimeError, match="bit 1"):
        ev.evaluate()
    ev.boundary, ev.n_records = False, Cn
    ev._buf = FakeArray(host[:Cn + 1].copy())
    ev._buf.host[Cn:].view(np.int32)[0] = 0
    assert ev.evaluate() == PQ.results(PQ.PQStats.from_records(host[:Cn]), ev.isthing)


def test_abi_of_the_new_calls():
    lib = _lib.load()
    assert lib.odise_hip_sizeof_pq_boundary_task() == C.sizeof(_lib.PqBoundaryTask) == 16
    assert lib.odise_hip_panoptic_quality_boundary(None, None, None) == -1        # refused before anything is touched
    assert lib.odise_hip_segment_boundaries(None, None, 1, 1, None, 0, 0, None, None) == -1
