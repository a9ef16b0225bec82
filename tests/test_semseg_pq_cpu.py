"""CPU: odise_amd/semseg_pq.py, the host specification of the PQ-for-semantic-segmentation metric: the rule on the four count vectors
against the literal restatement (integers equal, iou sums bit for bit), the crafted edges, the result table by hand, the front door's
grouping and painting, the ABI of the new calls, and HipSemSegEvaluator's default, which makes no new call."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import semseg_pq_cases as PC
from odise_amd import _lib, coco_rle
from odise_amd import panoptic_quality as PQ
from odise_amd import semseg_pq as SP


def counted(case, into=None):
    return SP.picture_stats(case.pred, case.gt(), case.K, into=into)


def row(stats, c):
    return (int(stats.tp[c]), int(stats.fp[c]), int(stats.fn[c]))


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_the_rule_on_the_counts_equals_the_literal_restatement(name):
    case = PC.CASES[name]
    want, flags = case.literal()
    got, got_flags = counted(case)
    assert flags == got_flags == 0
    assert np.array_equal(got.tp, want.tp) and np.array_equal(got.fp, want.fp) and np.array_equal(got.fn, want.fn)
    assert got.iou.tobytes() == want.iou.tobytes()
    counts = SP.image_counts(case.pred, case.gt(), case.K)
    assert counts.shape == (4, case.K) and int(counts[SP.AREA_PRED].sum()) == case.pred.size
    assert int(counts[SP.AREA_GT].sum()) == int((case.gt_raw != case.ignore_label).sum())
    assert (counts[SP.INTER] + counts[SP.VOID_PRED] <= counts[SP.AREA_PRED]).all() and (counts[SP.INTER] <= counts[SP.AREA_GT]).all()


def test_two_hundred_random_maps_equal_the_literal_restatement():
    shares, sizes, ks = [], set(), set()
    run_lit, run_cnt = {}, {}
    for seed in range(200):
        case = PC.random_case(seed)
        shares.append(float((case.gt_raw == case.ignore_label).mean()))
        sizes.add(case.hw)
        ks.add(case.K)
        want, _ = case.literal()
        got, flags = counted(case)
        assert flags == 0 and got == want, case.name                                 # PQStats.__eq__: counts equal, iou as bits
        # and as a stream: the pictures of one K accumulated in order into one PQStats
        SP.image_stats_literal(case.pred, case.gt_raw, case.K, case.ignore_label, into=run_lit.setdefault(case.K, PQ.PQStats(case.K)))
        counted(case, into=run_cnt.setdefault(case.K, PQ.PQStats(case.K)))
    assert all(run_cnt[K] == run_lit[K] for K in run_lit)
    assert min(shares) == 0.0 and max(shares) == 1.0 and 0.2 < np.median(shares) < 0.8   # from no VOID to nothing but VOID
    assert min(ks) == 1 and max(ks) == 300 and (1, 1) in sizes and (40, 60) in sizes


def test_crafted_edges():
    E = PC.EDGES
    s, _ = counted(E["iou_exactly_half"])
    assert row(s, 1) == (0, 1, 1) and s.iou[1] == 0.0                                 # 2 / 4 is not above one half: both sides lose
    assert row(s, 0) == (1, 0, 0) and s.iou[0] == 8 / 10
    s, _ = counted(E["iou_just_above_half"])
    assert row(s, 1) == (1, 0, 0) and s.iou[1] == 51 / 101
    s, _ = counted(E["void_share_exactly_half"])
    assert row(s, 2) == (0, 1, 0)                                                     # 1 / 2 is not above one half: counted
    s, _ = counted(E["void_share_above_half"])
    assert row(s, 2) == (0, 0, 0) and row(s, 0) == (1, 0, 0)                           # 2 / 3: skipped
    s, _ = counted(E["class_only_in_gt"])
    assert row(s, 1) == (0, 0, 1) and row(s, 0) == (1, 0, 0) and s.iou[0] == 5 / 8
    s, _ = counted(E["class_only_in_pred"])
    assert row(s, 2) == (0, 1, 0) and row(s, 0) == (1, 0, 0)
    s, _ = counted(E["void_leaves_the_union"])
    assert row(s, 0) == (1, 0, 0) and s.iou[0] == 3 / 4 and s.iou[1] == 2 / 3
    s, _ = counted(E["gt_all_void"])
    assert int(s.tp.sum() + s.fp.sum() + s.fn.sum()) == 0                             # every predicted class lies wholly on VOID
    s, _ = counted(E["one_pixel_right"])
    assert row(s, 0) == (1, 0, 0) and s.iou[0] == 1.0
    s, _ = counted(E["one_pixel_void"])
    assert row(s, 0) == (0, 0, 0)
    s, _ = counted(E["ignore255_K254"])
    assert row(s, 253) == (1, 0, 0) and s.iou[253] == 3 / 3 and row(s, 0) == (1, 0, 0) and s.iou[0] == 3 / 3 and row(s, 7) == (0, 0, 0)
    s, _ = counted(E["ignore65535_K300"])
    assert row(s, 255) == (1, 0, 0) and s.iou[255] == 3 / 3 and row(s, 299) == (1, 0, 0) and row(s, 7) == (0, 0, 0)
    # the device's ground truth: the ignore label is K, and anything outside [0, K] counts as K
    case = E["void_share_exactly_half"]
    g = case.gt()
    assert g.dtype == np.int32 and g[0, 0] == case.K
    for other in (-1, case.K + 7, 1 << 20):
        g2 = g.copy()
        g2[0, 0] = other
        assert SP.picture_stats(case.pred, g2, case.K)[0] == counted(case)[0]


def test_a_label_outside_the_classes_raises_the_flag_and_adds_nothing():
    case = PC.CASES["blobs_37x53_K150"]
    run = PQ.PQStats(150)
    counted(case, into=run)
    before = run.to_records().tobytes()
    for bad in (-1, 150):
        pred = case.pred.copy()
        pred[5, 5] = bad
        _, flags = SP.picture_stats(pred, case.gt(), 150, into=run)
        assert flags == SP.FLAG_BAD_LABEL and run.to_records().tobytes() == before
        _, flags = SP.image_stats_literal(pred, case.gt_raw, 150, 255, into=run)
        assert flags == SP.FLAG_BAD_LABEL and run.to_records().tobytes() == before
        counts = SP.image_counts(pred, case.gt(), 150)
        assert int(counts[SP.AREA_PRED].sum()) == pred.size - 1                       # counted in no row of the predicted side


def test_results_against_a_hand_computed_table():
    st = PQ.PQStats(4)
    st.iou[:], st.tp[:], st.fp[:], st.fn[:] = [1.5, 0.0, 0.6, 0.0], [2, 0, 1, 0], [1, 0, 0, 0], [1, 2, 1, 0]
    # class 0: pq 1.5 / 3, sq 0.75, rq 2 / 3; class 1: only misses: zeros; class 2: pq 0.6 / 1.5, sq 0.6, rq 1 / 1.5; class 3: no sample
    table = SP.results(st)
    assert table["All"] == table["Stuff"] == {"pq": (0.5 + 0.0 + 0.4) / 3, "sq": (0.75 + 0.0 + 0.6) / 3, "rq": (2 / 3 + 0.0 + 1 / 1.5) / 3, "n": 3}
    assert table["per_class"] == [{"pq": 0.5, "sq": 0.75, "rq": 2 / 3}, {"pq": 0.0, "sq": 0, "rq": 0.0}, {"pq": 0.6 / 1.5, "sq": 0.6, "rq": 1 / 1.5},
                                  {"pq": 0.0, "sq": 0.0, "rq": 0.0}]
    res = SP.evaluator_results(st, ["a", "b", "c", "d"])
    assert list(res) == ["PQ", "SQ", "RQ", "PQ-a", "PQ-b", "PQ-c", "PQ-d"]
    assert res["PQ"] == 100 * table["All"]["pq"] and res["SQ"] == 100 * table["All"]["sq"] and res["RQ"] == 100 * table["All"]["rq"]
    assert [res["PQ-a"], res["PQ-b"], res["PQ-c"], res["PQ-d"]] == [50.0, 0.0, 100 * (0.6 / 1.5), 0.0]
    text = SP.format_table(table).splitlines()
    assert text[0].split() == ["|", "PQ", "SQ", "RQ", "N"] and set(text[1]) == {"-"} and len(text) == 4
    assert text[2] == "All       |  30.0   45.0   44.4     3" and text[3] == text[2].replace("All  ", "Stuff")
    assert SP.results(PQ.PQStats(2))["All"] == {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}
    # the tool's mIoU: summed over the classes of the ground truth, divided by the classes of either side
    conf = np.array([[5, 2, 0, 3], [0, 0, 0, 0], [1, 0, 0, 9], [0, 0, 0, 0]], np.int64)   # class 2 is predicted, never in the ground truth
    assert SP.tool_miou(conf) == (5 / (6 + 7 - 5) + 0.0) / 3


def test_front_door_grouping_and_painting(tmp_path):
    cases = [PC.CASES["blobs_37x53_K150"], PC.EDGES["void_share_exactly_half"], PC.CASES["blobs_64x64_K150"]]
    names = ["ADE_val_1", "ADE_val_2", "x"]
    path, gt_dir, rows = PC.write_pictures(tmp_path, cases, names)
    groups = SP.group_rows(json.load(open(path)))
    assert list(groups) == names and sum(len(g) for g in groups.values()) == len(rows)
    for case, name in zip(cases, names):
        gt = SP.read_label_image(os.path.join(gt_dir, name + ".png"))
        assert np.array_equal(gt, case.gt_raw)
        assert np.array_equal(SP.paint(groups[name], gt.shape), case.pred)
    # the stem ends at the FIRST dot of the base name, and rows of one picture need not be adjacent
    mixed = [dict(rows[0], file_name="a/pic.0.jpg"), dict(rows[1], file_name="b/other.png"), dict(rows[2], file_name="pic.1.png")]
    assert {k: len(v) for k, v in SP.group_rows(mixed).items()} == {"pic": 2, "other": 1}
    # a later row paints over an earlier one; unpainted pixels stay class 0; a mapping translates dataset ids
    full, half = np.ones((2, 4), np.uint8), np.array([[1, 1, 0, 0]] * 2, np.uint8)
    painted = SP.paint([{"category_id": 30, "segmentation": coco_rle.encode(half)}], (2, 4))
    assert painted.tolist() == [[30, 30, 0, 0]] * 2
    two = [{"category_id": 30, "segmentation": coco_rle.encode(full)}, {"category_id": 50, "segmentation": coco_rle.encode(half)}]
    assert SP.paint(two, (2, 4)).tolist() == [[50, 50, 30, 30]] * 2 and SP.paint(two[::-1], (2, 4)).tolist() == [[30] * 4] * 2
    assert SP.paint(two, (2, 4), {30: 3, 50: 5}).tolist() == [[5, 5, 3, 3]] * 2


class StubLib:
    """Counts the calls of the library functions an evaluator makes; every call succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


class StubArray:
    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(shape)) * self.dtype.itemsize
        self.ptr = 4096

    def view(self, shape, dtype=None, offset_bytes=0):
        return StubArray(shape, dtype or self.dtype)


class StubContext:
    def __init__(self):
        self.lib, self.h, self.asked = StubLib(), None, []

    def empty(self, shape, dtype):
        return StubArray(shape, dtype)

    def semantic_eval_async(self, *args, **kw):
        self.asked.append(kw)
        return type("P", (), {"settle": lambda self: self})()


def test_the_evaluator_default_makes_no_new_call():
    from odise_amd.semseg_eval import HipSemSegEvaluator
    from odise_amd.runtime import DeviceArray
    for pq in (False, True):
        ctx = StubContext()
        ev = HipSemSegEvaluator(ctx, ["a", "b", "c"], 255, "d") if not pq else HipSemSegEvaluator(ctx, ["a", "b", "c"], 255, "d", pq=True)
        gt = DeviceArray.__new__(DeviceArray)
        ev.process(StubArray((4, 4), np.int32), gt, "f.png")
        assert ctx.lib.calls == ["odise_hip_memset"] * (2 if pq else 1)               # the accumulators; with pq one buffer more
        assert ("pq_stats" in ctx.asked[0]) == pq and hasattr(ev, "stats") == pq
        assert sorted(k for k in ctx.asked[0] if k != "pq_stats") == ["b_conf", "conf", "flags"]


def test_abi_of_the_new_calls():
    lib = _lib.load()
    assert lib.odise_hip_sizeof_semseg_pq_task() == C.sizeof(_lib.SemSegPqTask) == 8
    assert lib.odise_hip_semantic_pq(None, None, None, None, 1, 1, 1, None, None) == -1   # refused before anything is touched
    assert lib.odise_hip_semantic_eval_pq(None, None, None) == -1
    protos = _lib.header_prototypes()
    assert [t for t, _ in protos["odise_hip_semantic_pq"]][1:4] == ["const int32_t* labels", "const float* sem_seg", "const int32_t* gt"]
    assert len(protos["odise_hip_semantic_pq"]) == 9 and len(protos["odise_hip_semantic_eval_pq"]) == 3
