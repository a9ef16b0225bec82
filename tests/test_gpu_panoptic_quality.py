"""GPU: odise_hip_panoptic_quality (csrc/pq.hip) against the host restatement odise_amd.panoptic_quality.image_stats.  Counts and flags
are exact and the iou sums bit-identical: the statistics are compared as their raw 32-byte records."""
import numpy as np
import pytest

from odise_amd import panoptic_quality as PQ
from odise_amd._lib import MAX_SEGMENTS
from pq_cases import Case, blocky_case, hand_cases

pytestmark = pytest.mark.gpu

HAND = hand_cases()


def upload(ctx, case, layout=0, unaligned=False):
    """-> (record, gt) on the device.  unaligned: the record starts one int32, the RGB bytes one byte past a 16-byte boundary (a row of
    an exchange buffer; the kernel then reads pixel by pixel)."""
    rec = case.record(MAX_SEGMENTS)
    gt = case.rgb() if layout == 0 else case.pan_gt
    if not unaligned:
        return ctx.to_device(rec), ctx.to_device(gt)
    rbuf = ctx.to_device(np.concatenate([np.full(1, -7, np.int32), rec]))
    gbuf = ctx.to_device(np.concatenate([np.full(1, 255, gt.dtype), gt.reshape(-1)]))
    return rbuf.view(rec.shape, np.int32, 4), gbuf.view(gt.shape, gt.dtype, gt.dtype.itemsize)


def run(ctx, case, layout=0, stats=None, flags=None, unaligned=False):
    rec, gt = upload(ctx, case, layout, unaligned)
    return ctx.panoptic_quality_record(rec, case.pan_gt.shape, gt, case.gt_rows, case.C, stats, flags)


def check(stats, flags, ref, ref_flags=0):
    got = PQ.PQStats.from_records(stats.numpy())
    assert int(flags.numpy()[0]) == ref_flags
    assert np.array_equal(got.tp, ref.tp) and np.array_equal(got.fp, ref.fp) and np.array_equal(got.fn, ref.fn), (got, ref)
    assert got.iou.tobytes() == ref.iou.tobytes(), (got, ref)       # the raw 8 bytes
    assert stats.numpy().tobytes() == ref.to_records().tobytes()


# 1 pixel; H*W*3 no dword multiple (a 3-pixel tail behind 8 whole groups); odd sizes; several blocks and a ragged tail; many blocks flushing
# into one matrix.  Tables as large as the picture has room for.
SIZES = [(8, 1, 1, 1, 1), (7, 5, 7, 3, 2), (1, 67, 131, 37, 20), (12, 200, 333, 37, 20), (11, 512, 512, 37, 20)]


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("seed,h,w,n_gt,n", SIZES)
def test_sizes_and_ground_truth_layouts(ctx, seed, h, w, n_gt, n, layout):
    case = blocky_case(seed, h, w, n_gt, n)
    if min(h, w) >= 64:
        case.assert_every_rule_fires()
    ref, ref_flags = case.stats()
    assert ref_flags == 0
    check(*run(ctx, case, layout), ref)


# unsorted tables with ids 1 and 2^24 - 1.  (254, 100) is the case whose (n_gt + 2) x (n + 2) = 26112 cells exceed the LDS histogram
# (12288 cells): the pixel pass counts in the global matrix.  (254, 1) and (37, 100) fit.
@pytest.mark.parametrize("n", [0, 1, 100])
@pytest.mark.parametrize("n_gt", [0, 1, 37, 254])
def test_table_sizes(ctx, n_gt, n):
    seed = 100 + [0, 1, 37, 254].index(n_gt) * 3 + [0, 1, 100].index(n)
    case = blocky_case(seed, 200, 333, n_gt, n)
    assert len(case.gt_rows) == n_gt and len(case.pred_rows) == n
    if n_gt >= 2:
        assert {1, 2 ** 24 - 1} <= set(case.gt_rows[:, 0].tolist()) and list(case.gt_rows[:, 0]) != sorted(case.gt_rows[:, 0])
    if n >= 2:
        assert {1, 2 ** 24 - 1} <= set(case.pred_rows[:, 0].tolist()) and list(case.pred_rows[:, 0]) != sorted(case.pred_rows[:, 0])
    if n_gt >= 37 and n == 100:
        case.assert_every_rule_fires()
    ref, ref_flags = case.stats()
    assert ref_flags == 0
    check(*run(ctx, case), ref)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_record_that_is_not_16_byte_aligned(ctx, layout):
    case = blocky_case(1, 67, 131, 37, 20)
    rec, gt = upload(ctx, case, layout, unaligned=True)
    assert rec.ptr % 16 == 4 and gt.ptr % 16 == (1 if layout == 0 else 4)
    ref, _ = case.stats()
    check(*run(ctx, case, layout, unaligned=True), ref)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_pictures_on_the_device(ctx, name):
    """Among them: iou exactly 0.5, a crowd ratio of exactly 0.5, the last crowd row of a category, JSON areas that disagree with the map,
    a ground-truth row with two matches, the three flags."""
    case = HAND[name]
    ref, ref_flags = case.stats()
    assert ref_flags == case.flags
    for layout in (0, 1):
        check(*run(ctx, case, layout), ref, ref_flags)


def test_accumulation_is_ordered_and_repeatable(ctx):
    cases = [blocky_case(s, h, w, n_gt, n) for s, h, w, n_gt, n in ((1, 67, 131, 37, 20), (108, 200, 333, 37, 100), (12, 200, 333, 37, 20))]
    ref = PQ.PQStats(6)
    for c in cases:
        c.stats(into=ref)                                # pair by pair onto the running sums, as the evaluator's one PQStat
    runs = []
    for _ in range(2):
        stats = flags = None
        for c in cases:
            stats, flags = run(ctx, c, 0, stats, flags)
        check(stats, flags, ref)
        runs.append(stats.numpy().tobytes())
    assert runs[0] == runs[1]
    assert (ref.tp > 1).any()                            # some category adds several pairs: the order of the additions is exercised


def test_flags_leave_the_statistics_alone_and_survive(ctx):
    good = Case(HAND["crowd"].pan_gt, HAND["crowd"].gt_rows, HAND["crowd"].pan_pred, HAND["crowd"].pred_rows, 3)
    ref, _ = good.stats()
    stats, flags = run(ctx, good)
    check(stats, flags, ref)
    seen = 0
    for name, bit in (("flag_empty_row", 2), ("flag_missing_id", 1), ("flag_bad_category", 4)):
        seen |= bit
        run(ctx, HAND[name], 0, stats, flags)
        check(stats, flags, ref, seen)                   # this picture's bit, the earlier ones, nothing added
    good.stats(into=ref)
    run(ctx, good, 0, stats, flags)
    check(stats, flags, ref, 7)


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    good = HAND["crowd"]
    ref, _ = good.stats()
    stats, flags = run(ctx, good)
    rows = np.tile(np.array([[5, 1, 0, 3]], np.int32), (255, 1))
    rows[:, 0] = np.arange(1, 256)
    bad = {"255 ground-truth segments": rows, "category": [(6, 1, 1, 4), (5, good.C, 0, 3)], "iscrowd": [(6, 1, 2, 4), (5, 2, 0, 3)]}
    for what, table in bad.items():
        case = Case(good.pan_gt, table, good.pan_pred, good.pred_rows, good.C)
        with pytest.raises(RuntimeError, match=what):
            run(ctx, case, 0, stats, flags)
    assert ctx.lib.odise_hip_panoptic_quality(ctx.h, None) == -1
    ctx.sync()
    check(stats, flags, ref)
    most = Case(good.pan_gt, rows[:254], good.pan_pred, good.pred_rows, good.C)      # 254 rows are accepted
    check(*run(ctx, most), most.stats()[0])


def test_model_record_goes_straight_into_the_evaluator(ctx):
    """odise_hip_infer (small model, panoptic_on) writes its record into a caller-owned buffer; that buffer is the evaluator's input."""
    from odise_amd.panoptic_eval import HipPanopticEvaluator
    from small_model import GROUPS, THINGS, build_small, image_u8
    hip = build_small(ctx, semantic_on=False, instance_on=False)
    h = w = 512
    img = ctx.to_device(np.ascontiguousarray(image_u8(h, w, seed=3).numpy()))
    rec = ctx.empty((h * w + 1 + 3 * MAX_SEGMENTS,), np.int32)
    hip.infer_device([img], 1, [(h, w)], [(h, w)], pan_out=[rec])
    first = rec.numpy()
    n = int(first[h * w])
    pred_rows = first[h * w + 1:h * w + 1 + 3 * n].reshape(n, 3)
    assert n >= 1
    # ground truth: the previous run's map, shifted; ids and categories in the annotation's own spaces; one segment left out of the table
    C = len(GROUPS)
    to_contiguous = {10 + c: c for c in range(C)}
    pan_gt = np.roll(first[:h * w].reshape(h, w), (3, 5), (0, 1)).astype(np.int64) * 1000
    info = [{"id": int(i) * 1000, "category_id": 10 + int(c), "iscrowd": 0, "area": int((pan_gt == int(i) * 1000).sum())} for i, _, c in pred_rows]
    info = info[::-1][:max(1, n - 1)] if n > 2 else info
    gt = Case(pan_gt, [(s["id"], s["category_id"] - 10, s["iscrowd"], s["area"]) for s in info], np.zeros((h, w)), [], C)
    gt_rgb = ctx.to_device(gt.rgb())

    hip.infer_device([img], 1, [(h, w)], [(h, w)], pan_out=[rec])           # the run under evaluation
    stats, flags = ctx.panoptic_quality_record(rec, (h, w), gt_rgb, gt.gt_rows, C)
    now = rec.numpy()
    n2 = int(now[h * w])
    ref, ref_flags = PQ.image_stats(gt.pan_gt, gt.gt_rows, now[:h * w], now[h * w + 1:h * w + 1 + 3 * n2].reshape(n2, 3), C)
    assert ref_flags == 0 and ref.tp.sum() + ref.fp.sum() + ref.fn.sum() > 0
    check(stats, flags, ref)

    isthing = [c in THINGS for c in range(C)]
    ev = HipPanopticEvaluator(ctx, to_contiguous, isthing)
    ev.process(rec, (h, w), gt_rgb, info)
    assert ev.evaluate() == PQ.results(ref, isthing)
    ev.process(rec, (h, w), gt_rgb, info)
    PQ.image_stats(gt.pan_gt, gt.gt_rows, now[:h * w], now[h * w + 1:h * w + 1 + 3 * n2].reshape(n2, 3), C, into=ref)
    assert ev.evaluate() == PQ.results(ref, isthing) and ev.pq_stats == ref
    ev.reset()
    assert not ev._buf.numpy().view(np.uint8).any()
    ev.process(ctx.to_device(HAND["flag_missing_id"].record(MAX_SEGMENTS)), (1, 4), HAND["flag_missing_id"].rgb(), [])
    with pytest.raises(RuntimeError, match="bit 0"):
        ev.evaluate()
