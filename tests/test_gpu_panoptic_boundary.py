"""GPU: odise_hip_panoptic_quality_boundary and odise_hip_segment_boundaries (csrc/pq.hip) against the host restatement
odise_amd.panoptic_quality (image_boundary_stats, segment_boundaries).  Statistics are compared as their raw 32-byte records: counts exact,
the iou bytes equal.  Every case also checks that `stats` is byte-equal to what odise_hip_panoptic_quality alone writes, that the bare
boundary call equals the literal per-segment boundaries on both maps, and that its areas are the pixel counts.  That the generated cases
demote and lower a pair is proven on the CPU (tests/test_panoptic_boundary_cpu.py)."""
import numpy as np
import pytest

import pq_boundary_cases as BC
from odise_amd import panoptic_quality as PQ
from odise_amd._lib import MAX_SEGMENTS
from pq_cases import hand_cases
from test_gpu_panoptic_quality import upload

pytestmark = pytest.mark.gpu

HAND = hand_cases()


def radius_of(case):
    return int(getattr(case, "radius", None) or 0)


def run(ctx, case, layout=0, acc=None, unaligned=False):
    """-> (stats, b_stats, flags) of the boundary call and (stats, flags) of the plain call on the same inputs, both added to `acc`'s."""
    rec, gt = upload(ctx, case, layout, unaligned)
    both, plain = acc if acc is not None else ((None, None, None), (None, None))
    both = ctx.panoptic_quality_boundary_record(rec, case.pan_gt.shape, gt, case.gt_rows, case.C, *both, radius=radius_of(case))
    plain = ctx.panoptic_quality_record(rec, case.pan_gt.shape, gt, case.gt_rows, case.C, *plain)
    return both, plain


def check_records(arr, ref):
    got = PQ.PQStats.from_records(arr.numpy())
    assert np.array_equal(got.tp, ref.tp) and np.array_equal(got.fp, ref.fp) and np.array_equal(got.fn, ref.fn), (got, ref)
    assert got.iou.tobytes() == ref.iou.tobytes(), (got, ref)       # the raw 8 bytes
    assert arr.numpy().tobytes() == ref.to_records().tobytes()


def check(acc, ref, b_ref, ref_flags=0):
    (stats, b_stats, flags), (p_stats, p_flags) = acc
    assert int(flags.numpy()[0]) == ref_flags == int(p_flags.numpy()[0])
    assert stats.numpy().tobytes() == p_stats.numpy().tobytes()     # what odise_hip_panoptic_quality alone writes
    check_records(stats, ref)
    check_records(b_stats, b_ref)


def check_boundaries(ctx, case):
    """odise_hip_segment_boundaries on both maps: the map equals the literal one, the areas are its pixel counts."""
    r = radius_of(case)
    for pan, ids in ((case.pan_gt, case.gt_rows[:, 0]), (case.pan_pred, case.pred_rows[:, 0])):
        ref = PQ.segment_boundaries(pan, ids, r or None)
        got, area = ctx.segment_boundaries(ctx.to_device(np.ascontiguousarray(pan, np.int32)), ids, r, with_area=True)
        assert np.array_equal(got.numpy(), ref)
        if len(ids):
            first = [int(np.flatnonzero(ids == i)[0]) == k and i != 0 for k, i in enumerate(ids)]
            counts = [int(((pan == i) & (ref != 0)).sum()) if f else 0 for i, f in zip(ids, first)]
            assert area.numpy().tolist() == counts
        else:
            assert area is None and not ref.any()


def whole_case(ctx, case, layout=0, unaligned=False):
    ref, ref_flags = case.stats()
    b_ref, b_flags = case.boundary_stats()
    assert ref_flags == b_flags == 0
    check(run(ctx, case, layout, unaligned=unaligned), ref, b_ref)
    check_boundaries(ctx, case)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("seed,h,w,n_gt,n", BC.SIZES)
def test_sizes_and_ground_truth_layouts(ctx, seed, h, w, n_gt, n, layout):
    case = BC.size_case(seed, h, w, n_gt, n)
    if BC.must_fire(case):
        assert case.boundary_stats()[0] != case.stats()[0]
    whole_case(ctx, case, layout)


@pytest.mark.parametrize("radius", BC.RADII)
def test_explicit_radii(ctx, radius):
    whole_case(ctx, BC.radius_case(radius))


@pytest.mark.parametrize("n_gt,n", BC.TABLES)
def test_table_sizes(ctx, n_gt, n):
    case = BC.table_case(n_gt, n)
    assert len(case.gt_rows) == n_gt and len(case.pred_rows) == n
    whole_case(ctx, case)


@pytest.mark.parametrize("layout", [0, 1])
def test_a_record_and_ground_truth_that_are_not_16_byte_aligned(ctx, layout):
    case = BC.boundary_case(1, 67, 131, 37, 20)
    rec, gt = upload(ctx, case, layout, unaligned=True)
    assert rec.ptr % 16 == 4 and gt.ptr % 16 == (1 if layout == 0 else 4)
    whole_case(ctx, case, layout, unaligned=True)


def test_a_stream_of_three_pictures(ctx):
    cases = BC.stream_cases()
    ref, b_ref = PQ.PQStats(6), PQ.PQStats(6)
    for c in cases:
        c.stats(into=ref)
        c.boundary_stats(into=b_ref)
    runs = []
    for _ in range(2):
        acc = None
        for c in cases:
            acc = run(ctx, c, 0, acc)
        check(acc, ref, b_ref)
        runs.append(acc[0][1].numpy().tobytes())
    assert runs[0] == runs[1]
    assert (b_ref.tp > 1).any() and b_ref != ref


def test_a_missing_id_sets_the_flag_and_changes_neither_accumulator(ctx):
    good = BC.boundary_case(1, 67, 131, 37, 20)
    ref, _ = good.stats()
    b_ref, _ = good.boundary_stats()
    acc = run(ctx, good)
    check(acc, ref, b_ref)
    bad = BC.boundary_case(1, 67, 131, 37, 20)
    bad.pan_pred[30:33, 40:47] = 123456                  # an id that no row carries
    assert bad.boundary_stats()[1] == PQ.FLAG_MISSING_ID
    acc = run(ctx, bad, 0, acc)
    check(acc, ref, b_ref, PQ.FLAG_MISSING_ID)
    good.stats(into=ref)
    good.boundary_stats(into=b_ref)
    acc = run(ctx, good, 0, acc)                         # both matrices were left zeroed
    check(acc, ref, b_ref, PQ.FLAG_MISSING_ID)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_one_row_pictures(ctx, name):
    """One row: every pixel is a boundary pixel; the three flags among them."""
    case = HAND[name]
    ref, ref_flags = case.stats()
    b_ref, b_flags = PQ.image_boundary_stats(case.pan_gt, case.gt_rows, case.pan_pred, case.pred_rows, case.C)
    assert ref_flags == b_flags == case.flags
    check(run(ctx, case), ref, b_ref, ref_flags)


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    from odise_amd.panoptic_quality import STAT_DTYPE
    good = HAND["crowd"]
    rec, gt = upload(ctx, good)
    buf = ctx.zeros((2 * good.C,), STAT_DTYPE)
    stats = buf.view((good.C,), STAT_DTYPE)
    overlapping = buf.view((good.C,), STAT_DTYPE, STAT_DTYPE.itemsize)
    flags = ctx.zeros((1,), np.int32)
    with pytest.raises(RuntimeError, match="overlap"):
        ctx.panoptic_quality_boundary_record(rec, good.pan_gt.shape, gt, good.gt_rows, good.C, stats, overlapping, flags)
    assert ctx.lib.odise_hip_panoptic_quality_boundary(ctx.h, None, None) == -1
    with pytest.raises(RuntimeError, match="table of 255"):
        ctx.segment_boundaries(ctx.to_device(good.pan_gt), np.arange(1, 256))
    ctx.sync()
    assert not buf.numpy().view(np.uint8).any() and int(flags.numpy()[0]) == 0


def test_evaluator_with_boundary_end_to_end(ctx):
    from odise_amd.panoptic_eval import HipPanopticEvaluator
    cases = [BC.boundary_case(1, 67, 131, 37, 20), BC.boundary_case(12, 200, 333, 37, 20)]
    C = cases[0].C
    isthing = [c % 2 == 0 for c in range(C)]
    to_contiguous = {10 + c: c for c in range(C)}
    ev = HipPanopticEvaluator(ctx, to_contiguous, isthing, boundary=True)
    plain = HipPanopticEvaluator(ctx, to_contiguous, isthing)
    ref, b_ref = PQ.PQStats(C), PQ.PQStats(C)
    for c in cases:
        info = [{"id": int(i), "category_id": 10 + int(cat), "iscrowd": int(crowd), "area": int(area)} for i, cat, crowd, area in c.gt_rows]
        rec = ctx.to_device(c.record(MAX_SEGMENTS))
        for e in (ev, plain):
            e.process(rec, c.pan_gt.shape, ctx.to_device(c.rgb()), info)
        c.stats(into=ref)
        c.boundary_stats(into=b_ref)
    out = ev.evaluate()
    assert out == {**PQ.results(ref, isthing), **PQ.boundary_results(b_ref, isthing)}
    assert ev.pq_stats == ref and ev.boundary_stats == b_ref and out["BPQ"] < out["PQ"]
    assert plain.evaluate() == PQ.results(ref, isthing)                     # boundary=False: the dict of today
