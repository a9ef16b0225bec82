"""GPU: odise_hip_semantic_pq (csrc/sem_pq.hip), odise_hip_semantic_eval_pq (csrc/eval_ops.hip), Context.semantic_pq and
HipSemSegEvaluator(pq=True) against the host specification odise_amd/semseg_pq.py.  Every comparison is exact: the counts as integers, the
iou sums bit for bit (PQStats.__eq__ compares the records' bytes)."""
import ctypes as C

import numpy as np
import pytest

import semseg_pq_cases as PC
from odise_amd import panoptic_quality as PQ
from odise_amd import semseg_eval as SE
from odise_amd import semseg_pq as SP
from odise_amd._lib import SemSegEvalDesc, SemSegPqTask

pytestmark = pytest.mark.gpu


def device_stats(stats):
    return PQ.PQStats.from_records(stats.numpy())


def run(ctx, case, stats=None, flags=None):
    return ctx.semantic_pq(ctx.to_device(case.pred), ctx.to_device(case.gt()), case.K, stats, flags)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_labels_equal_the_host_specification(ctx, name):
    """The crafted edges and every size / class count: 1x1, odd sizes, more than one block; K = 3072 counts in LDS, 3073 in global memory."""
    case = PC.CASES[name]
    stats, flags = run(ctx, case)
    assert device_stats(stats) == case.literal()[0] and int(flags.numpy()[0]) == 0
    if name == "blobs_64x64_K3073":
        assert 4 * 3072 == 12288 < 4 * case.K                                         # on the two sides of the LDS histogram's size
    if case.hw[0] * case.hw[1] > 4:                                                   # a map that is only 4-byte aligned: pixel by pixel
        h, w = case.hw
        pad = lambda m: ctx.to_device(np.concatenate([np.full(1, -7, np.int32), m.reshape(-1)])).view((h, w), np.int32, 4)
        stats2, _ = ctx.semantic_pq(pad(case.pred), pad(case.gt()), case.K)
        assert stats2.numpy().tobytes() == stats.numpy().tobytes()


@pytest.mark.parametrize("K", [3, 21])
def test_scores_with_ties_equal_the_call_on_their_argmax(ctx, K):
    sem = PC.score_cases()[K]
    top = np.sort(sem, axis=0)
    assert (top[-1] == top[-2]).mean() > 0.3                                          # exact ties between the two best planes
    amax = sem.argmax(0).astype(np.int32)                                             # numpy's arg-max is the first maximum: the lower class
    rng = np.random.default_rng(K)
    gt = np.where(rng.random(amax.shape) < 0.8, amax, rng.integers(0, K + 1, amax.shape)).astype(np.int32)
    d_gt = ctx.to_device(gt)
    from_scores, f1 = ctx.semantic_pq(ctx.to_device(sem), d_gt)
    from_labels, f2 = ctx.semantic_pq(ctx.to_device(amax), d_gt, K)
    assert from_scores.numpy().tobytes() == from_labels.numpy().tobytes() and int(f1.numpy()[0]) == int(f2.numpy()[0]) == 0
    want, _ = SP.picture_stats(amax, gt, K)
    assert device_stats(from_scores) == want and int(want.tp.sum()) >= 1


def test_a_stream_of_pictures_equals_the_host_in_order_and_repeats_bit_for_bit(ctx):
    cases = PC.stream_cases()
    assert len(cases) == 6 and len(set(c.hw for c in cases)) == 6
    want = PQ.PQStats(150)
    for c in cases:
        SP.image_stats_literal(c.pred, c.gt_raw, c.K, c.ignore_label, into=want)
    runs = []
    for _ in range(2):
        stats = flags = None
        for c in cases:
            stats, flags = run(ctx, c, stats, flags)
        runs.append(stats.numpy().tobytes())
        assert int(flags.numpy()[0]) == 0
    assert runs[0] == want.to_records().tobytes() and runs[0] == runs[1]
    assert int((want.tp > 1).sum()) >= 3                                              # sums of several addends: the order matters
    backwards = PQ.PQStats(150)
    for c in cases[::-1]:
        SP.picture_stats(c.pred, c.gt(), c.K, into=backwards)
    assert backwards.iou.tobytes() != want.iou.tobytes() and np.array_equal(backwards.tp, want.tp)


@pytest.mark.parametrize("bad", [-1, 150])
def test_a_bad_label_raises_the_flag_adds_nothing_and_leaves_the_counters_clean(ctx, bad):
    first, clean = PC.CASES["blobs_37x53_K150"], PC.CASES["blobs_64x64_K150"]
    stats, flags = run(ctx, first)
    before = stats.numpy().tobytes()
    pred = PC.CASES["blobs_130x257_K150"].pred.copy()
    pred[77, 100] = bad
    ctx.semantic_pq(ctx.to_device(pred), ctx.to_device(PC.CASES["blobs_130x257_K150"].gt()), 150, stats, flags)
    assert int(flags.numpy()[0]) == 1 and stats.numpy().tobytes() == before
    run(ctx, clean, stats, flags)                                                     # the flag stays up; the next picture counts all the same
    want = PQ.PQStats(150)
    for c in (first, clean):
        SP.picture_stats(c.pred, c.gt(), c.K, into=want)
    assert device_stats(stats) == want and int(flags.numpy()[0]) == 1


def eval_call(ctx, pred, K, gt, boundary, pq, capacity=1 << 16, n=40):
    """One bare odise_hip_semantic_eval / _eval_pq with every output -> the outputs as bytes by name (+ "stats" with pq)."""
    h, w = gt.shape
    outs = dict(conf=ctx.zeros(((K + 1) ** 2,), np.int64), classes=ctx.to_device(np.full(n, -9, np.int32)), n_classes=ctx.to_device(np.full(1, -9, np.int32)),
                rle=ctx.to_device(np.full(capacity, 0x7E, np.uint8)), offsets=ctx.to_device(np.full(n + 1, -9, np.int64)),
                area=ctx.to_device(np.full(n, -9, np.int64)), flags=ctx.zeros((1,), np.int32))
    if boundary:
        outs["b_conf"] = ctx.zeros(((K + 1) ** 2,), np.int64)
    d = SemSegEvalDesc()
    d.K, d.H, d.W, d.gt, d.max_classes, d.capacity = K, h, w, gt.ptr, n, capacity
    if pred.dtype == np.float32:
        d.sem_seg = pred.ptr
    else:
        d.labels = pred.ptr
    for k, v in outs.items():
        setattr(d, k, v.ptr)
    if pq:
        outs["stats"] = ctx.zeros((K,), PQ.STAT_DTYPE)
        t = SemSegPqTask()
        t.stats = outs["stats"].ptr
        assert ctx.lib.odise_hip_semantic_eval_pq(ctx.h, C.byref(d), C.byref(t)) == 0
    else:
        assert ctx.lib.odise_hip_semantic_eval(ctx.h, C.byref(d)) == 0
    return {k: v.numpy().tobytes() for k, v in outs.items()}


@pytest.mark.parametrize("route", ["labels", "scores"])
@pytest.mark.parametrize("K,boundary", [(21, True), (300, False)])
def test_eval_pq_leaves_what_eval_leaves_and_adds_the_bare_calls_statistics(ctx, K, boundary, route):
    case = PC.picture(f"eval_K{K}", 65, 67, K, seed=40 + K, ignore_label=65535)
    gt = ctx.to_device(case.gt())
    if route == "scores":
        rng = np.random.default_rng(K)
        sem = rng.integers(0, 2, (K, 65, 67)).astype(np.float32)                      # ties everywhere below the planted maximum
        np.put_along_axis(sem, case.pred[None].astype(np.int64), 3.0, axis=0)
        assert np.array_equal(sem.argmax(0), case.pred)
        pred = ctx.to_device(sem)
    else:
        pred = ctx.to_device(case.pred)
    plain = eval_call(ctx, pred, K, gt, boundary, pq=False)
    both = eval_call(ctx, pred, K, gt, boundary, pq=True)
    assert sorted(both) == sorted(list(plain) + ["stats"])
    for k, v in plain.items():
        assert both[k] == v, k
    assert np.frombuffer(plain["n_classes"], np.int32)[0] >= 6 and np.frombuffer(plain["offsets"], np.int64)[-1] > 0
    bare, _ = ctx.semantic_pq(pred, gt, K)
    assert both["stats"] == bare.numpy().tobytes() == case.literal()[0].to_records().tobytes()
    # the statistics alone: no matrix, no strings
    d = SemSegEvalDesc()
    d.K, d.H, d.W, d.gt = K, 65, 67, gt.ptr
    setattr(d, "sem_seg" if route == "scores" else "labels", pred.ptr)
    stats, flags = ctx.zeros((K,), PQ.STAT_DTYPE), ctx.zeros((1,), np.int32)
    d.flags = flags.ptr
    t = SemSegPqTask()
    t.stats = stats.ptr
    assert ctx.lib.odise_hip_semantic_eval_pq(ctx.h, C.byref(d), C.byref(t)) == 0
    assert stats.numpy().tobytes() == both["stats"]


def test_a_picture_that_needs_the_rle_retry_counts_once(ctx):
    case = PC.CASES["blobs_130x257_K150"]
    pred, gt = ctx.to_device(case.pred), ctx.to_device(case.gt())
    stats, conf = ctx.zeros((150,), PQ.STAT_DTYPE), ctx.zeros((151, 151), np.int64)
    p = ctx.semantic_eval_async(pred, 150, gt, conf=conf, capacity=8, max_classes=2, pq_stats=stats)
    classes, rles, _ = p.result()
    assert p.launches == 3                                                            # more classes than asked for, then the exact size
    assert SE.rows_from_rle(classes, rles, "f") == SE.encode_json_sem_seg(case.pred, "f")
    assert device_stats(stats) == case.literal()[0] and np.array_equal(conf.numpy(), SE.confusion(case.pred, case.gt(), 150))
    # without the statistics the same call is the old one
    q = ctx.semantic_eval_async(pred, 150, gt, capacity=8, max_classes=2)
    assert q.pq_stats is None and q.result()[1] == rles and np.array_equal(q.conf.numpy(), conf.numpy())


def test_the_evaluator_with_pq_appends_its_keys_and_leaves_the_others(ctx):
    K, names = 150, [f"c{c}" for c in range(150)]
    cases = [PC.CASES[n] for n in ("blobs_37x53_K150", "blobs_64x64_K150", "blobs_130x257_K150", "blobs_1x1_K150")]
    got = {}
    for pq in (False, True):
        ev = SE.HipSemSegEvaluator(ctx, names, 255, "blobs", pq=pq)
        for round_ in range(2):                                                       # reset() starts over, the statistics included
            ev.reset()
            for i, c in enumerate(cases):
                ev.process(ctx.to_device(c.pred), c.gt_raw, f"{i}.png")               # a host ground truth: the ignore label is mapped here
        got[pq] = (ev.evaluate()["blobs/sem_seg"], ev)
    want = PQ.PQStats(K)
    for c in cases:
        SP.image_stats_literal(c.pred, c.gt_raw, K, 255, into=want)
    plain, with_pq = got[False][0], got[True][0]
    assert got[True][1].pq_stats == want and not hasattr(got[False][1], "pq_stats")
    extra = SP.evaluator_results(want, names)
    assert list(with_pq) == list(plain) + list(extra) and list(extra)[:3] == ["PQ", "SQ", "RQ"]
    assert repr({k: with_pq[k] for k in plain}) == repr(dict(plain))                  # NaN compares by its text
    assert {k: with_pq[k] for k in extra} == dict(extra) and 0 < with_pq["PQ"] < 100
    assert got[True][1].predictions == got[False][1].predictions


def test_the_front_door_counts_a_predictions_file_against_label_images(ctx, tmp_path):
    cases = [PC.CASES[n] for n in ("blobs_37x53_K150", "blobs_64x64_K150", "blobs_130x257_K150")]
    path, gt_dir, _ = PC.write_pictures(tmp_path, cases, ["a", "b", "c"])
    stats, conf = SP.evaluate_file(ctx, path, gt_dir, 150, 255)
    want = PQ.PQStats(150)
    for c in cases:                                                                   # file order
        SP.image_stats_literal(c.pred, c.gt_raw, 150, 255, into=want)
    assert stats == want and np.array_equal(conf, sum(SE.confusion(c.pred, c.gt(), 150) for c in cases))
    assert len(SP.format_table(SP.results(stats)).splitlines()) == 4 and 0.0 < SP.tool_miou(conf) < 1.0


def test_bad_arguments_are_err_arg_and_write_nothing(ctx):
    K, h, w = 5, 9, 11
    labels, sem, gt = ctx.to_device(np.zeros((h, w), np.int32)), ctx.to_device(np.zeros((K, h, w), np.float32)), ctx.to_device(np.zeros((h, w), np.int32))
    stats, flags = ctx.to_device(np.full(4 * K, -5, np.int64)), ctx.to_device(np.full(1, -5, np.int32))
    f = ctx.lib.odise_hip_semantic_pq
    good = dict(ctx=ctx.h, labels=labels.ptr, sem_seg=None, gt=gt.ptr, K=K, H=h, W=w, stats=stats.ptr, flags=flags.ptr)
    bad = [{"ctx": None}, {"labels": None}, {"sem_seg": sem.ptr}, {"gt": None}, {"stats": None}, {"flags": None},
           {"H": 0}, {"W": 0}, {"H": -1}, {"H": 1 << 15, "W": 1 << 14},                # H * W = 2^29 > 2^29 - 1
           {"K": 0}, {"K": -1}, {"K": 12289}]
    for kw in bad:
        a = {**good, **kw}
        assert f(a["ctx"], a["labels"], a["sem_seg"], a["gt"], a["K"], a["H"], a["W"], a["stats"], a["flags"]) == -1, kw
    # the call beside the evaluator step: what that refuses, a null task, null statistics, no ground truth
    d = SemSegEvalDesc()
    d.K, d.H, d.W, d.labels, d.gt, d.flags = K, h, w, labels.ptr, gt.ptr, flags.ptr
    t = SemSegPqTask()
    t.stats = stats.ptr
    g = ctx.lib.odise_hip_semantic_eval_pq
    assert g(ctx.h, C.byref(d), None) == -1 and g(ctx.h, None, C.byref(t)) == -1 and g(None, C.byref(d), C.byref(t)) == -1
    empty = SemSegPqTask()
    assert g(ctx.h, C.byref(d), C.byref(empty)) == -1
    d.gt = None
    assert g(ctx.h, C.byref(d), C.byref(t)) == -1
    d.gt, d.K = gt.ptr, 12289
    assert g(ctx.h, C.byref(d), C.byref(t)) == -1
    d.K, d.sem_seg = K, sem.ptr                                                       # a doubled prediction
    assert g(ctx.h, C.byref(d), C.byref(t)) == -1
    ctx.sync()
    assert (stats.numpy() == -5).all() and (flags.numpy() == -5).all()
    # and the good call goes through (K = 12288, the cap, is allowed)
    d.sem_seg = None
    fresh, fl = ctx.zeros((K,), PQ.STAT_DTYPE), ctx.zeros((1,), np.int32)
    d.flags, t.stats = fl.ptr, fresh.ptr
    assert g(ctx.h, C.byref(d), C.byref(t)) == 0
    assert device_stats(fresh) == SP.picture_stats(np.zeros((h, w), np.int32), np.zeros((h, w), np.int32), K)[0]
