"""GPU: odise_hip_semantic_eval (csrc/eval_ops.hip, csrc/sem_rle.hip), Context.semantic_eval and HipSemSegEvaluator against the host
restatement odise_amd/semseg_eval.py, the numpy counters (oracle/eval_ops.py, odise_amd/sem_boundary.py) and the two bare counting calls."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from odise_amd import sem_boundary as SB
from odise_amd import semseg_eval as SE
from odise_amd._lib import MAX_SEGMENTS, SemSegEvalDesc
from semseg_cases import CASES, argmax_first, score_cases

pytestmark = pytest.mark.gpu


def upload_labels(ctx, case):
    """The case's map on the device; `offset`: behind one int32 of padding, so the pointer is 4-byte aligned and no more."""
    if not case.offset:
        return ctx.to_device(case.labels)
    h, w = case.hw
    buf = ctx.to_device(np.concatenate([np.full(1, -7, np.int32), case.labels.reshape(-1)]))
    return buf.view((h, w), np.int32, 4)


def raw_call(ctx, case, labels, max_classes, capacity):
    """One bare call -> (classes, n_classes, offsets, area, bytes, flags) as the device wrote them, with guard values behind every output."""
    n = max_classes
    classes, n_classes = ctx.to_device(np.full(n + 2, -9, np.int32)), ctx.to_device(np.full(2, -9, np.int32))
    offsets, area = ctx.to_device(np.full(n + 3, -9, np.int64)), ctx.to_device(np.full(n + 2, -9, np.int64))
    buf, flags = ctx.to_device(np.full(capacity + 16, 0x7E, np.uint8)), ctx.zeros((2,), np.int32)
    d = SemSegEvalDesc()
    d.K, d.H, d.W, d.labels, d.max_classes, d.classes, d.n_classes = case.K, case.hw[0], case.hw[1], labels.ptr, n, classes.ptr, n_classes.ptr
    d.rle, d.capacity, d.offsets, d.area, d.flags = buf.ptr, capacity, offsets.ptr, area.ptr, flags.ptr
    assert ctx.lib.odise_hip_semantic_eval(ctx.h, C.byref(d)) == 0
    out = [a.numpy() for a in (classes, n_classes, offsets, area, buf, flags)]
    assert (out[0][n:] == -9).all() and out[1][1] == -9 and (out[2][n + 1:] == -9).all() and (out[3][n:] == -9).all() and out[5][1] == 0
    assert (out[4][capacity:] == 0x7E).all()                                          # nothing is written past the capacity
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_classes_offsets_area_and_string_bytes_equal_the_host_restatement(ctx, name):
    case = CASES[name]
    labels = upload_labels(ctx, case)
    want_classes, want_strings, want_area = case.expected()
    n_present, total = len(want_classes), sum(len(s) for s in want_strings)
    # the protocol of the bare call, twice: bytes equal from run to run
    n = case.max_classes or (case.K + 2 if case.K <= 3 else MAX_SEGMENTS)            # K + 2: entries that no class can fill
    enc = min(n, n_present)
    enc_bytes = "".join(want_strings[:enc]).encode("ascii")
    runs = [raw_call(ctx, case, labels, n, len(enc_bytes) + 5) for _ in range(2)]
    classes, n_classes, offsets, area, buf, flags = runs[0]
    assert int(n_classes[0]) == n_present and int(flags[0]) == case.flag
    assert classes[:enc].tolist() == want_classes[:enc].tolist() and (classes[enc:n] == -1).all()
    want_off = np.cumsum([0] + [len(s) for s in want_strings[:enc]] + [0] * (n - enc))
    assert offsets[:n + 1].tolist() == want_off.tolist()                              # past the count: empty strings ..
    assert area[:enc].tolist() == want_area[:enc].tolist() and (area[enc:n] == 0).all()   # .. of area 0
    assert buf[:len(enc_bytes)].tobytes() == enc_bytes and (buf[len(enc_bytes):] == 0x7E).all()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], runs[1]))
    if enc_bytes:                                                                    # one byte short: offsets complete, no string written
        short = raw_call(ctx, case, labels, n, len(enc_bytes) - 1)
        assert short[2].tobytes() == offsets.tobytes() and short[3].tobytes() == area.tobytes() and (short[4] == 0x7E).all()
    # the Python route with its retries returns every present class
    pending = ctx.semantic_eval_async(labels, case.K, max_classes=case.max_classes)
    got_classes, rles, got_area = pending.result()
    assert got_classes.tolist() == want_classes.tolist() and [r["counts"] for r in rles] == want_strings and got_area.tolist() == want_area.tolist()
    assert all(r["size"] == list(case.hw) for r in rles) and int(pending.flags.numpy()[0]) == case.flag
    assert pending.launches == 1 + (n_present > (case.max_classes or MAX_SEGMENTS)) + (total > ctx.sem_rle_bytes(case.hw)), pending.launches
    if not case.flag:
        rows = SE.rows_from_rle(got_classes, rles, "f")
        assert rows == SE.encode_json_sem_seg(case.labels, "f")


def test_the_checkerboards_need_the_retry_with_the_exact_size(ctx):
    forced = [c for n, c in CASES.items() if n.startswith("checker") and sum(len(s) for s in c.expected()[1]) > ctx.sem_rle_bytes(c.hw)]
    assert len(forced) >= 6
    case = forced[-1]
    pending = ctx.semantic_eval_async(ctx.to_device(case.labels), case.K)
    assert pending.result()[1] and pending.launches == 2 and pending.capacity == sum(len(s) for s in case.expected()[1])


@pytest.mark.parametrize("name", sorted(score_cases()))
def test_scores_equal_the_labels_path_on_their_own_argmax(ctx, name):
    sem = score_cases()[name]
    K = sem.shape[0]
    amax = argmax_first(sem)
    if name.startswith("ties"):
        assert ((np.sort(sem, axis=0)[-1] == np.sort(sem, axis=0)[-2]).mean() > 0.3)  # exact ties between the two best planes
    from_scores = ctx.semantic_eval(ctx.to_device(sem))
    from_labels = ctx.semantic_eval(ctx.to_device(amax), K)
    assert from_scores[0].tolist() == from_labels[0].tolist() == np.unique(amax).tolist()
    assert from_scores[1] == from_labels[1] and from_scores[2].tolist() == from_labels[2].tolist()
    assert SE.rows_from_rle(from_scores[0], from_scores[1], "s") == SE.encode_json_sem_seg(amax, "s")


def _count(ctx, pred, K, gt, boundary, conf=None, b_conf=None):
    conf = conf if conf is not None else ctx.zeros((K + 1, K + 1), np.int64)
    b_conf = (b_conf if b_conf is not None else ctx.zeros((K + 1, K + 1), np.int64)) if boundary else None
    p = ctx.semantic_eval_async(pred, K, gt, conf=conf, b_conf=b_conf, rle=False)
    assert p.launches == 1 and p.result()[1] == []
    return conf, b_conf, p.flags


@pytest.mark.parametrize("name", ["ties_K3", "random_K150"])
def test_counters_from_scores_equal_the_restatements_and_the_bare_calls_over_two_pictures(ctx, name):
    from oracle.eval_ops import semantic_confusion
    sem = score_cases()[name]
    K, h, w = sem.shape
    rng = np.random.default_rng(11)
    sems = [sem, np.ascontiguousarray(sem[:, ::-1, :])]
    gts = [rng.integers(0, K + 1, (h, w)).astype(np.int32) for _ in sems]
    gts[1][::7] = -3                                                                   # outside [0, K]: column K
    conf = b_conf = None
    ref_conf, ref_b = ctx.zeros((K + 1, K + 1), np.int64), ctx.zeros((K + 1, K + 1), np.int64)
    want_conf, want_b = np.zeros((K + 1, K + 1), np.int64), np.zeros((K + 1, K + 1), np.int64)
    for s, g in zip(sems, gts):
        d_s, d_g = ctx.to_device(s), ctx.to_device(g)
        conf, b_conf, flags = _count(ctx, d_s, K, d_g, True, conf, b_conf)
        ctx.semantic_boundary_confusion(d_s, d_g, ref_conf, ref_b)
        want_conf += semantic_confusion(s, SB.clamp_labels(g, K), ignore_label=K)
        want_b += SB.boundary_confusion(argmax_first(s), g, K)
    assert np.array_equal(conf.numpy(), want_conf) and np.array_equal(b_conf.numpy(), want_b) and int(flags.numpy()[0]) == 0
    assert conf.numpy().tobytes() == ref_conf.numpy().tobytes() and b_conf.numpy().tobytes() == ref_b.numpy().tobytes()
    only = ctx.semantic_confusion(ctx.to_device(sems[0]), ctx.to_device(gts[0]))       # conf alone, as odise_hip_semantic_confusion adds
    got, _, _ = _count(ctx, ctx.to_device(sems[0]), K, ctx.to_device(gts[0]), False)
    assert got.numpy().tobytes() == only.numpy().tobytes()
    # a radius of the caller's
    _, b3, _ = _count(ctx, ctx.to_device(sems[0]), K, ctx.to_device(gts[0]), True)
    p = ctx.semantic_eval_async(ctx.to_device(sems[0]), K, ctx.to_device(gts[0]), b_conf=ctx.zeros((K + 1, K + 1), np.int64), radius=3, rle=False)
    assert np.array_equal(p.b_conf.numpy(), SB.boundary_confusion(argmax_first(sems[0]), gts[0], K, 3)) and p.conf is None
    assert np.array_equal(b3.numpy(), SB.boundary_confusion(argmax_first(sems[0]), gts[0], K))


@pytest.mark.parametrize("name", ["hstripes_65x67_K847", "single_row64_K847", "offset_pointer_65x67_K847", "bad_minus1_K150", "bad_labelK_K150",
                                  "checker3_129x67_K150", "checker3_129x3_K3"])
def test_counters_from_labels_against_bincount(ctx, name):
    case = CASES[name]
    assert name != "hstripes_65x67_K847" or (case.K + 1) ** 2 == 719104                 # the global-memory side of the histogram
    boundary = case.K <= SB.MAX_CLASSES
    conf, b_conf, flags = _count(ctx, upload_labels(ctx, case), case.K, ctx.to_device(case.gt()), boundary)
    assert np.array_equal(conf.numpy(), case.conf()) and int(flags.numpy()[0]) == case.flag
    assert int(conf.numpy().sum()) == int(case.valid().sum())                         # a label outside [0, K) is counted nowhere
    if boundary:
        assert np.array_equal(b_conf.numpy(), SB.boundary_confusion(np.where(case.valid(), case.labels, case.K), case.gt(), case.K))


@pytest.mark.parametrize("K", [109, 110])
def test_counters_on_both_sides_of_the_lds_histogram_limit(ctx, K):
    assert ((K + 1) ** 2 <= 12288) == (K == 109)
    rng = np.random.default_rng(K)
    labels, gt = rng.integers(0, K, (65, 67)).astype(np.int32), rng.integers(0, K + 1, (65, 67)).astype(np.int32)
    conf, b_conf, _ = _count(ctx, ctx.to_device(labels), K, ctx.to_device(gt), True)
    assert np.array_equal(conf.numpy(), SE.confusion(labels, gt, K)) and np.array_equal(b_conf.numpy(), SB.boundary_confusion(labels, gt, K))
    # counting and the strings in one call
    p = ctx.semantic_eval_async(ctx.to_device(labels), K, ctx.to_device(gt))
    classes, rles, _ = p.result()
    assert np.array_equal(p.conf.numpy(), SE.confusion(labels, gt, K)) and SE.rows_from_rle(classes, rles, "x") == SE.encode_json_sem_seg(labels, "x")
    total = sum(len(r["counts"]) for r in rles)
    assert len(classes) == K > MAX_SEGMENTS and p.launches == 2 + (total > ctx.sem_rle_bytes((65, 67)))   # all K classes: the retry for more


def test_bad_arguments_are_err_arg_and_write_nothing(ctx):
    K, h, w, n = 5, 9, 11, 4
    labels, sem, gt = ctx.to_device(np.zeros((h, w), np.int32)), ctx.to_device(np.zeros((K, h, w), np.float32)), ctx.to_device(np.zeros((h, w), np.int32))
    big = ctx.to_device(np.zeros(8, np.int32))
    outs = dict(conf=ctx.to_device(np.full((K + 1) ** 2, -5, np.int64)), b_conf=ctx.to_device(np.full((K + 1) ** 2, -5, np.int64)),
                classes=ctx.to_device(np.full(n, -5, np.int32)), n_classes=ctx.to_device(np.full(1, -5, np.int32)),
                rle=ctx.to_device(np.full(64, 0x7E, np.uint8)), offsets=ctx.to_device(np.full(n + 1, -5, np.int64)),
                area=ctx.to_device(np.full(n, -5, np.int64)), flags=ctx.to_device(np.full(1, -5, np.int32)))

    def desc(**kw):
        d = SemSegEvalDesc()
        d.K, d.H, d.W, d.labels, d.gt, d.max_classes, d.capacity = K, h, w, labels.ptr, gt.ptr, n, 64
        for k, v in outs.items():
            setattr(d, k, v.ptr)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = [{"labels": None}, {"sem_seg": sem.ptr},                                     # a null and a doubled prediction
           {"gt": None}, {"gt": None, "b_conf": None}, {"gt": None, "conf": None},     # counting outputs without a ground truth
           {"H": 0}, {"W": 0}, {"H": -1}, {"H": 1 << 15, "W": 1 << 14, "labels": big.ptr},    # H * W = 2^29 > 2^29 - 1
           {"K": 0}, {"K": 12289}, {"K": 255},                                         # 255 classes with a boundary matrix
           {"max_classes": 0}, {"max_classes": 65536}, {"max_classes": -1},
           {"flags": None}, {"classes": None}, {"n_classes": None}, {"capacity": -1}, {"rle": None},
           {"conf": None, "b_conf": None, "offsets": None}]                            # nothing asked for
    for kw in bad:
        assert ctx.lib.odise_hip_semantic_eval(ctx.h, C.byref(desc(**kw))) == -1, kw
    assert ctx.lib.odise_hip_semantic_eval(ctx.h, None) == -1
    ctx.sync()
    for k, v in outs.items():
        host = v.numpy()
        assert (host == (0x7E if k == "rle" else -5)).all(), k
    d = desc(K=255, b_conf=None)                                                       # without the boundary matrix 255 classes are fine
    big_conf = ctx.zeros((256 * 256,), np.int64)
    d.conf = big_conf.ptr
    assert ctx.lib.odise_hip_memset(ctx.h, outs["flags"].ptr, 0, 4) == 0
    assert ctx.lib.odise_hip_semantic_eval(ctx.h, C.byref(d)) == 0
    assert int(big_conf.numpy()[0]) == h * w and int(outs["n_classes"].numpy()[0]) == 1 and outs["classes"].numpy().tolist() == [0, -1, -1, -1]


@pytest.fixture(scope="module")
def small_pictures(ctx):
    """Three small pictures through the small model: the score tensors stay on the device, the ground truth is seeded."""
    from small_model import GROUPS, build_small, image_u8
    hip = build_small(ctx, panoptic_on=False, instance_on=False)
    K = len(GROUPS)
    pics = []
    for i, (h, w) in enumerate([(130, 67), (64, 129), (97, 120)]):
        res = hip.forward([{"image": image_u8(256, 256, seed=20 + i), "height": h, "width": w}], to_host=False)[0]
        assert res["sem_seg"].shape == (K, h, w) and res["sem_seg"].dtype == np.float32
        host = res["sem_seg"].numpy()
        sem = ctx.to_device(host)                                                      # a buffer of its own: the model's is reused by the next forward
        amax = argmax_first(host)
        rng = np.random.default_rng(i)
        gt = np.where(rng.random((h, w)) < 0.7, amax, rng.integers(0, K, (h, w))).astype(np.int32)
        gt[rng.random((h, w)) < 0.1] = 255
        pics.append(dict(sem=sem, amax=amax, gt=gt, file_name=f"pic{i}.jpg"))
    return K, pics


def test_the_evaluator_equals_the_host_restatement_from_scores_and_from_labels(ctx, small_pictures, tmp_path):
    K, pics = small_pictures
    names = [f"class {c}" for c in range(K)]
    mapping = {c: 10 + 2 * c for c in range(K)}
    got = {}
    for route in ("scores", "labels"):
        ev = SE.HipSemSegEvaluator(ctx, names, 255, "small_sem_seg_val", prefix="open", contiguous_id_to_dataset_id=mapping)
        for round_ in range(2):                                                        # reset() starts over
            ev.reset()
            for p in pics:
                ev.process(p["sem"] if route == "scores" else ctx.to_device(p["amax"]), p["gt"], p["file_name"])
        out = str(tmp_path / route)
        got[route] = (ev.evaluate(out), json.load(open(os.path.join(out, "sem_seg_predictions.json"))), ev.conf_matrix, ev.b_conf_matrix)
    conf, b_conf, rows = np.zeros((K + 1, K + 1), np.int64), np.zeros((K + 1, K + 1), np.int64), []
    for p in pics:
        g = np.where(p["gt"] == 255, K, p["gt"])
        conf += SE.confusion(p["amax"], g, K)
        b_conf += SB.boundary_confusion(p["amax"], g, K)
        rows += SE.encode_json_sem_seg(p["amax"], p["file_name"], mapping)
    want = {"small_sem_seg_val/open_sem_seg": SE.results(conf, b_conf, names)}
    for route, (res, js, c, b) in got.items():
        assert np.array_equal(c, conf) and np.array_equal(b, b_conf), route
        assert repr(res) == repr(want), route                                          # key order included; NaN compares by its text
        assert js == rows, route
    assert repr(got["scores"][0]) == repr(got["labels"][0]) and got["scores"][1] == got["labels"][1]
    # a device ground truth must already be mapped; a flagged picture makes evaluate() raise
    ev = SE.HipSemSegEvaluator(ctx, names, 255, "d", compute_boundary_iou=False)
    ev.process(ctx.to_device(pics[0]["amax"]), ctx.to_device(np.where(pics[0]["gt"] == 255, K, pics[0]["gt"]).astype(np.int32)), "a")
    res = ev.evaluate()["d/sem_seg"]
    assert "BoundaryIoU-class 0" not in res and repr(res) == repr(SE.results(SE.confusion(pics[0]["amax"], np.where(pics[0]["gt"] == 255, K, pics[0]["gt"]), K), None, names))
    bad = pics[0]["amax"].copy()
    bad[0, 0] = K
    ev.reset()
    ev.process(ctx.to_device(bad), pics[0]["gt"], "a")
    with pytest.raises(RuntimeError, match="outside"):
        ev.evaluate()


def test_the_evaluator_on_maps_of_several_classes_from_one_hot_scores_and_from_labels(ctx):
    """The synthetic small model predicts few classes per picture: the same comparison on smooth maps of six classes each."""
    from semseg_cases import blobs
    K, names = 150, [f"c{c}" for c in range(150)]
    maps = [blobs(65, 67, K, seed=200 + i) for i in range(2)]
    gts = [np.where(np.random.default_rng(i).random(m.shape) < 0.8, m, 255).astype(np.int32) for i, m in enumerate(maps)]
    got = []
    for route in ("scores", "labels"):
        ev = SE.HipSemSegEvaluator(ctx, names, 255, "blobs")
        for i, (m, g) in enumerate(zip(maps, gts)):
            pred = ctx.to_device((np.arange(K)[:, None, None] == m[None]).astype(np.float32)) if route == "scores" else ctx.to_device(m)
            ev.process(pred, g, f"{i}.png")
        got.append((ev.evaluate(), ev.predictions))
    conf = sum(SE.confusion(m, np.where(g == 255, K, g), K) for m, g in zip(maps, gts))
    b_conf = sum(SB.boundary_confusion(m, np.where(g == 255, K, g), K) for m, g in zip(maps, gts))
    rows = [r for i, m in enumerate(maps) for r in SE.encode_json_sem_seg(m, f"{i}.png")]
    assert len(set(r["category_id"] for r in rows)) >= 6
    for res, pred_rows in got:
        assert repr(res) == repr({"blobs/sem_seg": SE.results(conf, b_conf, names)}) and pred_rows == rows
