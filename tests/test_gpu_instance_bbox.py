"""Boxes of instance masks and the bbox task of instance evaluation on the device (odise_amd/csrc/inst_box.hip, inst_eval.hip):
`odise_hip_instance_boxes`, `odise_hip_box_iou` and `odise_hip_instance_eval_bbox` against the host restatement
(odise_amd/instance_eval.py, itself pinned by tests/test_instance_bbox_cpu.py) - integers equal, doubles bit for bit, rows byte for byte -
on crafted masks, on the small model's mask logits, `HipInstanceSegEvaluator(tasks=("bbox", "segm"))` end to end and the model's
`instance_boxes` switch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import inst_bbox_cases as BC
import inst_cases as IC
from odise_amd import instance_eval as IE
from odise_amd._lib import F32, U8, InstBboxTask, InstEvalDesc
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator
from small_model import GROUPS, build_small, image_u8
from test_gpu_instance_eval import Guarded, _annotations_from, _pad_case

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


# ---- boxes, dense path --------------------------------------------------------------------------------------------------------------------
def _dense_boxes(ctx, masks, topk=None, count=None):
    """-> boxes [topk, 4] through a guarded output; count: the table's count (None: no table)"""
    topk = topk or len(masks)
    table = None
    if count is not None:
        host = np.zeros(1 + 2 * topk, np.int32)
        host[0] = count
        table = ctx.to_device(host)
    out = Guarded(ctx, (topk, 4), np.float32)
    ctx.instance_boxes(masks.shape[1:], topk, table, masks=ctx.to_device(masks), boxes=out.arr)
    ctx.sync()
    return out.read()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 130), (130, 1), (63, 5), (64, 5), (65, 5), (200, 300)])
def test_boxes_of_the_mask_set(ctx, h, w, dtype):
    ms = IC.mask_set(h, w)
    ms = ms if dtype == np.uint8 else ms.astype(np.float32) * np.float32(0.75)
    np.testing.assert_array_equal(_dense_boxes(ctx, ms), IE.mask_boxes(ms))


def test_boxes_of_crafted_masks(ctx):
    h, w = 65, 7
    m = np.zeros((6, h, w), np.uint8)
    m[1] = 1
    m[2, 63, 3] = 1
    m[3, 64, 3] = 1
    m[4, h - 1, 6] = 1
    m[5, 0, 6] = m[5, h - 1, 0] = 1
    want = np.asarray([[0, 0, 0, 0], [0, 0, w, h], [3, 63, 4, 64], [3, 64, 4, 65], [6, 64, 7, 65], [0, 0, w, h]], np.float32)
    np.testing.assert_array_equal(IE.mask_boxes(m), want)
    np.testing.assert_array_equal(_dense_boxes(ctx, m), want)
    # a picture of 300 words per column: more words per column than the block has threads
    tall = np.zeros((2, 64 * 300 - 5, 3), np.uint8)
    tall[0, 64 * 299, 2] = tall[0, 777, 1] = 1
    tall[1, -1, 0] = 1
    np.testing.assert_array_equal(_dense_boxes(ctx, tall), IE.mask_boxes(tall))


def test_rows_past_the_count_are_zeros(ctx):
    """topk = 100 with a count of 3: rows 3..99 are zeros although their masks are all ones; a count of 0 gives zeros only."""
    h, w = 65, 9
    masks = np.ones((100, h, w), np.uint8)
    masks[:3] = IC.mask_set(h, w)[[7, 2, 0]]                                # blobs, a corner pixel, the empty mask
    want = np.zeros((100, 4), np.float32)
    want[:3] = IE.mask_boxes(masks[:3])
    assert want[0].any() and not want[2].any()
    np.testing.assert_array_equal(_dense_boxes(ctx, masks, 100, count=3), want)
    np.testing.assert_array_equal(_dense_boxes(ctx, masks, 100, count=0), np.zeros((100, 4), np.float32))
    np.testing.assert_array_equal(_dense_boxes(ctx, masks, 100, count=1000)[3:], np.asarray([[0, 0, w, h]] * 97, np.float32))   # clamped to topk


def test_boxes_bad_arguments_write_nothing(ctx):
    from odise_amd._lib import InstBoxesDesc
    masks = ctx.to_device(IC.mask_set(20, 9))
    out = Guarded(ctx, (101, 4), np.float32)

    def call(**over):
        d = InstBoxesDesc()
        d.h, d.w, d.masks, d.dtype, d.topk, d.boxes = 20, 9, masks.ptr, U8, 9, out.arr.ptr
        for k, v in over.items():
            setattr(d, k, v)
        return ctx.lib.odise_hip_instance_boxes(ctx.h, C.byref(d)), ctx.lib.odise_hip_last_error().decode()

    for over, word in (({"topk": 0}, "topk"), ({"topk": 101}, "topk"), ({"h": 0}, "size"), ({"dtype": 0}, "dtype"), ({"boxes": None}, "null"),
                       ({"masks": None}, "null")):
        rc, msg = call(**over)
        assert rc != 0 and word in msg, (over, rc, msg)
    ctx.sync()
    out.read(intact=True)
    assert call()[0] == 0
    ctx.sync()
    np.testing.assert_array_equal(out.read()[:9], IE.mask_boxes(IC.mask_set(20, 9)))


# ---- box_iou ------------------------------------------------------------------------------------------------------------------------------
def test_box_iou_is_bit_equal_to_the_host_loop(ctx):
    """100 x 40 fractional boxes (sixteenths and free doubles), crowds, pairs that touch and pairs that miss."""
    g = np.random.default_rng(21)
    gt = np.concatenate([g.random((40, 2)) * 60, g.random((40, 2)) * 30 + 0.25], 1)
    gt[::3] = np.round(gt[::3] * 16) / 16
    dt = np.concatenate([gt[g.integers(0, 40, 100), :2] + g.integers(-3, 4, (100, 2)), g.integers(1, 30, (100, 2))], 1).astype(np.float64)
    dt[:10] = gt[:10]                                                       # identical boxes
    dt[10:20, 0] = gt[10:20, 0] + gt[10:20, 2]                              # touching edges
    crowd = (g.random(40) < 0.25).astype(np.uint8)
    want = IE.box_iou(dt, gt, crowd)
    assert (want == 0).any() and (want > 0.5).any() and (want[:, crowd == 1] > 0).any()
    out = Guarded(ctx, (100, 40), np.float64)
    ddt, dgt, dcr = ctx.to_device(dt), ctx.to_device(gt), ctx.to_device(crowd)
    assert ctx.lib.odise_hip_box_iou(ctx.h, ddt.ptr, 100, dgt.ptr, 40, dcr.ptr, out.arr.ptr) == 0
    ctx.sync()
    got = out.read()
    bad = np.flatnonzero(got.view(np.uint64).reshape(-1) != want.view(np.uint64).reshape(-1))
    assert bad.size == 0, (bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])
    assert ctx.box_iou(dt, gt).numpy().tobytes() == IE.box_iou(dt, gt).tobytes()   # no crowds, through the binding
    for n, n_gt in ((0, 40), (100, 0)):
        fresh = Guarded(ctx, (100, 40), np.float64)
        assert ctx.lib.odise_hip_box_iou(ctx.h, ddt.ptr, n, dgt.ptr, n_gt, dcr.ptr, fresh.arr.ptr) == 0
        ctx.sync()
        fresh.read(intact=True)


# ---- instance_eval_bbox on crafted dense masks ----------------------------------------------------------------------------------------------
class Slots:
    """Guarded rows / n_rows of both tasks, the boxes and the flags of one call."""

    def __init__(self, ctx, topk):
        self.topk = topk
        self.bbox, self.segm = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (topk,), IE.ROW_DTYPE)
        self.n_bbox, self.n_segm = Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
        self.boxes = Guarded(ctx, (topk, 4), np.float32)
        self.flags = ctx.zeros((1,), np.int32)


def _eval_bbox(ctx, c, image, s, segm=True, gt=None, boxes=None, dtype=np.uint8):
    masks, table, scores = _pad_case(c, s.topk)
    if gt is None:
        gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    dgt = ctx.instance_gt_to_device(*gt, boxes=IE.gt_boxes(c["annotations"]) if boxes is None else boxes)
    ctx.instance_eval_bbox(masks.shape[1:], ctx.to_device(table), ctx.to_device(scores), s.topk, dgt, c["K"], image, s.bbox.arr, s.n_bbox.arr, s.flags,
                           *((s.segm.arr, s.n_segm.arr) if segm else (None, None)), boxes=s.boxes.arr, masks=ctx.to_device(masks.astype(dtype)))
    ctx.sync()
    return dgt, (masks, table, scores)


def _assert_rows(got, want):
    for field in IE.ROW_DTYPE.names:
        np.testing.assert_array_equal(got[field], want[field], err_msg=field)
    assert got.tobytes() == want.tobytes()


CASES = sorted(IC.matching_cases()) + ["ells", "random", "jittered", "no_gt"]


def _case(name):
    if name == "ells":
        return BC.ell_case()
    if name == "random":
        return BC.bbox_case(IC.random_case(n=100, n_gt=40, K=5))
    if name == "jittered":                                                  # fractional ground-truth boxes: IoUs that are no ratios of pixel counts
        return BC.bbox_case(IC.random_case(seed=6, n=60, n_gt=30, K=3), np.random.default_rng(2))
    if name == "no_gt":
        return BC.bbox_case(IC.random_case(seed=9, n=25, n_gt=0))
    return BC.bbox_case(IC.matching_cases()[name])


@pytest.mark.parametrize("name", CASES)
def test_bbox_rows_equal_the_host_loop_and_segm_rows_those_of_the_segm_call(ctx, name):
    c = _case(name)
    topk = 100 if name == "random" else len(c["masks"]) + 3                 # rows past n are zeroed
    s = Slots(ctx, topk)
    dgt, (masks, table, scores) = _eval_bbox(ctx, c, 17, s, dtype=np.float32 if name == "random" else np.uint8)
    want, n, f, _, _ = BC.want_rows(c, 17, topk, "bbox")
    assert f == 0 and int(s.flags.numpy()[0]) == 0 and int(s.n_bbox.read()[0]) == n == len(c["masks"]) == int(s.n_segm.read()[0])
    _assert_rows(s.bbox.read(), want)
    np.testing.assert_array_equal(s.boxes.read()[:n], IE.mask_boxes(c["masks"]))
    assert not s.boxes.read()[n:].any()
    # the segm rows of the same call: those of odise_hip_instance_eval_poly on the same inputs, and of the host loop
    alone, n_alone = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32)
    ctx.instance_eval(masks.shape[1:], ctx.to_device(table), ctx.to_device(scores), topk, dgt, c["K"], 17, alone.arr, n_alone.arr, s.flags,
                      masks=ctx.to_device(masks))
    ctx.sync()
    assert s.segm.read().tobytes() == alone.read().tobytes() == BC.want_rows(c, 17, topk, "segm")[0].tobytes()
    if name == "ells":
        assert s.segm.read()["matched"].tolist() != s.bbox.read()["matched"].tolist()
    # the bbox task alone: the same bbox rows, the segm outputs untouched
    t = Slots(ctx, topk)
    _eval_bbox(ctx, c, 17, t, segm=False)
    _assert_rows(t.bbox.read(), want)
    t.segm.read(intact=True)
    t.n_segm.read(intact=True)


def test_a_second_picture_leaves_the_first_rows_alone(ctx):
    a, b = BC.bbox_case(IC.random_case(seed=8, n=40, n_gt=20)), BC.bbox_case(IC.random_case(seed=9, n=25, n_gt=0))
    topk = 40
    buf = {t: ctx.zeros((2 * topk,), IE.ROW_DTYPE) for t in ("bbox", "segm")}
    counts, flags = {t: ctx.zeros((2,), np.int32) for t in ("bbox", "segm")}, ctx.zeros((1,), np.int32)
    for i, c in enumerate((a, b)):
        masks, table, scores = _pad_case(c, topk)
        dgt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])}), boxes=IE.gt_boxes(c["annotations"]))
        slot = lambda t: (buf[t].view((topk,), IE.ROW_DTYPE, i * topk * 32), counts[t].view((1,), np.int32, 4 * i))
        ctx.instance_eval_bbox((IC.H, IC.W), ctx.to_device(table), ctx.to_device(scores), topk, dgt, c["K"], i, *slot("bbox"), flags, *slot("segm"),
                               masks=ctx.to_device(masks))
        ctx.sync()
        if i == 0:
            first = {t: buf[t].numpy()[:topk].copy() for t in buf}
    for t in ("bbox", "segm"):
        host = buf[t].numpy()
        assert host[:topk].tobytes() == first[t].tobytes() == BC.want_rows(a, 0, topk, t)[0].tobytes()
        assert host[topk:].tobytes() == BC.want_rows(b, 1, topk, t)[0].tobytes()
        assert list(counts[t].numpy()) == [40, 25]
    assert int(flags.numpy()[0]) == 0


def test_flags_zero_the_rows_they_concern(ctx):
    """A NaN ground-truth box (4) and a class outside the categories (2) zero both tasks' rows; bad runs (1) zero the segm rows only."""
    c = BC.bbox_case(IC.random_case(seed=8, n=40, n_gt=20))
    topk = 40
    gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    nan_boxes = IE.gt_boxes(c["annotations"])
    nan_boxes[7, 3] = np.nan
    inf_boxes = IE.gt_boxes(c["annotations"])
    inf_boxes[0, 0] = np.inf
    runs = gt[1].copy()
    runs[3] += 1
    bad_cls = dict(c, classes=np.where(np.arange(40) == 5, c["K"], c["classes"]).astype(np.int32))
    want_bbox = BC.want_rows(c, 2, topk, "bbox")[0]
    for case, g, boxes, flag, bbox_lives in ((c, gt, nan_boxes, 4, False), (c, gt, inf_boxes, 4, False), (bad_cls, gt, None, 2, False),
                                             (c, (gt[0], runs, gt[2]), None, 1, True)):
        s = Slots(ctx, topk)
        _eval_bbox(ctx, case, 2, s, gt=g, boxes=boxes)
        assert int(s.flags.numpy()[0]) == flag, (flag, int(s.flags.numpy()[0]))
        assert int(s.n_segm.read()[0]) == 0 and not s.segm.read().view(np.uint8).any()
        if bbox_lives:
            assert int(s.n_bbox.read()[0]) == 40
            _assert_rows(s.bbox.read(), want_bbox)
        else:
            assert int(s.n_bbox.read()[0]) == 0 and not s.bbox.read().view(np.uint8).any()
    # the NaN box with the bbox task alone
    s = Slots(ctx, topk)
    _eval_bbox(ctx, c, 2, s, segm=False, boxes=nan_boxes)
    assert int(s.flags.numpy()[0]) == 4 and int(s.n_bbox.read()[0]) == 0 and not s.bbox.read().view(np.uint8).any()


def test_bad_arguments_write_nothing(ctx):
    c = BC.bbox_case(IC.matching_cases()["areas"])
    masks, table, scores = _pad_case(c, 101)
    gt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {0: 0}), boxes=IE.gt_boxes(c["annotations"]))
    s = Slots(ctx, 101)
    flags = Guarded(ctx, (1,), np.int32)
    dm, dt, ds = ctx.to_device(masks), ctx.to_device(table), ctx.to_device(scores)
    thr = np.ascontiguousarray(IE.IOU_THRS)

    def call(null_task=False, task_over=None, **over):
        d = InstEvalDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk = IC.H, IC.W, dm.ptr, U8, dt.ptr, ds.ptr, 2
        d.gt_runs, d.gt_offsets, d.gt_rows, d.n_gt, d.num_categories = gt["runs"].ptr, gt["offsets"].ptr, gt["rows"].ptr, 1, 1
        d.iou_thresholds, d.rows, d.n_rows, d.flags = thr.ctypes.data, s.segm.arr.ptr, s.n_segm.arr.ptr, flags.arr.ptr
        for k, v in over.items():
            setattr(d, k, v)
        t = InstBboxTask()
        t.gt_boxes, t.rows, t.n_rows, t.boxes = gt["boxes"].ptr, s.bbox.arr.ptr, s.n_bbox.arr.ptr, s.boxes.arr.ptr
        for k, v in (task_over or {}).items():
            setattr(t, k, v)
        rc = ctx.lib.odise_hip_instance_eval_bbox(ctx.h, C.byref(d), None, None if null_task else C.byref(t))
        return rc, ctx.lib.odise_hip_last_error().decode()

    for kw, word in (({"null_task": True}, "null"), ({"topk": 0}, "topk"), ({"topk": 101}, "topk"), ({"n_gt": 1025}, "ground-truth"),
                     ({"task_over": {"rows": None}}, "null"), ({"task_over": {"gt_boxes": None}}, "null"), ({"rows": None}, "null"),
                     ({"flags": None}, "null")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    ctx.sync()
    for o in (s.bbox, s.segm, s.n_bbox, s.n_segm, s.boxes, flags):
        o.read(intact=True)
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    assert call()[0] == 0                                                   # the same descriptor, valid
    ctx.sync()
    assert int(s.n_bbox.read()[0]) == 2 == int(s.n_segm.read()[0]) and int(flags.read()[0]) == 0


# ---- the small model: from the mask logits ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


@pytest.fixture(scope="module")
def forwards(small, ctx):
    """One forward per size with everything the tests below compare, computed once: the instances, the boxes and both tasks' rows from the
    mask logits (taken right behind the forward, while its selection is the resident one)."""
    hip, K = small, len(GROUPS)
    topk = int(hip.test_topk_per_image)
    out = {}
    hip.keep_instance_selection = True
    try:
        for h, w in ((512, 512), (500, 502)):                               # the x4 form, and the generic sampler
            inst = hip.forward([{"image": image_u8(h, w, seed=h + w)}])[0]["instances"]
            sel = hip.last_selection
            table, scores = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)
            boxes = ctx.instance_boxes((h, w), topk, table, b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0]).numpy()
            anns = BC.with_bbox(_annotations_from(inst["pred_masks"], inst["pred_classes"]), np.random.default_rng(h))
            gt = ctx.instance_gt_to_device(*IE.gt_rows(anns, {k: k for k in range(K)}), boxes=IE.gt_boxes(anns))
            rows = {t: ctx.zeros((topk,), IE.ROW_DTYPE) for t in ("bbox", "segm", "alone")}
            n_rows, flags = ctx.zeros((3,), np.int32), ctx.zeros((1,), np.int32)
            eval_boxes = ctx.zeros((topk, 4), np.float32)
            ctx.instance_eval_bbox((h, w), table, scores, topk, gt, K, 4, rows["bbox"], n_rows.view((1,), np.int32), flags, rows["segm"],
                                   n_rows.view((1,), np.int32, 4), boxes=eval_boxes, b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0])
            ctx.instance_eval((h, w), table, scores, topk, gt, K, 4, rows["alone"], n_rows.view((1,), np.int32, 8), flags, b=0, pad_hw=sel["pad_hw"],
                              img_hw=sel["img_hw"][0])
            out[(h, w)] = dict(inst=inst, anns=anns, boxes=boxes, eval_boxes=eval_boxes.numpy(), rows={t: r.numpy() for t, r in rows.items()},
                               n_rows=n_rows.numpy(), flags=int(flags.numpy()[0]), topk=topk)
    finally:
        hip.keep_instance_selection = False
    return out


@pytest.mark.parametrize("h,w", [(512, 512), (500, 502)])
def test_logits_path_boxes_and_rows_equal_the_dense_form(forwards, h, w):
    f, K = forwards[(h, w)], len(GROUPS)
    inst, topk = f["inst"], f["topk"]
    n = len(inst["scores"])
    masks = inst["pred_masks"] > 0.5                                        # odise_hip_instance_masks of the same selection
    want = np.zeros((topk, 4), np.float32)
    want[:n] = IE.mask_boxes(masks)
    assert n > 6 and want[:n].any()
    np.testing.assert_array_equal(f["boxes"], want)
    np.testing.assert_array_equal(f["eval_boxes"], want)
    assert list(f["n_rows"]) == [n, n, n] and f["flags"] == 0
    c = IC.case(list(masks.astype(np.uint8)), inst["scores"], inst["pred_classes"], f["anns"], K)
    assert f["rows"]["bbox"].tobytes() == BC.want_rows(c, 4, topk, "bbox")[0].tobytes()
    assert f["rows"]["segm"].tobytes() == f["rows"]["alone"].tobytes() == BC.want_rows(c, 4, topk, "segm")[0].tobytes()
    assert (f["rows"]["bbox"]["matched"] & ~f["rows"]["bbox"]["ignored"]).any()


def test_evaluator_end_to_end_with_both_tasks(small, ctx):
    """Three pictures through HipInstanceSegEvaluator(tasks=("bbox", "segm")); evaluate() equals the host route per task, and its segm group
    that of a segm-only evaluator fed the same pictures."""
    hip, K = small, len(GROUPS)
    names = [f"class{k}" for k in range(K)]
    ids = {100 + k: k for k in range(K)}
    both = HipInstanceSegEvaluator(ctx, ids, names, topk=int(hip.test_topk_per_image), tasks=("bbox", "segm"))
    segm = HipInstanceSegEvaluator(ctx, ids, names, topk=int(hip.test_topk_per_image))
    bbox = HipInstanceSegEvaluator(ctx, ids, names, topk=int(hip.test_topk_per_image), tasks=("bbox",))
    for ev in (both, segm, bbox):
        ev.CHUNK = 2                                                        # three pictures cross a block of the row buffer
        ev.reset()
    host_rows, npig = {"bbox": [], "segm": []}, np.zeros((K, 4), np.int64)
    hip.keep_instance_selection = True
    try:
        for i, (h, w) in enumerate(((512, 512), (320, 448), (500, 502))):
            inst = hip.forward([{"image": image_u8(h, w, seed=40 + i)}])[0]["instances"]
            anns = BC.with_bbox(_annotations_from(inst["pred_masks"], inst["pred_classes"], shift=2 + i), np.random.default_rng(i))
            c = IC.case(list((inst["pred_masks"] > 0.5).astype(np.uint8)), inst["scores"], inst["pred_classes"], anns, K)
            for t in host_rows:
                want, n, f, (table, _, _), _ = BC.want_rows(c, i, len(inst["scores"]), t)
                assert f == 0
                host_rows[t].append(want[:n])
            npig += IE.npig(table, K)
            for a in anns:
                a["category_id"] += 100                                     # dataset ids
            for ev in (both, segm, bbox):
                ev.process_selection(hip.last_selection, [anns], [i])
    finally:
        hip.keep_instance_selection = False
    got = both.evaluate()
    assert list(got) == ["bbox", "segm"]
    for t in ("bbox", "segm"):
        want = IE.results(*IE.accumulate(np.concatenate(host_rows[t]), npig, K), names)
        assert both.rows(t).tobytes() == np.concatenate(host_rows[t]).tobytes()
        assert set(got[t]) == set(want) and not math.isnan(got[t]["AP"]) and got[t]["AP"] > 0
        for k in want:
            assert got[t][k] == want[k] or (math.isnan(got[t][k]) and math.isnan(want[k])), (t, k)
    assert got["bbox"] != got["segm"]
    alone = segm.evaluate()
    assert set(alone) == set(got["segm"]) and "AP" in alone                 # the default: the flat group, as before
    for k in alone:
        assert alone[k] == got["segm"][k] or (math.isnan(alone[k]) and math.isnan(got["segm"][k])), k
    only = bbox.evaluate()
    assert list(only) == ["bbox"] and bbox.rows().tobytes() == both.rows("bbox").tobytes()
    for k in only["bbox"]:
        assert only["bbox"][k] == got["bbox"][k] or (math.isnan(only["bbox"][k]) and math.isnan(got["bbox"][k])), k


def test_the_model_switch_fills_pred_boxes(small):
    hip = small
    img = [{"image": image_u8(320, 448, seed=3)}]
    plain = hip.forward(img)[0]["instances"]
    assert plain["pred_boxes"].shape == (len(plain["scores"]), 4) and plain["pred_boxes"].dtype == np.float32 and not plain["pred_boxes"].any()
    hip.instance_boxes = True
    try:
        boxed = hip.forward(img)[0]["instances"]
    finally:
        hip.instance_boxes = False
    assert len(boxed["scores"]) > 6
    np.testing.assert_array_equal(boxed["pred_boxes"], IE.mask_boxes(boxed["pred_masks"] > 0.5))
    assert boxed["pred_boxes"].any()
    for k in ("pred_masks", "scores", "pred_classes", "query_index"):
        np.testing.assert_array_equal(boxed[k], plain[k])
