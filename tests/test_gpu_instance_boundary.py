"""Boundary AP for instance masks on the device (odise_amd/csrc/inst_boundary.hip, inst_eval.hip): `odise_hip_mask_boundary`,
`odise_hip_mask_boundary_iou` and `odise_hip_instance_eval_boundary` against the host restatement (odise_amd/instance_eval.py, itself pinned
by tests/test_instance_boundary_cpu.py) - bytes equal, integers equal, doubles bit for bit, rows byte for byte - on crafted masks, on the
small model's mask logits, and `HipInstanceSegEvaluator(tasks=("bbox", "segm", "boundary"))` end to end."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import inst_bbox_cases as BC
import inst_cases as IC
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE
from odise_amd._lib import F32, U8, InstBboxTask, InstBoundaryTask, InstEvalDesc
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator
from small_model import GROUPS, build_small, image_u8
from test_gpu_instance_eval import Guarded, _annotations_from, _pad_case
from test_instance_boundary_cpu import SIZES, edge_masks, radii

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


# ---- mask_boundary ------------------------------------------------------------------------------------------------------------------------
def _boundary(ctx, masks, r):
    out, area = Guarded(ctx, masks.shape, np.uint8), Guarded(ctx, (len(masks),), np.int64)
    dev = ctx.to_device(masks)
    rc = ctx.lib.odise_hip_mask_boundary(ctx.h, dev.ptr, F32 if masks.dtype == np.float32 else U8, len(masks), masks.shape[1], masks.shape[2], r,
                                         out.arr.ptr, area.arr.ptr)
    assert rc == 0, ctx.lib.odise_hip_last_error()
    ctx.sync()
    return out.read(), area.read()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("h,w", SIZES)
def test_mask_boundary_is_byte_equal_to_the_host(ctx, h, w, dtype):
    """A single word, a word edge at 63 / 64 / 65 rows, r a multiple of 64, r >= 64 with R >= 3 (130 and 200 rows), fewer columns than the
    window, both sides of "everything erodes", masks that touch all four picture edges."""
    ms = edge_masks(h, w)
    ms = ms if dtype == np.uint8 else ms.astype(np.float32) * np.float32(0.75)
    for r in [0] + radii(h, w):
        want = IE.mask_boundary(ms, r)
        got, area = _boundary(ctx, ms, r)
        np.testing.assert_array_equal(got, want, err_msg=f"r {r}")
        np.testing.assert_array_equal(area, want.reshape(len(ms), -1).sum(1))


def test_mask_boundary_binding_and_bad_arguments(ctx):
    ms = edge_masks(70, 40)
    dev = ctx.to_device(ms)
    np.testing.assert_array_equal(ctx.mask_boundary(dev).numpy(), IE.mask_boundary(ms))
    b, area = ctx.mask_boundary(ctx.to_device(ms.astype(bool)), radius=3, with_area=True)
    np.testing.assert_array_equal(b.numpy(), IE.mask_boundary(ms, 3))
    np.testing.assert_array_equal(area.numpy(), IE.mask_boundary(ms, 3).reshape(len(ms), -1).sum(1))
    out = Guarded(ctx, ms.shape, np.uint8)
    for args, word in (((dev.ptr, U8, -1, 70, 40, 0, out.arr.ptr, None), "masks"), ((dev.ptr, U8, 3, 0, 40, 0, out.arr.ptr, None), "size"),
                       ((dev.ptr, 0, 3, 70, 40, 0, out.arr.ptr, None), "dtype"), ((None, U8, 3, 70, 40, 0, out.arr.ptr, None), "null"),
                       ((dev.ptr, U8, 3, 70, 40, 0, None, None), "null")):
        assert ctx.lib.odise_hip_mask_boundary(ctx.h, *args) != 0 and word in ctx.lib.odise_hip_last_error().decode(), args
    assert ctx.lib.odise_hip_mask_boundary(ctx.h, dev.ptr, U8, 0, 70, 40, 0, out.arr.ptr, None) == 0    # n == 0 writes nothing
    ctx.sync()
    out.read(intact=True)


# ---- mask_boundary_iou --------------------------------------------------------------------------------------------------------------------
def _boundary_iou(ctx, masks, counts, iscrowd, r, n=None, n_gt=None):
    n, n_gt = len(masks) if n is None else n, len(counts) if n_gt is None else n_gt
    h, w = masks.shape[1:]
    gt = ctx.instance_gt_to_device(np.zeros((len(counts), 3), np.int32), np.concatenate([np.asarray(c, np.uint32) for c in counts] + [np.zeros(0, np.uint32)]),
                                   np.concatenate(([0], np.cumsum([len(c) for c in counts]))).astype(np.int64))
    crowd = ctx.to_device(np.asarray(iscrowd, np.uint8)) if iscrowd is not None else None
    shape = (max(n, 1), max(n_gt, 1))
    out = [Guarded(ctx, shape, np.float64), Guarded(ctx, shape, np.float64), Guarded(ctx, shape, np.float64), Guarded(ctx, shape, np.int32),
           Guarded(ctx, (max(n, 1),), np.int64), Guarded(ctx, (max(n_gt, 1),), np.int64), Guarded(ctx, (1,), np.int32)]
    if n and n_gt:
        ctx.lib.odise_hip_memset(ctx.h, out[6].arr.ptr, 0, 4)
    dev = ctx.to_device(masks)
    rc = ctx.lib.odise_hip_mask_boundary_iou(ctx.h, dev.ptr, F32 if masks.dtype == np.float32 else U8, n, h, w, gt["runs"].ptr, gt["offsets"].ptr, n_gt,
                                             crowd.ptr if crowd is not None else None, r, *[o.arr.ptr for o in out])
    assert rc == 0, ctx.lib.odise_hip_last_error()
    ctx.sync()
    return out


def _check_boundary_iou(ctx, masks, counts, iscrowd=None, r=0, flag=0):
    iou, m_iou, b_iou, inter, area_d, area_g, flags = (o.read() for o in _boundary_iou(ctx, masks, counts, iscrowd, r))
    h, w = masks.shape[1:]
    want = IE.boundary_iou(masks, counts, iscrowd, r)
    for got, ref, what in zip((iou, m_iou, b_iou), want, ("iou", "mask_iou", "boundary_iou")):
        assert got.tobytes() == ref.tobytes(), (what, np.abs(got - ref).max())
    d = masks != 0
    g = np.stack([IE.decode_runs(c, h, w) for c in counts]).astype(bool)
    np.testing.assert_array_equal(inter, np.stack([(di.reshape(1, -1) & g.reshape(len(g), -1)).sum(1) for di in d]))
    np.testing.assert_array_equal(area_d, d.reshape(len(d), -1).sum(1))
    np.testing.assert_array_equal(area_g, g.reshape(len(g), -1).sum(1))
    assert int(flags[0]) == flag
    return want


@pytest.mark.parametrize("h,w", [(63, 5), (65, 5), (130, 1), (200, 300)])
def test_mask_boundary_iou_is_bit_equal_to_the_host_loop(ctx, h, w):
    ms = edge_masks(h, w)
    counts = [R.mask_counts(m) for m in ms]
    crowd = [k % 3 == 1 for k in range(len(ms))]
    want = _check_boundary_iou(ctx, ms, counts, crowd)
    if (h, w) == (200, 300):
        assert (want[2] > 0).any() and (want[2] < want[1]).any() and (want[0] == want[2]).any()
    _check_boundary_iou(ctx, ms.astype(np.float32) * np.float32(0.75), [IC.with_zero_runs(c, k) for k, c in enumerate(counts)], None, 2)
    # the binding
    iou, m_iou, b_iou, flags = ctx.mask_boundary_iou(ctx.to_device(ms), counts, crowd, radius=1)
    ref = IE.boundary_iou(ms, counts, crowd, 1)
    assert iou.numpy().tobytes() == ref[0].tobytes() and m_iou.numpy().tobytes() == ref[1].tobytes() and b_iou.numpy().tobytes() == ref[2].tobytes()
    assert int(flags.numpy()[0]) == 0


def test_mask_boundary_iou_flag_1_and_empty_sides(ctx):
    h, w = 65, 5
    ms = edge_masks(h, w)
    counts = [R.mask_counts(m).copy() for m in ms]
    counts[7][len(counts[7]) // 2] += 7                                      # the blobs: their runs no longer sum to h * w
    _check_boundary_iou(ctx, ms, counts, flag=IE.FLAG_BAD_RUNS)
    counts = [R.mask_counts(m) for m in ms]
    for n, n_gt in ((0, 3), (3, 0)):
        for o in _boundary_iou(ctx, ms[:3], counts[:3], None, 0, n, n_gt):
            o.read(intact=True)


# ---- instance_eval_boundary on crafted dense masks ------------------------------------------------------------------------------------------
class Slots:
    """Guarded rows / n_rows of the three tasks and the flags of one call."""

    def __init__(self, ctx, topk):
        self.topk = topk
        self.rows = {t: Guarded(ctx, (topk,), IE.ROW_DTYPE) for t in ("bbox", "segm", "boundary")}
        self.n = {t: Guarded(ctx, (1,), np.int32) for t in ("bbox", "segm", "boundary")}
        self.flags = ctx.zeros((1,), np.int32)


def want_rows(c, image, topk, iou_type, radius=None, polygons=False):
    gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    table, runs, offs = gt
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"], iou_type=iou_type,
                                gt_boxes=IE.gt_boxes(c["annotations"]) if iou_type == "bbox" else None, radius=radius)
    full = np.zeros(topk, IE.ROW_DTYPE)
    full[:len(rows)] = rows
    return full, len(rows), flags


def _eval(ctx, c, image, s, tasks=("bbox", "segm", "boundary"), gt=None, radius=0, dtype=np.uint8, masks=None):
    padded, table, scores = _pad_case(c, s.topk)
    if gt is None:
        gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    dgt = ctx.instance_gt_to_device(*gt, boxes=IE.gt_boxes(c["annotations"]) if "bbox" in tasks else None)
    dev = ctx.to_device((padded if masks is None else masks).astype(dtype))
    segm = (s.rows["segm"].arr, s.n["segm"].arr) if "segm" in tasks else (None, None)
    boundary = (s.rows["boundary"].arr, s.n["boundary"].arr, radius) if "boundary" in tasks else None
    if "bbox" in tasks:
        ctx.instance_eval_bbox(padded.shape[1:], ctx.to_device(table), ctx.to_device(scores), s.topk, dgt, c["K"], image, s.rows["bbox"].arr, s.n["bbox"].arr,
                               s.flags, *segm, masks=dev, boundary=boundary)
    else:
        ctx.instance_eval(padded.shape[1:], ctx.to_device(table), ctx.to_device(scores), s.topk, dgt, c["K"], image, *segm, s.flags, masks=dev,
                          boundary=boundary)
    ctx.sync()


def _shifted_case():
    return BC.bbox_case(IC.case([IC.rect(10, 50, 14, 54, 64, 64)], [.9], [0], [IC.ann(IC.rect(10, 50, 10, 50, 64, 64))]))


def _case(name):
    if name == "ells":
        return BC.ell_case()
    if name == "random":
        return BC.bbox_case(IC.random_case(n=100, n_gt=40, K=5))
    if name == "no_gt":
        return BC.bbox_case(IC.random_case(seed=9, n=25, n_gt=0))
    if name == "shifted":
        return _shifted_case()
    return BC.bbox_case(IC.matching_cases()[name])


CASES = sorted(IC.matching_cases()) + ["ells", "random", "no_gt", "shifted"]


@pytest.mark.parametrize("name", CASES)
def test_boundary_rows_equal_the_host_loop_and_the_other_rows_those_of_the_bbox_call(ctx, name):
    c = _case(name)
    topk = 100 if name == "random" else len(c["masks"]) + 3                 # rows past n are zeroed
    s = Slots(ctx, topk)
    _eval(ctx, c, 17, s, dtype=np.float32 if name == "random" else np.uint8)
    want, n, f = want_rows(c, 17, topk, "boundary")
    assert f == 0 and int(s.flags.numpy()[0]) == 0 and all(int(s.n[t].read()[0]) == n == len(c["masks"]) for t in s.n)
    assert s.rows["boundary"].read().tobytes() == want.tobytes()
    # segm and bbox rows of the same call: byte-equal to those of odise_hip_instance_eval_bbox alone
    two = Slots(ctx, topk)
    _eval(ctx, c, 17, two, tasks=("bbox", "segm"))
    for t in ("bbox", "segm"):
        assert s.rows[t].read().tobytes() == two.rows[t].read().tobytes() == want_rows(c, 17, topk, t)[0].tobytes(), t
    two.rows["boundary"].read(intact=True)
    # the boundary task alone, with a radius of its own: the same walk, the other outputs untouched
    one = Slots(ctx, topk)
    _eval(ctx, c, 17, one, tasks=("boundary",), radius=5)
    assert one.rows["boundary"].read().tobytes() == want_rows(c, 17, topk, "boundary", 5)[0].tobytes()
    for t in ("bbox", "segm"):
        one.rows[t].read(intact=True)
        one.n[t].read(intact=True)
    if name == "shifted":
        assert IC.bits(s.rows["segm"].read()["matched"][0], 0) == [1] * 7 + [0] * 3 and int(s.rows["boundary"].read()["matched"][0]) == 0


def test_polygon_ground_truth(ctx):
    """Two ground truths as polygons, one crowd as runs: the boundary rows equal the host loop on the rasterised masks."""
    from odise_amd import coco_poly
    h, w = IC.H, IC.W
    polys = [[[10.0, 10.0, 40.0, 12.0, 38.0, 50.0, 8.0, 45.0]], [[50.5, 20.5, 75.0, 20.5, 75.0, 60.0, 50.5, 60.0], [52.0, 70.0, 70.0, 70.0, 60.0, 90.0]]]
    gms = [IE.decode_runs(coco_poly.annotation_to_counts(p, h, w), h, w) for p in polys]
    crowd = IC.rect(0, 30, 40, 80)
    anns_poly = [{"category_id": 0, "iscrowd": 0, "area": float(m.sum()), "segmentation": p} for m, p in zip(gms, polys)] + [IC.ann(crowd, iscrowd=1)]
    anns_rle = [IC.ann(m) for m in gms] + [IC.ann(crowd, iscrowd=1)]
    # the first ground truth's own mask: matched in both tasks; the second one shifted by three rows: matched in segm alone
    dets = [gms[0], np.roll(gms[1], -3, axis=0), gms[0] & IC.rect(0, 96, 0, 30), IC.rect(5, 20, 45, 70)]
    c = IC.case(dets, [.9, .8, .7, .6], [0, 0, 0, 0], anns_rle)
    topk = 6
    s = Slots(ctx, topk)
    gt = IE.gt_rows(anns_poly, {0: 0}, polygons=True, hw=(h, w))
    _eval(ctx, c, 5, s, tasks=("segm", "boundary"), gt=gt)
    assert int(s.flags.numpy()[0]) == 0
    for t in ("segm", "boundary"):
        want, n, f = want_rows(c, 5, topk, t)
        assert f == 0 and int(s.n[t].read()[0]) == n == 4
        assert s.rows[t].read().tobytes() == want.tobytes(), t
    assert s.rows["boundary"].read()["matched"].any() and s.rows["boundary"].read()["matched"].tolist() != s.rows["segm"].read()["matched"].tolist()


def test_a_second_picture_leaves_the_first_rows_alone(ctx):
    a, b = IC.random_case(seed=8, n=40, n_gt=20), IC.random_case(seed=9, n=25, n_gt=0)
    topk = 40
    buf, counts, flags = ctx.zeros((2 * topk,), IE.ROW_DTYPE), ctx.zeros((2,), np.int32), ctx.zeros((1,), np.int32)
    for i, c in enumerate((a, b)):
        masks, table, scores = _pad_case(c, topk)
        dgt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])}))
        ctx.instance_eval((IC.H, IC.W), ctx.to_device(table), ctx.to_device(scores), topk, dgt, c["K"], i, None, None, flags, masks=ctx.to_device(masks),
                          boundary=(buf.view((topk,), IE.ROW_DTYPE, i * topk * 32), counts.view((1,), np.int32, 4 * i)))
        ctx.sync()
        if i == 0:
            first = buf.numpy()[:topk].copy()
    host = buf.numpy()
    assert host[:topk].tobytes() == first.tobytes() == want_rows(a, 0, topk, "boundary")[0].tobytes()
    assert host[topk:].tobytes() == want_rows(b, 1, topk, "boundary")[0].tobytes()
    assert list(counts.numpy()) == [40, 25] and int(flags.numpy()[0]) == 0


def test_flags_zero_the_rows_they_concern(ctx):
    """Bad runs (1), a class outside the categories (2), a bad ground-truth category (4) and a bad polygon (8) zero the boundary rows as they
    zero the segm rows; bad runs leave the bbox rows alive."""
    c = BC.bbox_case(IC.random_case(seed=8, n=40, n_gt=20))
    topk = 40
    gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    runs = gt[1].copy()
    runs[3] += 1
    bad_cls = dict(c, classes=np.where(np.arange(40) == 5, c["K"], c["classes"]).astype(np.int32))
    bad_cat = gt[0].copy()
    bad_cat[2, 0] = c["K"]
    want_bbox = want_rows(c, 2, topk, "bbox")[0]
    for case, g, flag, bbox_lives in ((c, (gt[0], runs, gt[2]), 1, True), (bad_cls, gt, 2, False), (c, (bad_cat, gt[1], gt[2]), 4, False)):
        s = Slots(ctx, topk)
        _eval(ctx, case, 2, s, gt=g)
        assert int(s.flags.numpy()[0]) == flag, (flag, int(s.flags.numpy()[0]))
        for t in ("segm", "boundary"):
            assert int(s.n[t].read()[0]) == 0 and not s.rows[t].read().view(np.uint8).any(), (flag, t)
        if bbox_lives:
            assert int(s.n["bbox"].read()[0]) == 40 and s.rows["bbox"].read().tobytes() == want_bbox.tobytes()
        else:
            assert int(s.n["bbox"].read()[0]) == 0 and not s.rows["bbox"].read().view(np.uint8).any()
        # the boundary task alone finds the same flag
        s = Slots(ctx, topk)
        _eval(ctx, case, 2, s, tasks=("boundary",), gt=g)
        assert int(s.flags.numpy()[0]) == flag and int(s.n["boundary"].read()[0]) == 0 and not s.rows["boundary"].read().view(np.uint8).any()
    # a polygon of two vertices: flag 8
    anns = [{"category_id": 0, "iscrowd": 0, "area": 100.0, "segmentation": [[10.0, 10.0, 40.0, 12.0, 38.0, 50.0]]}]
    g = list(IE.gt_rows(anns, {0: 0}, polygons=True, hw=(IC.H, IC.W)))
    g[4] = np.asarray([0, 2], np.int64)                                      # poly_offsets: the polygon keeps two vertices
    g[3] = g[3][:4]
    one = IC.case([IC.rect(10, 50, 10, 40)], [.9], [0], anns)
    s = Slots(ctx, 3)
    _eval(ctx, one, 2, s, tasks=("segm", "boundary"), gt=tuple(g))
    assert int(s.flags.numpy()[0]) == 8
    for t in ("segm", "boundary"):
        assert int(s.n[t].read()[0]) == 0 and not s.rows[t].read().view(np.uint8).any()


def test_bad_arguments_write_nothing(ctx):
    c = BC.bbox_case(IC.matching_cases()["areas"])
    masks, table, scores = _pad_case(c, 101)
    gt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {0: 0}), boxes=IE.gt_boxes(c["annotations"]))
    s = Slots(ctx, 101)
    flags = Guarded(ctx, (1,), np.int32)
    dm, dt, ds = ctx.to_device(masks), ctx.to_device(table), ctx.to_device(scores)
    thr = np.ascontiguousarray(IE.IOU_THRS)

    def call(task_over=None, bbox=True, **over):
        d = InstEvalDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk = IC.H, IC.W, dm.ptr, U8, dt.ptr, ds.ptr, 2
        d.gt_runs, d.gt_offsets, d.gt_rows, d.n_gt, d.num_categories = gt["runs"].ptr, gt["offsets"].ptr, gt["rows"].ptr, 1, 1
        d.iou_thresholds, d.rows, d.n_rows, d.flags = thr.ctypes.data, s.rows["segm"].arr.ptr, s.n["segm"].arr.ptr, flags.arr.ptr
        for k, v in over.items():
            setattr(d, k, v)
        t = InstBboxTask()
        t.gt_boxes, t.rows, t.n_rows = gt["boxes"].ptr, s.rows["bbox"].arr.ptr, s.n["bbox"].arr.ptr
        bd = InstBoundaryTask()
        bd.radius, bd.rows, bd.n_rows = 0, s.rows["boundary"].arr.ptr, s.n["boundary"].arr.ptr
        for k, v in (task_over or {}).items():
            setattr(bd, k, v)
        rc = ctx.lib.odise_hip_instance_eval_boundary(ctx.h, C.byref(d), None, C.byref(t) if bbox else None, C.byref(bd))
        return rc, ctx.lib.odise_hip_last_error().decode()

    for kw, word in (({"task_over": {"rows": None}}, "null boundary"), ({"task_over": {"n_rows": None}}, "null boundary"), ({"topk": 0}, "topk"),
                     ({"topk": 101}, "topk"), ({"n_gt": 1025}, "ground-truth"), ({"rows": None}, "null"), ({"flags": None}, "null"),
                     ({"gt_runs": None, "rows": None, "n_rows": None, "bbox": False}, "null ground truth"), ({"h": 0}, "size")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    ctx.sync()
    for o in list(s.rows.values()) + list(s.n.values()) + [flags]:
        o.read(intact=True)
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    assert call()[0] == 0                                                   # the same descriptor, valid
    ctx.sync()
    assert all(int(s.n[t].read()[0]) == 2 for t in s.n) and int(flags.read()[0]) == 0


def test_rows_past_the_count_are_zeros_and_their_masks_are_not_read(ctx):
    """topk = 100 with a count of 3: the other 97 masks are all ones - read, they would share boundary pixels with every ground truth and
    their rows would not be zeros - and the rows equal those of the three masks alone."""
    c = IC.matching_cases()["two_on_one"]
    c = IC.case(list(c["masks"]) + [IC.rect(40, 70, 30, 60)], [.9, .8, .7], [0, 0, 0], c["annotations"] + [IC.ann(IC.rect(41, 70, 30, 61))])
    topk = 100
    padded, _, _ = _pad_case(c, topk)
    padded[3:] = 1
    s = Slots(ctx, topk)
    _eval(ctx, c, 9, s, tasks=("segm", "boundary"), masks=padded)
    for t in ("segm", "boundary"):
        want, n, f = want_rows(c, 9, topk, t)
        got = s.rows[t].read()
        assert n == 3 == int(s.n[t].read()[0]) and got.tobytes() == want.tobytes() and not got[3:].view(np.uint8).any()
    assert s.rows["boundary"].read()["matched"].any()


# ---- the small model: from the mask logits ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


@pytest.mark.parametrize("h,w", [(512, 512),      # x4 form
                                 (500, 502)])     # ragged: the generic sampler
def test_logits_path_equals_the_dense_form(small, ctx, h, w):
    hip, K = small, len(GROUPS)
    topk = int(hip.test_topk_per_image)
    hip.keep_instance_selection = True
    try:
        inst = hip.forward([{"image": image_u8(h, w, seed=h + w)}])[0]["instances"]
        sel = hip.last_selection
        table, scores = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)
        anns = _annotations_from(inst["pred_masks"], inst["pred_classes"])
        gt = ctx.instance_gt_to_device(*IE.gt_rows(anns, {k: k for k in range(K)}))
        rows = {t: ctx.zeros((topk,), IE.ROW_DTYPE) for t in ("segm", "boundary", "dense")}
        n_rows, flags = ctx.zeros((3,), np.int32), ctx.zeros((1,), np.int32)
        ctx.instance_eval((h, w), table, scores, topk, gt, K, 4, rows["segm"], n_rows.view((1,), np.int32), flags, b=0, pad_hw=sel["pad_hw"],
                          img_hw=sel["img_hw"][0], boundary=(rows["boundary"], n_rows.view((1,), np.int32, 4)))
        n = len(inst["scores"])
        dense = np.zeros((topk, h, w), np.uint8)
        dense[:n] = inst["pred_masks"] > 0.5
        ctx.instance_eval((h, w), table, scores, topk, gt, K, 4, None, None, flags, masks=ctx.to_device(dense),
                          boundary=(rows["dense"], n_rows.view((1,), np.int32, 8)))
        ctx.sync()
    finally:
        hip.keep_instance_selection = False
    assert n > 6 and list(n_rows.numpy()) == [n, n, n] and int(flags.numpy()[0]) == 0
    got = rows["boundary"].numpy()
    assert got.tobytes() == rows["dense"].numpy().tobytes()
    c = IC.case(list(dense[:n]), inst["scores"], inst["pred_classes"], anns, K)
    assert got.tobytes() == want_rows(c, 4, topk, "boundary")[0].tobytes()
    assert rows["segm"].numpy().tobytes() == want_rows(c, 4, topk, "segm")[0].tobytes()
    assert (got["matched"] & ~got["ignored"]).any()


def test_evaluator_end_to_end_with_three_tasks(small, ctx):
    """Three pictures through HipInstanceSegEvaluator(tasks=("bbox", "segm", "boundary")); evaluate() equals the host route per task, with the
    device accumulation and with the host one, and a boundary-only evaluator gives the same boundary group."""
    hip, K = small, len(GROUPS)
    names = [f"class{k}" for k in range(K)]
    ids = {100 + k: k for k in range(K)}
    topk = int(hip.test_topk_per_image)
    three = HipInstanceSegEvaluator(ctx, ids, names, topk=topk, tasks=("boundary", "bbox", "segm"))
    only = HipInstanceSegEvaluator(ctx, ids, names, topk=topk, tasks=("boundary",))
    assert three.tasks == ("bbox", "segm", "boundary") and only.tasks == ("boundary",)
    for ev in (three, only):
        ev.CHUNK = 2                                                        # three pictures cross a block of the row buffer
        ev.reset()
    assert three._chunks is three._task_chunks["segm"]
    host_rows, npig = {t: [] for t in three.tasks}, np.zeros((K, 4), np.int64)
    hip.keep_instance_selection = True
    try:
        for i, (h, w) in enumerate(((512, 512), (320, 448), (500, 502))):
            inst = hip.forward([{"image": image_u8(h, w, seed=40 + i)}])[0]["instances"]
            anns = BC.with_bbox(_annotations_from(inst["pred_masks"], inst["pred_classes"], shift=2 + i), np.random.default_rng(i))
            c = IC.case(list((inst["pred_masks"] > 0.5).astype(np.uint8)), inst["scores"], inst["pred_classes"], anns, K)
            for t in host_rows:
                want, n, f = want_rows(c, i, len(inst["scores"]), t)
                assert f == 0
                host_rows[t].append(want[:n])
            npig += IE.npig(IE.gt_rows(anns, {k: k for k in range(K)})[0], K)
            for a in anns:
                a["category_id"] += 100                                     # dataset ids
            for ev in (three, only):
                ev.process_selection(hip.last_selection, [anns], [i])
    finally:
        hip.keep_instance_selection = False
    for where in ("device", "host"):
        got = three.evaluate(accumulate_on=where)
        assert list(got) == ["bbox", "segm", "boundary"]
        for t in got:
            want = IE.results(*IE.accumulate(np.concatenate(host_rows[t]), npig, K), names)
            assert three.rows(t).tobytes() == np.concatenate(host_rows[t]).tobytes()
            assert set(got[t]) == set(want) and not math.isnan(got[t]["AP"]) and got[t]["AP"] > 0
            for k in want:
                assert got[t][k] == want[k] or (math.isnan(got[t][k]) and math.isnan(want[k])), (where, t, k)
    assert got["boundary"] != got["segm"]
    alone = only.evaluate()
    assert list(alone) == ["boundary"] and only.rows().tobytes() == three.rows("boundary").tobytes()
    for k in alone["boundary"]:
        assert alone["boundary"][k] == got["boundary"][k] or (math.isnan(alone["boundary"][k]) and math.isnan(got["boundary"][k])), k
