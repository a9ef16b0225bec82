"""Polygon annotations on the device (odise_amd/csrc/poly.hip): `odise_hip_polygon_rle` against the host restatement of maskApi.c rleFrPoly
(odise_amd/coco_poly.py, pinned by tests/test_polygon_cpu.py) - strings byte for byte, areas equal - and `odise_hip_instance_eval_poly`
against the host loop and against the run-length form of the same pictures, rows byte for byte.  No tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import inst_cases as IC
import poly_cases as PC
from odise_amd import coco_poly as P
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE
from odise_amd._lib import U8, InstEvalDesc, InstPolyGt
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xA5, 256


class Guarded:
    """A device output with canary bytes around it."""

    def __init__(self, ctx, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = ctx.to_device(np.full(self.nbytes + 2 * PAD, CANARY, np.uint8))
        self.arr = self.buf.view(shape, dtype, PAD)

    def read(self, intact=False):
        raw = self.buf.numpy()
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + self.nbytes:] == CANARY).all(), "canary overwritten"
        if intact:
            assert (raw == CANARY).all(), "output written"
        return self.arr.numpy()


def _raw_polygon_rle(ctx, xy, poly_offsets, ann_polys, h, w, capacity):
    """odise_hip_polygon_rle through guarded outputs -> (bytes, offsets, area, flags)"""
    n, n_poly = len(ann_polys) - 1, len(poly_offsets) - 1
    d_xy = ctx.to_device(np.asarray(xy, np.float64).reshape(-1)) if len(xy) else ctx.zeros((2,), np.float64)
    d_off, d_ann = ctx.to_device(np.asarray(poly_offsets, np.int64)), ctx.to_device(np.asarray(ann_polys, np.int32))
    out = [Guarded(ctx, (max(capacity, 1),), np.uint8), Guarded(ctx, (n + 1,), np.int64), Guarded(ctx, (max(n, 1),), np.int64), Guarded(ctx, (1,), np.int32)]
    ctx.lib.odise_hip_memset(ctx.h, out[3].arr.ptr, 0, 4)
    rc = ctx.lib.odise_hip_polygon_rle(ctx.h, d_xy.ptr, d_off.ptr, d_ann.ptr, n, n_poly, h, w, out[0].arr.ptr, capacity, out[1].arr.ptr, out[2].arr.ptr,
                                       out[3].arr.ptr)
    assert rc == 0, ctx.lib.odise_hip_last_error()
    ctx.sync()
    return out


# ---- polygon_rle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", PC.SIZES)
def test_polygon_rle_equals_the_host_on_the_case_set(ctx, h, w):
    anns = PC.annotations(h, w)
    _, strings, areas = PC.reference(h, w)
    rles, area = ctx.polygon_rle(anns, (h, w))
    assert [r["counts"] for r in rles] == strings
    assert all(r["size"] == [h, w] for r in rles) and list(area) == areas


def test_polygon_rle_equals_the_host_on_2000_random_polygons_in_one_call(ctx):
    h, w = PC.RANDOM_HW
    _, strings, areas = PC.reference(h, w, random=True)
    rles, area = ctx.polygon_rle(PC.random_annotations(), (h, w))
    assert len(rles) == PC.RANDOM_N and [r["counts"] for r in rles] == strings and list(area) == areas


def test_a_small_capacity_completes_the_offsets_and_writes_no_string(ctx):
    h, w = 70, 45
    anns = PC.annotations(h, w)
    _, strings, areas = PC.reference(h, w)
    xy, offs, ann = P.pack_polygons(anns)
    total = sum(len(s) for s in strings)
    want_off = np.concatenate(([0], np.cumsum([len(s) for s in strings])))
    for cap in (0, total - 1):
        buf, off, area, flags = _raw_polygon_rle(ctx, xy, offs, ann, h, w, cap)
        np.testing.assert_array_equal(off.read(), want_off)
        np.testing.assert_array_equal(area.read(), areas)
        buf.read(intact=True)
        assert int(flags.read()[0]) == 0
    buf, off, area, flags = _raw_polygon_rle(ctx, xy, offs, ann, h, w, total)
    assert buf.read().tobytes().decode("ascii") == "".join(strings)


@pytest.mark.parametrize("bad", ["two_vertices", "nan", "1e9"])
def test_a_bad_polygon_raises_flag_8_and_stays_inside(ctx, bad):
    h, w = 70, 45
    good = PC.shapes(h, w)
    polys = [good["tri_skew"], {"two_vertices": [3.0, 4.0, 20.0, 30.0], "nan": [3.0, 4.0, float("nan"), 30.0, 10.0, 40.0],
                                "1e9": [3.0, 4.0, 1e9, 30.0, 10.0, 40.0]}[bad], good["bow_tie"]]
    xy = np.concatenate([np.asarray(p, np.float64) for p in polys])
    offs = np.concatenate(([0], np.cumsum([len(p) // 2 for p in polys])))
    want = [R.counts_to_string(P.polygon_counts(polys[k], h, w)) for k in (0, 2)]
    buf, off, area, flags = _raw_polygon_rle(ctx, xy, offs, [0, 1, 2, 3], h, w, 4096)
    assert int(flags.read()[0]) == IE.FLAG_BAD_POLYGON
    o, raw = off.read(), buf.read().tobytes()
    area.read()
    assert raw[o[0]:o[1]].decode() == want[0] and raw[o[2]:o[3]].decode() == want[1]      # the neighbours are what they always are
    assert raw[o[1]:o[2]].decode() == R.counts_to_string([h * w])                        # the bad one contributes nothing


# ---- instance_eval_poly -------------------------------------------------------------------------------------------------------------------
def _pad_case(c, topk):
    n = len(c["masks"])
    masks = np.zeros((topk,) + c["masks"].shape[1:], np.uint8)
    masks[:n] = c["masks"]
    table = np.zeros(1 + 2 * topk, np.int32)
    table[0] = n
    table[1 + topk:1 + topk + n] = c["classes"]
    scores = np.zeros(topk, np.float32)
    scores[:n] = c["scores"]
    return masks, table, scores


def _box(mask):
    ys, xs = np.nonzero(mask)
    return int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1


def _as_polygons(anns, keep_crowds=True):
    """The rectangle annotations of inst_cases with the segmentation as a polygon (crowds stay RLE, as in COCO); the polygon decodes to
    exactly the annotation's mask - asserted here on the host."""
    out = []
    for a in anns:
        mask = IE.decode_runs(IE.annotation_counts(a["segmentation"]), IC.H, IC.W)
        if a["iscrowd"] and keep_crowds:
            out.append(a)
            continue
        poly = PC.rect_poly(*_box(mask))
        np.testing.assert_array_equal(IE.decode_runs(P.polygon_counts(poly, IC.H, IC.W), IC.H, IC.W), mask)
        out.append(dict(a, segmentation=[poly]))
    return out


def _eval(ctx, c, anns, image, topk, polygons):
    """-> (rows [topk], n_rows, flags) of one picture through Context.instance_eval"""
    masks, table, scores = _pad_case(c, topk)
    ident = {k: k for k in range(c["K"])}
    gt = IE.gt_rows(anns, ident, polygons=True, hw=(IC.H, IC.W)) if polygons else IE.gt_rows(anns, ident)
    dgt = ctx.instance_gt_to_device(*gt)
    assert ("gt_polys" in dgt) == polygons
    rows, n_rows, flags = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), ctx.zeros((1,), np.int32)
    ctx.instance_eval((IC.H, IC.W), ctx.to_device(table), ctx.to_device(scores), topk, dgt, c["K"], image, rows.arr, n_rows.arr, flags,
                      masks=ctx.to_device(masks))
    ctx.sync()
    return rows.read(), int(n_rows.read()[0]), int(flags.numpy()[0])


def _host_rows(c, image, topk):
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"])
    assert flags == 0
    full = np.zeros(topk, IE.ROW_DTYPE)
    full[:len(rows)] = rows
    return full


def test_a_null_polygon_part_is_instance_eval(ctx):
    c = IC.random_case()
    topk = 100
    masks, table, scores = _pad_case(c, topk)
    gt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])}))
    dm, dt, ds = ctx.to_device(masks), ctx.to_device(table), ctx.to_device(scores)
    thr = np.ascontiguousarray(IE.IOU_THRS)
    got = []
    for fn in ("eval", "poly"):
        rows, n_rows, flags = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
        ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
        d = InstEvalDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk = IC.H, IC.W, dm.ptr, U8, dt.ptr, ds.ptr, topk
        d.gt_runs, d.gt_offsets, d.gt_rows, d.n_gt, d.num_categories, d.image = gt["runs"].ptr, gt["offsets"].ptr, gt["rows"].ptr, gt["n_gt"], c["K"], 5
        d.iou_thresholds, d.rows, d.n_rows, d.flags = thr.ctypes.data, rows.arr.ptr, n_rows.arr.ptr, flags.arr.ptr
        rc = ctx.lib.odise_hip_instance_eval(ctx.h, C.byref(d)) if fn == "eval" else ctx.lib.odise_hip_instance_eval_poly(ctx.h, C.byref(d), None)
        assert rc == 0, ctx.lib.odise_hip_last_error()
        ctx.sync()
        got.append((rows.read().tobytes(), int(n_rows.read()[0]), int(flags.read()[0])))
    assert got[0] == got[1] and got[0][1:] == (100, 0)
    assert got[0][0] == _host_rows(c, 5, topk).tobytes()


@pytest.mark.parametrize("name", sorted(IC.matching_cases()) + ["random"])
def test_polygon_ground_truth_gives_the_rows_of_the_host_loop_and_of_the_rle_form(ctx, name):
    c = IC.random_case() if name == "random" else IC.matching_cases()[name]
    topk = 100 if name == "random" else len(c["masks"]) + 3
    poly_anns = _as_polygons(c["annotations"], keep_crowds=name != "crowd")    # that picture has nothing but a crowd: a crowd polygon
    assert any(not isinstance(a["segmentation"], dict) for a in poly_anns)
    want = _host_rows(c, 9, topk)
    as_rle = _eval(ctx, c, c["annotations"], 9, topk, polygons=False)
    as_poly = _eval(ctx, c, poly_anns, 9, topk, polygons=True)
    assert as_rle[1:] == as_poly[1:] == (len(c["masks"]), 0)
    for field in IE.ROW_DTYPE.names:
        np.testing.assert_array_equal(as_poly[0][field], want[field], err_msg=field)
    assert as_poly[0].tobytes() == want.tobytes() == as_rle[0].tobytes()


def test_runs_and_polygons_on_one_ground_truth_raise_flag_4_and_a_bad_polygon_flag_8(ctx):
    c = IC.matching_cases()["break"]
    topk = 4
    poly_anns = _as_polygons(c["annotations"])
    ident = {0: 0}
    rows, runs, offs, xy, poly_offs, gt_polys = IE.gt_rows(poly_anns, ident, polygons=True, hw=(IC.H, IC.W))
    assert list(gt_polys) == [0, 0, 1] and offs[1] > 0 and offs[2] == offs[1]
    masks, table, scores = _pad_case(c, topk)

    def run(runs, offs, xy):
        dgt = ctx.instance_gt_to_device(rows, runs, offs, xy, poly_offs, gt_polys)
        out, n_rows, flags = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), ctx.zeros((1,), np.int32)
        ctx.lib.odise_hip_memset(ctx.h, out.arr.ptr, 0xFF, out.nbytes)
        ctx.instance_eval((IC.H, IC.W), ctx.to_device(table), ctx.to_device(scores), topk, dgt, 1, 0, out.arr, n_rows.arr, flags,
                          masks=ctx.to_device(masks))
        ctx.sync()
        return out.read(), int(n_rows.read()[0]), int(flags.numpy()[0])

    good = run(runs, offs, xy)
    assert good[1:] == (1, 0) and good[0].tobytes() == _host_rows(c, 0, topk).tobytes()
    mixed = run(np.concatenate([runs, runs]), np.asarray([0, offs[1], 2 * offs[1]]), xy)   # the polygon ground truth carries valid runs as well
    assert mixed[1:] == (0, IE.FLAG_BAD_GT) and not mixed[0].view(np.uint8).any()
    nan = xy.copy()
    nan[3] = np.nan
    broken = run(runs, offs, nan)
    assert broken[1:] == (0, IE.FLAG_BAD_POLYGON) and not broken[0].view(np.uint8).any()


def test_evaluator_end_to_end_on_polygons_mixed_with_rle_crowds(ctx):
    """Three pictures of dense detections against COCO-style ground truth - polygons for the objects, RLE for the crowds - through
    HipInstanceSegEvaluator; evaluate() equals the host accumulate / results over annotation_to_counts."""
    K = 5
    names = [f"class{k}" for k in range(K)]
    ev = HipInstanceSegEvaluator(ctx, {100 + k: k for k in range(K)}, names, topk=40)
    ev.CHUNK = 2
    ev.reset()
    host_rows, npig = [], np.zeros((K, 4), np.int64)
    for i, (seed, n, n_gt) in enumerate(((21, 40, 20), (22, 25, 12), (23, 33, 30))):
        c = IC.random_case(seed=seed, n=n, n_gt=n_gt, K=K)
        anns = _as_polygons(c["annotations"])
        assert any(isinstance(a["segmentation"], dict) for a in anns) and any(isinstance(a["segmentation"], list) for a in anns)
        counts = [P.annotation_to_counts(a["segmentation"], IC.H, IC.W) for a in anns]
        table = IE.gt_rows(anns, {k: k for k in range(K)}, polygons=True, hw=(IC.H, IC.W))[0]
        rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, i, num_categories=K)
        assert flags == 0
        host_rows.append(rows)
        npig += IE.npig(table, K)
        masks, inst_table, scores = _pad_case(c, 40)
        dataset_anns = [dict(a, category_id=a["category_id"] + 100) for a in anns]
        ev.process(0, ctx.to_device(inst_table), ctx.to_device(scores), (0, 0), (0, 0), (IC.H, IC.W), dataset_anns, i, pred_masks=ctx.to_device(masks))
    got = ev.evaluate()
    want = IE.results(*IE.accumulate(np.concatenate(host_rows), npig, K), names)
    assert ev.rows().tobytes() == np.concatenate(host_rows).tobytes()
    assert set(got) == set(want) and not math.isnan(got["AP"]) and got["AP"] > 0
    for k in want:
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), k
