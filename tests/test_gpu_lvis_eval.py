"""GPU: odise_hip_lvis_eval (csrc/lvis_eval.hip) against the numpy specification (odise_amd/lvis_eval.py image_rows).  Everything is
integers and single double divisions, so every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch

from odise_amd import coco_poly, coco_rle
from odise_amd import instance_eval as IE
from odise_amd import lvis_eval as LE
from odise_amd._lib import LvisTask
from odise_amd.runtime import _inst_eval_desc, _inst_poly_gt
from small_model import GROUPS, build_small, image_u8

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

CANARY, PAD = 0xA5, 256
H, W = 70, 37          # two words per column, the second ragged; an odd width
K = 70                 # bitsets of three words, the last ragged
TOPK, COUNT = 300, 257 # more than four 64-lane chunks of detections; rows past the count must stay unread
BIG, NEG, NEX, NEITHER = 5, 50, 41, 60   # 66 ground truths; no ground truth and in neg; not exhaustive; in no list and without ground truth
OTHERS = (3, 19, 40, NEX)                # one ground truth each; 3 and 19 share a wave (category & 15)
IDENT = {k: k for k in range(K)}


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


def rect(y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def rand_rect(g):
    y0, x0 = int(g.integers(0, H - 4)), int(g.integers(0, W - 4))
    return y0, int(g.integers(y0 + 2, H + 1)), x0, int(g.integers(x0 + 2, W + 1))


def picture(seed=0, polygons=True):
    """-> dict(masks uint8 [TOPK, H, W], scores, classes, anns, neg, nex): 257 detections over 19 categories, 70 ground truths of which
    66 share category BIG; scores in sixteenths (ties); a few ground truths carry `ignore` or an area in another range; junk past the count."""
    g = np.random.default_rng(seed)
    boxes = [rand_rect(g) for _ in range(66 + len(OTHERS))]
    cats = [BIG] * 66 + list(OTHERS)
    anns = []
    for i, (bx, c) in enumerate(zip(boxes, cats)):
        y0, y1, x0, x1 = bx
        if polygons and i % 3 == 1:
            seg = [[float(x0), float(y0), float(x1), float(y0), float(x1), float(y1), float(x0), float(y1)]]
        else:
            m = rect(*bx)
            seg = coco_rle.encode(m) if i % 3 == 0 else {"size": [H, W], "counts": coco_rle.mask_counts(m).tolist()}
        a = {"category_id": c, "segmentation": seg, "area": float((y1 - y0) * (x1 - x0)) * (20.0 if i % 7 == 0 else 1.0)}
        if i % 11 == 5:
            a["ignore"] = 1
        anns.append(a)
    det_cats = np.array([BIG] * 6 + list(OTHERS) + [NEG, NEITHER, 7, 23, 33, 34, 35, 36, 37, 38, 8, 9, 10, 24], np.int32)   # 19 values; 7 and 23 share a wave
    masks = np.ones((TOPK, H, W), np.uint8)
    classes = np.full(TOPK, 1 << 20, np.int32)
    scores = np.full(TOPK, np.nan, np.float32)
    for i in range(COUNT):
        classes[i] = det_cats[g.integers(0, len(det_cats))]
        src = [j for j, c in enumerate(cats) if c == classes[i]]
        if src and g.random() < .7:                                   # a ground truth of its category, shifted a little
            y0, y1, x0, x1 = boxes[src[int(g.integers(0, len(src)))]]
            dy, dx = (int(v) for v in g.integers(-1, 2, 2))
            masks[i] = rect(max(y0 + dy, 0), y1 + dy, max(x0 + dx, 0), x1 + dx)
        else:
            masks[i] = rect(*rand_rect(g))
        scores[i] = g.integers(0, 17) / 16
    return dict(masks=masks, scores=scores, classes=classes, anns=anns, neg=[NEG, 7, 33], nex=[NEX, 34, BIG] if seed % 2 else [NEX, 34])


def table_of(n, classes, queries=None, topk=TOPK):
    t = np.full(1 + 2 * topk, -77, np.int32)
    t[0] = n
    t[1:1 + topk] = np.arange(topk) if queries is None else queries
    t[1 + topk:] = classes
    return t


def gt_counts(anns, h=H, w=W):
    return [IE.annotation_counts(a["segmentation"]) if isinstance(a["segmentation"], dict) else coco_poly.annotation_to_counts(a["segmentation"], h, w)
            for a in anns]


def upload_gt(ctx, anns, neg, nex, hw=(H, W), k=K, poke=None):
    table, runs, offsets, xy, poly_offsets, gt_polys = LE.gt_rows(anns, {i: i for i in range(k)}, polygons=True, hw=hw)
    if poke:
        poke(table, runs, xy)
    gt = ctx.instance_gt_to_device(table, runs, offsets, *((xy, poly_offsets, gt_polys) if len(poly_offsets) > 1 else ()),
                                   lvis_bits=(LE.category_bits(neg, k), LE.category_bits(nex, k)))
    return gt, table


def device_rows(ctx, masks, table, scores, gt, topk=TOPK, k=K, image=7, hw=(H, W), **logits):
    """-> (rows [n_rows], flags) with the canaries and the zeroed tail checked."""
    rows, n_rows, flags = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    ctx.lvis_eval(hw, ctx.to_device(table), ctx.to_device(scores), topk, gt, k, image, rows.arr, n_rows.arr, flags.arr,
                  masks=None if masks is None else ctx.to_device(masks), **logits)
    ctx.sync()
    r, n, f = rows.read(), int(n_rows.read()[0]), int(flags.read()[0])
    assert 0 <= n <= topk and r[n:].tobytes() == bytes(32 * (topk - n))
    return r[:n], f


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_picture_equals_the_specification(ctx, dtype):
    """Dense masks of both dtypes; polygons, compressed and uncompressed runs mixed; 66 ground truths walked by one wave."""
    for seed in (0, 1):
        p = picture(seed)
        gt, table = upload_gt(ctx, p["anns"], p["neg"], p["nex"])
        assert (table[:, 0] == BIG).sum() == 66 and len(table) == 70 and len(np.unique(p["classes"][:COUNT])) >= 17 and "gt_polys" in gt
        want, wf = LE.image_rows(p["masks"][:COUNT], p["scores"], p["classes"], gt_counts(p["anns"]), table, p["neg"], p["nex"], 7, num_categories=K)
        got, f = device_rows(ctx, (p["masks"] * 3).astype(dtype), table_of(COUNT, p["classes"]), p["scores"], gt)
        assert wf == 0 and f == 0 and 64 < len(want) < COUNT                    # some dropped, the rest in more than one chunk
        assert got.tobytes() == want.tobytes()
        assert not (want["category"] == NEITHER).any() and (want["category"] == NEG).any() and (want["matched"] != 0).any()
        un = want[(want["category"] == NEX) & (want["matched"] == 0)]
        assert len(un) and (un["ignored"] == (1 << 40) - 1).all()


def test_flags_zero_the_picture(ctx):
    p = picture(0)
    def bad_runs(table, runs, xy): runs[0] += 1
    def bad_gt_cat(table, runs, xy): table[3, 0] = K
    def crowd(table, runs, xy): table[4, 1] = 1
    def bad_poly(table, runs, xy): xy[0] = np.nan
    for flag, poke, classes in ((1, bad_runs, None), (4, bad_gt_cat, None), (4, crowd, None), (8, bad_poly, None), (2, None, COUNT - 1)):
        gt, _ = upload_gt(ctx, p["anns"], p["neg"], p["nex"], poke=poke)
        cl = p["classes"].copy()
        if classes is not None:
            cl[classes] = K
        got, f = device_rows(ctx, p["masks"], table_of(COUNT, cl), p["scores"], gt)
        assert f == flag and len(got) == 0, (flag, f)


def test_bad_arguments_write_nothing(ctx):
    p = picture(0)
    gt, _ = upload_gt(ctx, p["anns"], p["neg"], p["nex"])
    rows, n_rows, flags = Guarded(ctx, (TOPK + 1,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
    masks, table, scores = ctx.to_device(np.ones((TOPK + 1, H, W), np.uint8)), ctx.to_device(table_of(COUNT, p["classes"])), ctx.to_device(p["scores"])

    def call(topk=TOPK, lv=True, neg=True, nex=True, n_gt=70, k=K):
        d, _thr = _inst_eval_desc("lvis_eval", out_hw=(H, W), table_row=table, scores_row=scores, topk=TOPK, gt=gt, num_categories=k, image=0,
                                  rows=rows.arr, n_rows=n_rows.arr, flags=flags.arr, masks=None, b=0, pad_hw=(0, 0), img_hw=(0, 0), iou_thresholds=None)
        d.masks, d.dtype, d.topk, d.n_gt = masks.ptr, 2, topk, n_gt
        t = LvisTask()
        t.neg_bits, t.not_exhaustive_bits = gt["neg_bits"].ptr if neg else None, gt["not_exhaustive_bits"].ptr if nex else None
        return ctx.lib.odise_hip_lvis_eval(ctx.h, C.byref(d), _inst_poly_gt(gt), C.byref(t) if lv else None)

    for bad in (dict(topk=0), dict(topk=301), dict(lv=False), dict(neg=False), dict(nex=False), dict(n_gt=1025), dict(k=0), dict(k=65536)):
        assert call(**bad) == -1, bad
    ctx.sync()
    for o in (rows, n_rows, flags):
        o.read(intact=True)
    assert ctx.lib.odise_hip_instance_eval(ctx.h, C.byref(_inst_eval_desc("x", out_hw=(H, W), table_row=table, scores_row=scores, topk=101, gt=gt,
                                           num_categories=K, image=0, rows=rows.arr, n_rows=n_rows.arr, flags=flags.arr, masks=None, b=0, pad_hw=(0, 0),
                                           img_hw=(0, 0), iou_thresholds=None)[0])) == -1          # the cap of 100 stays where it was
    assert b"1..100" in ctx.lib.odise_hip_last_error()
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    assert call() == 0                                                                              # the same descriptor, valid
    ctx.sync()
    assert int(flags.read()[0]) == 0 and 0 < int(n_rows.read()[0]) < COUNT


def test_no_ground_truth(ctx):
    p = picture(1)
    gt, table = upload_gt(ctx, [], p["neg"], [])
    got, f = device_rows(ctx, p["masks"], table_of(COUNT, p["classes"]), p["scores"], gt)
    want, _ = LE.image_rows(p["masks"][:COUNT], p["scores"], p["classes"], [], table, p["neg"], [], 7, num_categories=K)
    assert f == 0 and got.tobytes() == want.tobytes() and len(got) == np.isin(p["classes"][:COUNT], p["neg"]).sum() > 0
    assert (got["matched"] == 0).all() and (got["ignored"] & 0x3FF == 0).all()                      # every kept detection a false positive
    gt, _ = upload_gt(ctx, [], [], p["nex"])
    got, f = device_rows(ctx, p["masks"], table_of(COUNT, p["classes"]), p["scores"], gt)
    assert f == 0 and len(got) == 0                                                                 # every detection dropped


def test_without_its_rules_it_is_instance_eval(ctx):
    """topk 100, every detection's category with a ground truth, empty bitsets: the rows of odise_hip_instance_eval."""
    p = picture(2, polygons=False)
    keep = np.flatnonzero(np.isin(p["classes"][:COUNT], (BIG,) + OTHERS))[:93]
    masks, classes, scores = np.ones((100, H, W), np.uint8), np.full(100, 1 << 20, np.int32), np.full(100, np.nan, np.float32)
    masks[:93], classes[:93], scores[:93] = p["masks"][keep], p["classes"][keep], p["scores"][keep]
    for a in p["anns"]:
        a.pop("ignore", None)
    gt, table = upload_gt(ctx, p["anns"], [], [])
    got, f = device_rows(ctx, masks, table_of(93, classes, topk=100), scores, gt, topk=100)
    rows, n_rows, flags = Guarded(ctx, (100,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), ctx.zeros((1,), np.int32)
    ctx.instance_eval((H, W), ctx.to_device(table_of(93, classes, topk=100)), ctx.to_device(scores), 100, gt, K, 7, rows.arr, n_rows.arr, flags,
                      masks=ctx.to_device(masks))
    ctx.sync()
    assert f == 0 and int(flags.numpy()[0]) == 0 and int(n_rows.read()[0]) == 93 == len(got)
    assert rows.read()[:93].tobytes() == got.tobytes() and (got["matched"] != 0).any()


@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


def test_the_logits_path_packs_a_query_once_and_equals_the_dense_path(small, ctx):
    """A table of (query, class) pairs of the test's own over the mask logits of a head forward: the rows of the dense path on the masks
    odise_hip_instance_masks gives for the same pairs."""
    hip, h, w, oh, ow = small, 500, 502, 125, 122
    hip.keep_instance_selection = True
    try:
        hip.forward([{"image": image_u8(h, w, seed=1)}])
    finally:
        hip.keep_instance_selection = False
    sel = hip.last_selection
    Q, k = 20, len(GROUPS)
    g = np.random.default_rng(4)
    n = 150
    queries = np.full(TOPK, 1 << 20, np.int32)
    queries[:n] = g.integers(0, Q - 1, n)                       # query Q - 1 never; most several times
    queries[:4] = (3, 9, 3, 3)
    classes = np.full(TOPK, 1 << 20, np.int32)
    classes[:n] = g.integers(0, k, n)
    counts = np.bincount(queries[:n], minlength=Q)
    assert counts.max() >= 3 and (counts == 0).any() and counts[3] >= 3 and counts[Q - 1] == 0
    scores = np.full(TOPK, np.nan, np.float32)
    scores[:n] = g.integers(0, 17, n) / 16
    idx = ctx.to_device(np.where(queries < Q, queries, 0).astype(np.int32))
    dense = ctx.zeros((TOPK, oh, ow), np.float32)
    (ph, pw), (ih, iw) = sel["pad_hw"], sel["img_hw"][0]
    for c in range(0, TOPK, 100):
        assert ctx.lib.odise_hip_instance_masks(ctx.h, 0, C.c_void_p(idx.ptr + 4 * c), 100, ph, pw, ih, iw, oh, ow,
                                                C.c_void_p(dense.ptr + 4 * c * oh * ow)) == 0
    masks = (dense.numpy() != 0).astype(np.uint8)
    assert masks[:n].any()
    anns = [{"category_id": int(classes[i]), "area": float(masks[i].sum()), "segmentation": coco_rle.encode(masks[i])} for i in (0, 1, 5, 8)]
    neg = [c for c in range(k) if c % 2]
    gt, table = upload_gt(ctx, anns, neg, [2], hw=(oh, ow), k=k)
    t = table_of(n, classes, queries)
    want, wf = LE.image_rows(masks[:n], scores, classes, gt_counts(anns, oh, ow), table, neg, [2], 7, num_categories=k)
    by_dense, f0 = device_rows(ctx, masks, t, scores, gt, k=k, hw=(oh, ow))
    by_logits, f1 = device_rows(ctx, None, t, scores, gt, k=k, hw=(oh, ow), b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0])
    assert wf == f0 == f1 == 0 and len(want) > 0 and (want["matched"] != 0).any()
    assert by_dense.tobytes() == want.tobytes() and by_logits.tobytes() == by_dense.tobytes()
