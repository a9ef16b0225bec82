"""Host restatement of the segm evaluation of instance masks (numpy): the reference of `Context.mask_iou` / `Context.instance_eval`
(csrc/inst_eval.hip) and the metric arithmetic of InstanceSegEvaluator / COCOEvaluator(tasks=("segm",)), which stays on the host.

`image_rows` is pycocotools' `COCOeval.evaluateImg` for iouType "segm", useCats = 1 and maxDets 100, written the way it is written there -
Python loops over the detections and the ground truths sorted by ignore - for all four area ranges and the ten IoU thresholds at once:

    iou                      maskApi.c rleIou on exact pixel counts: inter == 0 -> 0, a crowd ground truth -> inter / area_d, otherwise
                             inter / (area_d + area_g - inter)
    detections               of a category in descending score, ties in table order (mergesort on -score)
    ground truths            ignore = iscrowd or the annotation's area outside the range; non-ignored first, each group in annotation order
    matching                 best = min(t, 1 - 1e-10); a ground truth already matched that is no crowd is skipped; the walk stops at the
                             first ignored one once a non-ignored match is held; iou < best is skipped; otherwise the match moves there
    ignored detections       a matched one takes the ignore bit of its ground truth, an unmatched one is ignored when its own area (the
                             pixels of its mask) lies outside the range

What it keeps of a detection is one `ROW_DTYPE` record (odise_inst_eval_row): score, category, area, image and the matched / ignored
bits of the 40 (range a, threshold t) cells, bit 10 a + t.  `accumulate` is `COCOeval.accumulate` over such rows and the count of
non-ignored ground truths per (category, range), `summarize` the twelve COCO numbers, `results` detectron2's dict.

iouType "bbox" is the same walk over another IoU: `image_rows(..., iou_type="bbox", gt_boxes=...)` takes the detections' boxes from their
masks (`mask_boxes`: detectron2 BitMasks.get_bounding_boxes; csrc/inst_box.hip), `box_iou` is maskApi.c bbIou, a row's area is its box's
w * h (COCO.loadRes), and the ignore bits of the ground truth stay those of `gt_rows` (the annotation's `area` in both tasks).

iouType "boundary" (Boundary AP: Cheng et al., "Boundary IoU", CVPR 2021; the iouType LVIS scores with) is the same walk again:
`image_rows(..., iou_type="boundary")` matches on `boundary_iou` = min(mask IoU, rleIou of the two boundaries), a boundary being
`mask_boundary` = mask & ~erode(mask) (csrc/inst_boundary.hip); a row's area and the ignore rule of an unmatched detection are the segm
task's.  The rule is restated from the paper and from detectron2's `_mask_to_boundary` (sem_boundary.py) and pinned to the literal
repeated 3x3 erosion and to hand-worked pictures (tests/test_instance_boundary_cpu.py); parity with the published boundary-iou package is
UNPINNED: that package is no dependency of this project and no test compares against it.

Ground truth is RLE (compressed or uncompressed) or polygons: `gt_rows(..., polygons=True)` packs the polygons for the device, which
rasterises them (csrc/poly.hip; host reference: odise_amd/coco_poly.py).
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from . import coco_poly, coco_rle, sem_boundary

# odise_inst_eval_row (include/odise_hip.h)
ROW_DTYPE = np.dtype([("score", "<f4"), ("category", "<i4"), ("area", "<i4"), ("image", "<i4"), ("matched", "<u8"), ("ignored", "<u8")])
IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)     # cocoeval.Params.setDetParams
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))    # all, small, medium, large; ends included
MAX_DETECTIONS, MAX_GT = 100, 1024
FLAG_BAD_RUNS, FLAG_BAD_CLASS, FLAG_BAD_GT, FLAG_BAD_POLYGON = 1, 2, 4, 8
FLAG_NAMES = {FLAG_BAD_RUNS: "the run lengths of a ground-truth mask do not sum to h * w",
              FLAG_BAD_CLASS: "a predicted class is outside [0, num_categories)",
              FLAG_BAD_GT: "a ground-truth category is outside [0, num_categories), iscrowd is not 0 / 1, a ground truth has both runs "
                           "and polygons, or a ground-truth box has a member that is not finite",
              FLAG_BAD_POLYGON: "a polygon has fewer than three vertices, or a coordinate is NaN or larger than 2^26 in magnitude"}


def flag_names(flags: int) -> list:
    return [name for bit, name in FLAG_NAMES.items() if flags & bit]


# ---- masks --------------------------------------------------------------------------------------------------------------------------------
def decode_runs(counts, h: int, w: int) -> np.ndarray:
    """uint8 [h, w] mask of uncompressed run lengths over the column-major order (zeros first, alternating; zero-length runs anywhere).
    Counts that do not sum to h * w are what flag 1 reports: the missing tail is zeros, what lies past the end is dropped."""
    cnts = np.asarray(counts, np.int64).reshape(-1)
    vals = (np.arange(cnts.size) & 1).astype(np.uint8)
    flat = np.repeat(vals, cnts)[: h * w]
    flat = np.concatenate([flat, np.zeros(h * w - flat.size, np.uint8)])
    return flat.reshape((h, w), order="F")


def rle_iou(inter: int, area_d: int, area_g: int, crowd: bool) -> float:
    if inter == 0:
        return 0.0
    return float(np.float64(inter) / np.float64(area_d)) if crowd else float(np.float64(inter) / np.float64(area_d + area_g - inter))


def mask_iou(dense_masks, gt_counts, iscrowd=None) -> np.ndarray:
    """float64 [n, n_gt]: pycocotools' mask.iou of dense masks [n, h, w] (nonzero = 1) against run-length masks."""
    d = np.asarray(dense_masks) != 0
    n, h, w = d.shape
    g = np.stack([decode_runs(c, h, w) for c in gt_counts]).astype(bool) if len(gt_counts) else np.zeros((0, h, w), bool)
    crowd = np.zeros(len(g), bool) if iscrowd is None else np.asarray(iscrowd).astype(bool)
    area_d, area_g = d.reshape(n, h * w).sum(1), g.reshape(len(g), h * w).sum(1)
    out = np.zeros((n, len(g)), np.float64)
    for i in range(n):
        for j in range(len(g)):
            out[i, j] = rle_iou(int(np.count_nonzero(d[i] & g[j])), int(area_d[i]), int(area_g[j]), bool(crowd[j]))
    return out


# ---- boundaries ---------------------------------------------------------------------------------------------------------------------------
def mask_boundary(masks, radius=None) -> np.ndarray:
    """uint8 [n, h, w]: m & ~erode(m, r) of masks [n, h, w] (nonzero = 1), erode the (2 r + 1)^2 minimum that sees zeros outside the
    picture; radius None (or <= 0): sem_boundary.boundary_radius(h, w).  With 2 r + 1 > min(h, w) everything erodes and the boundary is
    the mask itself.  This is sem_boundary.mask_to_boundary on a 0 / 1 map, written another way (window sums of a zero-padded summed-area
    table: a pixel survives the erosion when its window holds (2 r + 1)^2 ones), so that a test can hold the two against each other."""
    m = (np.asarray(masks) != 0).astype(np.uint8)
    n, h, w = m.shape
    r = sem_boundary.boundary_radius(h, w) if radius is None or radius <= 0 else int(radius)
    L = 2 * r + 1
    if L > min(h, w) or n == 0:
        return m
    out = np.empty_like(m)
    for i in range(n):
        sat = np.zeros((h + L, w + L), np.int64)                              # sat[y, x] = ones of the padded mask above and left of (y, x)
        sat[r + 1:r + 1 + h, r + 1:r + 1 + w] = m[i]
        sat = sat.cumsum(0).cumsum(1)
        win = sat[L:, L:] - sat[:-L, L:] - sat[L:, :-L] + sat[:-L, :-L]       # [h, w]: the ones of the window centred on every pixel
        out[i] = m[i] & (win != L * L)
    return out


def boundary_iou(dense_masks, gt_counts, iscrowd=None, radius=None):
    """-> (iou, mask_iou, b_iou), float64 [n, n_gt] each: `mask_iou`, the same rleIou on the exact pixel counts of the two boundaries
    (`mask_boundary` of both sides, one radius; inter == 0 -> 0, a crowd -> inter / the area of the detection's boundary), and their
    minimum, the IoU that Boundary AP matches on (Cheng et al., "Boundary IoU", CVPR 2021)."""
    d = np.asarray(dense_masks) != 0
    n, h, w = d.shape
    g = np.stack([decode_runs(c, h, w) for c in gt_counts]).astype(bool) if len(gt_counts) else np.zeros((0, h, w), bool)
    crowd = np.zeros(len(g), bool) if iscrowd is None else np.asarray(iscrowd).astype(bool)
    bd, bg = mask_boundary(d, radius).astype(bool), mask_boundary(g, radius).astype(bool)
    area_d, area_g = bd.reshape(n, h * w).sum(1), bg.reshape(len(g), h * w).sum(1)
    m_iou, b_iou = mask_iou(d, gt_counts, iscrowd), np.zeros((n, len(g)), np.float64)
    for i in range(n):
        for j in range(len(g)):
            b_iou[i, j] = rle_iou(int(np.count_nonzero(bd[i] & bg[j])), int(area_d[i]), int(area_g[j]), bool(crowd[j]))
    return np.minimum(m_iou, b_iou), m_iou, b_iou


# ---- boxes --------------------------------------------------------------------------------------------------------------------------------
def mask_boxes(masks) -> np.ndarray:
    """float32 [n, 4] XYXY: detectron2 BitMasks.get_bounding_boxes of masks [n, h, w] (nonzero = 1) - first column with a pixel, first row
    with a pixel, last column + 1, last row + 1; a mask without a pixel gives zeros."""
    m = np.asarray(masks) != 0
    boxes = np.zeros((m.shape[0], 4), np.float32)
    for i in range(m.shape[0]):
        x, y = np.flatnonzero(m[i].any(axis=0)), np.flatnonzero(m[i].any(axis=1))
        if len(x) > 0 and len(y) > 0:
            boxes[i] = (x[0], y[0], x[-1] + 1, y[-1] + 1)
    return boxes


def xyxy_to_xywh(boxes) -> np.ndarray:
    """float64 [n, 4] XYWH of XYXY boxes (BoxMode.convert(XYXY_ABS, XYWH_ABS): exact on the integers of `mask_boxes`)."""
    b = np.array(boxes, np.float64).reshape(-1, 4)
    b[:, 2] -= b[:, 0]
    b[:, 3] -= b[:, 1]
    return b


def box_iou(dt_xywh, gt_xywh, iscrowd=None) -> np.ndarray:
    """float64 [n, n_gt]: maskApi.c bbIou (pycocotools mask.iou of boxes) in Python floats, one rounded operation per statement."""
    dt = np.asarray(dt_xywh, np.float64).reshape(-1, 4).tolist()
    gt = np.asarray(gt_xywh, np.float64).reshape(-1, 4).tolist()
    crowd = [False] * len(gt) if iscrowd is None else [bool(c) for c in np.asarray(iscrowd).reshape(-1)]
    out = np.zeros((len(dt), len(gt)), np.float64)
    for g, G in enumerate(gt):
        ga = G[2] * G[3]
        for d, D in enumerate(dt):
            da = D[2] * D[3]
            dr = D[2] + D[0]
            gr = G[2] + G[0]
            w = min(dr, gr) - max(D[0], G[0])
            if w <= 0:
                continue
            db = D[3] + D[1]
            gb = G[3] + G[1]
            h = min(db, gb) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            if crowd[g]:
                u = da
            else:
                u = da + ga
                u = u - i
            out[d, g] = i / u
    return out


def gt_boxes(annotations) -> np.ndarray:
    """float64 [n_gt, 4]: the XYWH `bbox` of every annotation; one without a `bbox` raises ValueError."""
    out = np.zeros((len(annotations), 4), np.float64)
    for i, ann in enumerate(annotations):
        if "bbox" not in ann:
            raise ValueError(f"bbox evaluation: annotation {i} has no bbox")
        out[i] = np.asarray(ann["bbox"], np.float64).reshape(4)
    return out


# ---- ground truth -------------------------------------------------------------------------------------------------------------------------
def annotation_counts(segmentation) -> np.ndarray:
    """Uncompressed counts of an RLE dict: `counts` a compressed string / bytes or a list of run lengths."""
    c = segmentation["counts"]
    if isinstance(c, (bytes, bytearray)):
        c = c.decode("utf-8")
    return coco_rle.string_to_counts(c) if isinstance(c, str) else np.asarray(c, np.int64)


def gt_rows(annotations, to_contiguous: Dict[int, int], polygons: bool = False, hw=None):
    """The annotation dicts of a picture (category_id as in the dataset, iscrowd, area, segmentation = RLE dict) ->
    (rows int32 [n_gt, 3] = contiguous category | iscrowd | bits 0..3: area outside range a, runs uint32 (all masks back to back),
    offsets int64 [n_gt + 1]).  The area is the annotation's float `area` (the evaluator compares that, not the mask); without one, the
    pixels of the mask.
    polygons=True also takes annotations whose segmentation is a list of polygons (flat lists x0 y0 x1 y1 ..), on a picture of
    hw = (h, w), and returns three more: xy float64 (all vertices), poly_offsets int64 [n_poly + 1] in vertices, gt_polys int32
    [n_gt + 1] - the arguments of odise_hip_instance_eval_poly.  A polygon annotation has an empty run range; without an `area` its mask
    is rasterised on the host (coco_poly) for the pixel count.  A malformed polygon (odd length, fewer than 6 numbers) raises ValueError."""
    rows = np.zeros((len(annotations), 3), np.int32)
    runs, offsets = [], [0]
    xy, poly_offsets, gt_polys = [], [0], [0]
    for i, ann in enumerate(annotations):
        seg = ann["segmentation"]
        if not isinstance(seg, dict):
            if not polygons:
                raise ValueError("instance evaluation takes RLE ground truth; convert polygon annotations to RLE first")
            if hw is None:
                raise ValueError("polygon ground truth needs the picture's (h, w)")
            for poly in seg:
                poly = coco_poly.check_polygon(poly)
                xy.append(poly)
                poly_offsets.append(poly_offsets[-1] + poly.size // 2)
            cnts = np.zeros(0, np.int64)
            area = float(ann["area"]) if "area" in ann else float(coco_poly.annotation_to_counts(seg, int(hw[0]), int(hw[1]))[1::2].sum())
        else:
            cnts = annotation_counts(seg)
            area = float(ann["area"]) if "area" in ann else float(cnts[1::2].sum())
        outside = sum(1 << a for a, (lo, hi) in enumerate(AREA_RNG) if area < lo or area > hi)
        rows[i] = (to_contiguous[int(ann["category_id"])], int(ann.get("iscrowd", 0)), outside)
        runs.append(np.asarray(cnts, np.uint32))
        offsets.append(offsets[-1] + len(cnts))
        gt_polys.append(len(poly_offsets) - 1)
    out = rows, (np.concatenate(runs) if runs else np.zeros(0, np.uint32)), np.asarray(offsets, np.int64)
    if polygons:
        out += ((np.concatenate(xy) if xy else np.zeros(0, np.float64)), np.asarray(poly_offsets, np.int64), np.asarray(gt_polys, np.int32))
    return out


def npig(rows, K: int) -> np.ndarray:
    """int64 [K, 4]: the ground truths of a category that are not ignored in range a (no crowd, area inside)."""
    out = np.zeros((K, 4), np.int64)
    for cat, crowd, outside in np.asarray(rows, np.int64).reshape(-1, 3):
        for a in range(4):
            if not crowd and not (outside >> a) & 1:
                out[cat, a] += 1
    return out


# ---- evaluateImg --------------------------------------------------------------------------------------------------------------------------
def area_outside(area, a: int) -> bool:
    return bool(area < AREA_RNG[a][0] or area > AREA_RNG[a][1])


def image_rows(masks, scores, classes, gt_counts, gt_table, image: int = 0, iou_thrs=IOU_THRS, num_categories=None, iou_type: str = "segm",
               gt_boxes=None, radius=None):
    """COCOeval.evaluateImg of one picture -> (rows ROW_DTYPE [n] in descending score, flags).  masks [n, h, w] (nonzero = 1), n <= 100;
    gt_counts: the run lengths of every ground truth; gt_table: `gt_rows`' table.  A picture that raises a flag has no rows.
    iou_type "bbox": the IoU is `box_iou` of `mask_boxes(masks)` against gt_boxes float64 [n_gt, 4] XYWH, a row's area is its box's
    w * h, and gt_counts is not looked at (None will do).
    iou_type "boundary": the IoU is `boundary_iou(masks, gt_counts, iscrowd, radius)[0]`; areas, flags and ignore bits are those of "segm"."""
    assert iou_type in ("segm", "bbox", "boundary"), iou_type
    bbox = iou_type == "bbox"
    d = np.asarray(masks) != 0
    n, h, w = d.shape
    scores, classes = np.asarray(scores, np.float32).reshape(-1), np.asarray(classes, np.int64).reshape(-1)
    table = np.asarray(gt_table, np.int64).reshape(-1, 3)
    n_gt = len(table)
    assert n <= MAX_DETECTIONS and len(scores) >= n and len(classes) >= n and (bbox or len(gt_counts) == n_gt)
    flags = 0
    if bbox:
        gtb = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
        assert len(gtb) == n_gt, (len(gtb), n_gt)
        if not np.isfinite(gtb).all():
            flags |= FLAG_BAD_GT
    elif any(int(np.asarray(c, np.int64).sum()) != h * w for c in gt_counts):
        flags |= FLAG_BAD_RUNS
    flags |= _table_flags(n, classes, table, num_categories)
    if flags:
        return np.zeros(0, ROW_DTYPE), flags
    if bbox:
        dtb = xyxy_to_xywh(mask_boxes(d))
        ious, areas = box_iou(dtb, gtb, table[:, 1]), (dtb[:, 2] * dtb[:, 3]).astype(np.int64)
    elif iou_type == "boundary":
        ious, areas = boundary_iou(d, gt_counts, table[:, 1], radius)[0], d.reshape(n, h * w).sum(1)
    else:
        ious, areas = mask_iou(d, gt_counts, table[:, 1]), d.reshape(n, h * w).sum(1)
    return _walk(n, scores, classes, table, ious, areas, None, image, iou_thrs), 0


def _table_flags(n: int, classes, table, num_categories) -> int:
    """Flags 2 and 4 of the classes of n detections and of a ground-truth table (num_categories None: the ranges are not checked)."""
    flags, n_gt = 0, len(table)
    if num_categories is not None:
        if n and (classes[:n].min() < 0 or classes[:n].max() >= num_categories):
            flags |= FLAG_BAD_CLASS
        if n_gt and (table[:, 0].min() < 0 or table[:, 0].max() >= num_categories):
            flags |= FLAG_BAD_GT
    if n_gt and not np.isin(table[:, 1], (0, 1)).all():
        flags |= FLAG_BAD_GT
    return flags


def _walk(n: int, scores, classes, table, ious, areas, outside, image: int, iou_thrs):
    """The walk of `image_rows` over an IoU matrix from outside -> rows ROW_DTYPE [n] in descending score.  ious float64 [n, n_gt];
    areas [n]: what a row shows; outside: bool [n, 4], an unmatched detection lies outside range a - None = `area_outside` of the row's
    area.  The seam video_eval.video_rows enters by: a track stands where a detection stands."""
    n_gt = len(table)
    order = np.argsort(-scores[:n], kind="mergesort")
    rows = np.zeros(n, ROW_DTYPE)
    rows["score"], rows["category"], rows["image"] = scores[order], classes[order], image
    rows["area"] = areas[order]
    pos = {int(dd): k for k, dd in enumerate(order)}
    for c in np.unique(classes[:n]):
        dt = [int(i) for i in order if classes[i] == c]
        gt_c = [j for j in range(n_gt) if table[j, 0] == c]
        for a in range(4):
            ignore = [bool(table[j, 1]) or bool((table[j, 2] >> a) & 1) for j in gt_c]
            gtind = np.argsort(np.asarray(ignore, np.int64), kind="mergesort") if gt_c else []
            gt = [gt_c[i] for i in gtind]
            gt_ig = [ignore[i] for i in gtind]
            crowd = [bool(table[j, 1]) for j in gt]
            for t, thr in enumerate(iou_thrs):
                gtm = [False] * len(gt)
                for i in dt:
                    iou = min(float(thr), 1 - 1e-10)
                    m = -1
                    for gind, j in enumerate(gt):
                        if gtm[gind] and not crowd[gind]:      # already matched, and not a crowd
                            continue
                        if m > -1 and not gt_ig[m] and gt_ig[gind]:   # a regular match is held and only ignored ones follow
                            break
                        if ious[i, j] < iou:
                            continue
                        iou = ious[i, j]
                        m = gind
                    bit = np.uint64(1 << (10 * a + t))
                    if m > -1:
                        gtm[m] = True
                        rows["matched"][pos[i]] |= bit
                        ig = gt_ig[m]
                    else:
                        ig = area_outside(int(rows["area"][pos[i]]), a) if outside is None else bool(outside[i][a])
                    if ig:
                        rows["ignored"][pos[i]] |= bit
    return rows


# ---- accumulate / summarize ---------------------------------------------------------------------------------------------------------------
def accumulate(rows, npig_ka, K: int):
    """COCOeval.accumulate for maxDets (1, 10, 100) and recThrs linspace(0, 1, 101) -> (precision [T, R, K, A, M], recall [T, K, A, M]),
    -1 where a (category, range) has no non-ignored ground truth.  rows: ROW_DTYPE of any number of pictures, every picture's rows in
    descending score; they are ordered by `image` first (stable), so the result does not depend on how the pictures were sharded."""
    rows = np.asarray(rows, ROW_DTYPE).reshape(-1)
    rows = rows[np.argsort(rows["image"], kind="stable")]
    npig_ka = np.asarray(npig_ka, np.int64).reshape(K, 4)
    T, R, A, M = len(IOU_THRS), len(REC_THRS), 4, len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        rk = rows[rows["category"] == k]
        first = np.flatnonzero(np.r_[True, rk["image"][1:] != rk["image"][:-1]]) if len(rk) else np.zeros(0, np.int64)
        rank = np.arange(len(rk)) - np.repeat(first, np.diff(np.r_[first, len(rk)]))         # position among the picture's rows of category k
        for mi, max_det in enumerate(MAX_DETS):
            sel = rk[rank < max_det]
            sel = sel[np.argsort(-sel["score"], kind="mergesort")]
            for a in range(A):
                n_pos = int(npig_ka[k, a])
                if n_pos == 0:
                    continue
                for t in range(T):
                    bit = np.uint64(10 * a + t)
                    dtm = ((sel["matched"] >> bit) & np.uint64(1)).astype(bool)
                    dt_ig = ((sel["ignored"] >> bit) & np.uint64(1)).astype(bool)
                    tp = np.cumsum(dtm & ~dt_ig).astype(np.float64)
                    fp = np.cumsum(~dtm & ~dt_ig).astype(np.float64)
                    nd = len(tp)
                    rc = tp / n_pos
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr       # the right-to-left running maximum
                    q = np.zeros(R)
                    inds = np.searchsorted(rc, REC_THRS, side="left")
                    ok = inds < nd                                                  # entries past the end stay 0
                    q[ok] = pr[inds[ok]]
                    precision[t, :, k, a, mi] = q
    return precision, recall


# odise_hip_instance_accumulate (csrc/inst_accum.hip): `accumulate` on the device
ACCUM_FLAG_BAD_CLASS, ACCUM_FLAG_NAN_SCORE = 1, 2
ACCUM_FLAG_NAMES = {ACCUM_FLAG_BAD_CLASS: "a row's category is outside [0, num_categories)", ACCUM_FLAG_NAN_SCORE: "a row's score is NaN"}


def accumulate_flag_names(flags: int) -> list:
    return [name for bit, name in ACCUM_FLAG_NAMES.items() if flags & bit]


def score_sort_key(scores) -> np.ndarray:
    """uint32 keys whose ascending order is the descending order of float32 scores, as `-score` orders them: -0 ties with +0, +inf comes
    first, equal scores (and only those) have equal keys.  The key the device sort uses (csrc/inst_accum.hip score_key); NaN has no
    place in it."""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1)
    u = np.where(s == 0, np.float32(0), s).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return ~u


def _mean_valid(s: np.ndarray) -> float:
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def summarize(precision, recall) -> np.ndarray:
    """COCOeval.summarize: AP, AP50, AP75, APs, APm, APl (maxDets 100), AR at maxDets 1 / 10 / 100, ARs, ARm, ARl (maxDets 100)."""
    t50, t75 = int(np.flatnonzero(np.isclose(IOU_THRS, .5))[0]), int(np.flatnonzero(np.isclose(IOU_THRS, .75))[0])
    s = np.zeros(12)
    s[0] = _mean_valid(precision[:, :, :, 0, 2])
    s[1] = _mean_valid(precision[t50:t50 + 1, :, :, 0, 2])
    s[2] = _mean_valid(precision[t75:t75 + 1, :, :, 0, 2])
    for i, a in enumerate((1, 2, 3)):
        s[3 + i] = _mean_valid(precision[:, :, :, a, 2])
        s[9 + i] = _mean_valid(recall[:, :, a, 2])
    for i in range(3):
        s[6 + i] = _mean_valid(recall[:, :, 0, i])
    return s


def results(precision, recall, class_names: Sequence[str]) -> dict:
    """detectron2 COCOEvaluator._derive_coco_results for "segm": AP, AP50, AP75, APs, APm, APl (x 100, NaN where nothing is > -1) and
    AP-<class name> per category."""
    s = summarize(precision, recall)
    out = {name: float(s[i] * 100) if s[i] >= 0 else float("nan") for i, name in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl"))}
    assert len(class_names) == precision.shape[2], (len(class_names), precision.shape)
    for k, name in enumerate(class_names):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        out["AP-" + name] = float(np.mean(p) * 100) if p.size else float("nan")
    return out
