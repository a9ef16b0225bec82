"""Host restatement of LVIS AP for instance masks (numpy): the reference of `Context.lvis_eval` / `Context.lvis_accumulate`
(csrc/lvis_eval.hip, csrc/inst_accum.hip) and the metric arithmetic of detectron2's LVISEvaluator for "segm", which stays on the host.

This docstring is the SPECIFICATION.  It restates lvis-api's `LVISEval` / `LVISResults` and detectron2's `_evaluate_predictions_on_lvis`;
it is pinned to hand-worked pictures, each built to separate one clause (tests/lvis_cases.py, tests/test_lvis_eval_cpu.py).  Parity with
the published `lvis` package is UNPINNED: that package is no dependency of this project and no test runs the two side by side.

    cut                      per picture, the detections in descending score keep the first MAX_DETS = 300 (over ALL categories); the
                             sort is stable, ties stay in table order (`limit_dets`)
    federated filter         pos(img) = the categories with a ground truth in the picture.  A detection whose category is in neither
                             pos(img) nor neg_category_ids(img) is DROPPED: it produces no row and is counted nowhere
    iou                      pycocotools mask.iou with iscrowd = 0 for every ground truth: instance_eval.rle_iou without the crowd branch.
                             LVIS has no crowds: a ground truth with iscrowd != 0 is an input error (flag 4)
    ground-truth ignore      per area range a: the annotation's `ignore`, or its area < rng[0] or > rng[1] (COCO's four ranges).  The caller
                             encodes an `ignore` ground truth as outside bits 0b1111 in gt_rows[..][2]; it is no crowd: it can be matched
                             once, at its plain IoU
    walk                     detections of a category in descending score; ground truths non-ignored first, each group in annotation order;
                             best = min(t, 1 - 1e-10); a matched ground truth is skipped; the walk stops at the first ignored ground truth
                             once a non-ignored match is held; iou < best is skipped; on equal IoU the later ground truth wins; a matched
                             detection takes the ignore bit of its ground truth
    unmatched detection      ignored in range a when its area (the pixels of its mask) lies outside a, OR when its category is in
                             not_exhaustive_category_ids(img) - the second in every range
    accumulate               per category k and range a, all rows of k over all pictures by argsort(-score, kind="mergesort") in picture
                             order (`image`, then arrival); no further cut.  npig[k][a] = the non-ignored ground truths; where it is <= 0
                             every cell of (k, a) is -1.  tp / fp inclusive counts, rc = tp / npig, pr = tp / (fp + tp + np.spacing(1)),
                             pr replaced by its right-to-left running maximum, precision[t][r][k][a] = pr[searchsorted(rc, rec_thrs[r],
                             "left")] or 0 past the end (a category with ground truth and no detections), recall[t][k][a] = the last rc,
                             0 without rows.  precision [10][101][K][4], recall [10][K][4]
    summarize                every number is mean(s[s > -1]), -1 when nothing is above -1: AP (all t, range all), AP50, AP75, APs / APm / APl
                             (ranges 1..3), APr / APc / APf (AP over the categories of frequency "r" / "c" / "f"), AR@300, ARs / ARm / ARl@300
    results                  detectron2's dict for "segm": AP, AP50, AP75, APs, APm, APl, APr, APc, APf, each times 100

The row record, the thresholds, the masks, the IoU and the ground-truth table are instance_eval's.  Scope: iouType "segm"; LVIS "bbox" and
"boundary" are not part of this.

Front door: `python -m odise_amd.lvis_eval --results lvis_instances_results.json --gt lvis_val.json [--device cpu]`.
"""
from __future__ import annotations

import argparse
import json
import sys
from typing import Dict, Optional, Sequence

import numpy as np

from . import coco_poly
from . import instance_eval as IE

MAX_DETS = 300                      # LVISEval.params.max_dets: per picture, over all categories
MAX_GT = IE.MAX_GT
FREQUENCIES = ("r", "c", "f")       # rare, common, frequent
IGNORE_BITS = 0b1111                # gt_rows[..][2] of a ground truth whose annotation carries `ignore`
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")
FLAG_NAMES = dict(IE.FLAG_NAMES)
FLAG_NAMES[IE.FLAG_BAD_GT] = ("a ground-truth category is outside [0, num_categories), iscrowd is not 0 (LVIS has no crowds), or a ground "
                              "truth has both runs and polygons")


def flag_names(flags: int) -> list:
    return [name for bit, name in FLAG_NAMES.items() if flags & bit]


# ---- the cut and the ground truth -------------------------------------------------------------------------------------------------------
def limit_dets(scores, max_dets: int = MAX_DETS) -> np.ndarray:
    """The table indices of the detections a picture keeps: descending score, stable, the first max_dets (LVISResults.limit_dets_per_image)."""
    return np.argsort(-np.asarray(scores, np.float32).reshape(-1), kind="mergesort")[:max_dets]


def gt_rows(annotations, to_contiguous: Dict[int, int], polygons: bool = False, hw=None):
    """instance_eval.gt_rows with LVIS' `ignore`: a ground truth whose annotation sets it is outside every range (IGNORE_BITS)."""
    out = IE.gt_rows(annotations, to_contiguous, polygons, hw)
    for i, ann in enumerate(annotations):
        if ann.get("ignore", 0):
            out[0][i, 2] = IGNORE_BITS
    return out


def category_bits(category_ids, K: int) -> np.ndarray:
    """uint32 [ceil(K / 32)]: bit k % 32 of word k / 32 stands for contiguous category k (the bitsets of odise_hip_lvis_eval)."""
    bits = np.zeros((K + 31) // 32, np.uint32)
    for k in category_ids:
        assert 0 <= int(k) < K, (k, K)
        bits[int(k) >> 5] |= np.uint32(1 << (int(k) & 31))
    return bits


def npig(rows, K: int) -> np.ndarray:
    """int64 [K, 4]: the ground truths of a category that are not ignored in range a (`ignore` unset, area inside)."""
    out = np.zeros((K, 4), np.int64)
    for cat, _, outside in np.asarray(rows, np.int64).reshape(-1, 3):
        for a in range(4):
            if not (outside >> a) & 1:
                out[cat, a] += 1
    return out


# ---- evaluate_img -----------------------------------------------------------------------------------------------------------------------
def image_rows(masks, scores, classes, gt_counts, gt_table, neg_category_ids=(), not_exhaustive_category_ids=(), image: int = 0,
               iou_thrs=IE.IOU_THRS, num_categories=None):
    """LVISEval.evaluate_img of one picture for all categories, ranges and thresholds -> (rows IE.ROW_DTYPE [kept] in descending score,
    flags).  masks [n, h, w] (nonzero = 1) with scores [n] and classes [n] (contiguous ids); more than MAX_DETS are cut here (`limit_dets`).
    gt_counts: the run lengths of every ground truth; gt_table: `gt_rows`' table; neg_category_ids / not_exhaustive_category_ids: the
    picture's two lists as contiguous ids.  A picture that raises a flag (instance_eval's 1 / 2 / 4, 4 also for iscrowd != 0) has no rows."""
    d = np.asarray(masks) != 0
    scores, classes = np.asarray(scores, np.float32).reshape(-1), np.asarray(classes, np.int64).reshape(-1)
    assert len(scores) >= len(d) and len(classes) >= len(d)
    cut = limit_dets(scores[:len(d)])
    d, scores, classes = d[cut], scores[cut], classes[cut]          # descending score from here on
    n, h, w = d.shape
    table = np.asarray(gt_table, np.int64).reshape(-1, 3)
    n_gt = len(table)
    assert n <= MAX_DETS and n_gt <= MAX_GT and len(gt_counts) == n_gt
    flags = 0
    if any(int(np.asarray(c, np.int64).sum()) != h * w for c in gt_counts):
        flags |= IE.FLAG_BAD_RUNS
    flags |= IE._table_flags(n, classes, table, num_categories)
    if n_gt and (table[:, 1] != 0).any():
        flags |= IE.FLAG_BAD_GT
    if flags:
        return np.zeros(0, IE.ROW_DTYPE), flags
    neg, not_exhaustive = {int(k) for k in neg_category_ids}, {int(k) for k in not_exhaustive_category_ids}
    pos = {int(c) for c in table[:, 0]}
    keep = [i for i in range(n) if int(classes[i]) in pos or int(classes[i]) in neg]       # the federated filter
    ious = IE.mask_iou(d, gt_counts)                                                       # iscrowd = 0 for every ground truth
    areas = d.reshape(n, h * w).sum(1)
    rows = np.zeros(len(keep), IE.ROW_DTYPE)
    where = {i: k for k, i in enumerate(keep)}
    for k, i in enumerate(keep):
        rows[k] = (scores[i], classes[i], areas[i], image, 0, 0)
    for c in sorted({int(classes[i]) for i in keep}):
        dt = [i for i in keep if classes[i] == c]
        gt_c = [j for j in range(n_gt) if table[j, 0] == c]
        for a in range(4):
            ignore = [bool((table[j, 2] >> a) & 1) for j in gt_c]
            gtind = np.argsort(np.asarray(ignore, np.int64), kind="mergesort") if gt_c else []
            gt = [gt_c[g] for g in gtind]
            gt_ig = [ignore[g] for g in gtind]
            for t, thr in enumerate(iou_thrs):
                gtm = [False] * len(gt)
                for i in dt:
                    iou = min(float(thr), 1 - 1e-10)
                    m = -1
                    for gind, j in enumerate(gt):
                        if gtm[gind]:                                   # already matched
                            continue
                        if m > -1 and not gt_ig[m] and gt_ig[gind]:     # a regular match is held and only ignored ones follow
                            break
                        if ious[i, j] < iou:
                            continue
                        iou = ious[i, j]
                        m = gind
                    bit = np.uint64(1 << (10 * a + t))
                    if m > -1:
                        gtm[m] = True
                        rows["matched"][where[i]] |= bit
                        ig = gt_ig[m]
                    else:
                        ig = IE.area_outside(int(areas[i]), a) or c in not_exhaustive
                    if ig:
                        rows["ignored"][where[i]] |= bit
    return rows, 0


# ---- accumulate / summarize -------------------------------------------------------------------------------------------------------------
def accumulate(rows, npig_ka, K: int, rec_thrs=IE.REC_THRS):
    """LVISEval.accumulate -> (precision [T, R, K, A], recall [T, K, A]), -1 where a (category, range) has no non-ignored ground truth.
    rows: IE.ROW_DTYPE of any number of pictures, every picture's rows in descending score; they are ordered by `image` first (stable),
    so the result does not depend on how the pictures were sharded."""
    rows = np.asarray(rows, IE.ROW_DTYPE).reshape(-1)
    rows = rows[np.argsort(rows["image"], kind="stable")]
    npig_ka = np.asarray(npig_ka, np.int64).reshape(K, 4)
    rec_thrs = np.asarray(rec_thrs, np.float64).reshape(-1)
    T, R, A = len(IE.IOU_THRS), len(rec_thrs), 4
    precision, recall = -np.ones((T, R, K, A)), -np.ones((T, K, A))
    for k in range(K):
        rk = rows[rows["category"] == k]
        rk = rk[np.argsort(-rk["score"], kind="mergesort")]
        for a in range(A):
            n_pos = int(npig_ka[k, a])
            if n_pos <= 0:
                continue
            for t in range(T):
                bit = np.uint64(10 * a + t)
                dtm = ((rk["matched"] >> bit) & np.uint64(1)).astype(bool)
                dt_ig = ((rk["ignored"] >> bit) & np.uint64(1)).astype(bool)
                tp = np.cumsum(dtm & ~dt_ig).astype(np.float64)
                fp = np.cumsum(~dtm & ~dt_ig).astype(np.float64)
                nd = len(tp)
                rc = tp / n_pos
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, k, a] = rc[-1] if nd else 0
                pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr        # the right-to-left running maximum
                q = np.zeros(R)
                inds = np.searchsorted(rc, rec_thrs, side="left")
                ok = inds < nd                                                   # entries past the end stay 0
                q[ok] = pr[inds[ok]]
                precision[t, :, k, a] = q
    return precision, recall


def summarize(precision, recall, frequencies: Sequence[str]) -> np.ndarray:
    """LVISEval.summarize -> the 13 numbers of STAT_NAMES; frequencies: "r", "c" or "f" per contiguous category."""
    assert len(frequencies) == precision.shape[2] and set(frequencies) <= set(FREQUENCIES), (len(frequencies), precision.shape)
    t50, t75 = int(np.flatnonzero(np.isclose(IE.IOU_THRS, .5))[0]), int(np.flatnonzero(np.isclose(IE.IOU_THRS, .75))[0])
    s = np.zeros(len(STAT_NAMES))
    s[0] = IE._mean_valid(precision[:, :, :, 0])
    s[1] = IE._mean_valid(precision[t50:t50 + 1, :, :, 0])
    s[2] = IE._mean_valid(precision[t75:t75 + 1, :, :, 0])
    for i, a in enumerate((1, 2, 3)):
        s[3 + i] = IE._mean_valid(precision[:, :, :, a])
        s[10 + i] = IE._mean_valid(recall[:, :, a])
    for i, f in enumerate(FREQUENCIES):
        ks = np.asarray([k for k, fk in enumerate(frequencies) if fk == f], np.int64)
        s[6 + i] = IE._mean_valid(precision[:, :, ks, 0])
    s[9] = IE._mean_valid(recall[:, :, 0])
    return s


def results(precision, recall, frequencies: Sequence[str]) -> dict:
    """detectron2 _evaluate_predictions_on_lvis for "segm": AP, AP50, AP75, APs, APm, APl, APr, APc, APf, each times 100 (an empty group is
    -1 times 100)."""
    s = summarize(precision, recall, frequencies)
    return {name: float(s[i] * 100) for i, name in enumerate(STAT_NAMES[:9])}


# ---- the front door ---------------------------------------------------------------------------------------------------------------------
def _counts(seg, h: int, w: int) -> np.ndarray:
    """Uncompressed counts of a segmentation: an RLE dict (compressed or uncompressed counts) or a list of polygons."""
    return IE.annotation_counts(seg) if isinstance(seg, dict) else coco_poly.annotation_to_counts(seg, h, w)


def evaluate_files(results_path: str, gt_path: str, device: str = "cpu", ctx=None) -> dict:
    """-> {"stats": the 13 numbers of STAT_NAMES, "results": detectron2's dict, "flags"} of an LVIS results file (image_id, category_id,
    score, segmentation = RLE) against an LVIS annotation file (images with neg_category_ids / not_exhaustive_category_ids, categories
    with `frequency`).  device "cpu": this module alone; "gpu": HipLvisEvaluator on U8 masks decoded here, on `ctx` (None: the
    process-wide context)."""
    with open(gt_path) as f:
        gt = json.load(f)
    with open(results_path) as f:
        res = json.load(f)
    cats = sorted(gt["categories"], key=lambda c: c["id"])
    to_contiguous = {int(c["id"]): k for k, c in enumerate(cats)}
    names = [str(c.get("name", c["id"])) for c in cats]
    freqs = [str(c["frequency"]) for c in cats]
    K = len(cats)
    images = sorted(gt["images"], key=lambda im: im["id"])
    gt_by, dt_by = {}, {}
    for a in gt["annotations"]:
        gt_by.setdefault(a["image_id"], []).append(a)
    for r in res:
        dt_by.setdefault(r["image_id"], []).append(r)
    ev = None
    if device != "cpu":
        from .lvis_seg_eval import HipLvisEvaluator
        from .runtime import default_context
        ev = HipLvisEvaluator(ctx if ctx is not None else default_context(), to_contiguous, names, freqs)
    all_rows, npig_ka, flags = [], np.zeros((K, 4), np.int64), 0
    for ii, im in enumerate(images):
        h, w = int(im["height"]), int(im["width"])
        anns, dts = gt_by.get(im["id"], []), dt_by.get(im["id"], [])
        dts = [dts[i] for i in limit_dets([float(r["score"]) for r in dts])]
        scores = np.asarray([float(r["score"]) for r in dts], np.float32)
        classes = np.asarray([to_contiguous[int(r["category_id"])] for r in dts], np.int32)
        masks = np.zeros((len(dts), h, w), np.uint8)
        for i, r in enumerate(dts):
            masks[i] = IE.decode_runs(_counts(r["segmentation"], h, w), h, w)
        neg, nex = im.get("neg_category_ids", []), im.get("not_exhaustive_category_ids", [])
        if ev:
            ev.process_masks(masks, scores, classes, anns, neg, nex, ii)
        else:
            table = gt_rows(anns, to_contiguous, polygons=True, hw=(h, w))[0]
            npig_ka += npig(table, K)
            rows, fl = image_rows(masks, scores, classes, [_counts(a["segmentation"], h, w) for a in anns], table,
                                  [to_contiguous[int(c)] for c in neg], [to_contiguous[int(c)] for c in nex], ii, num_categories=K)
            flags |= fl
            all_rows.append(rows)
    if ev:
        out = ev.evaluate()["segm"]
        precision, recall = ev.precision, ev.recall
    else:
        if flags:
            raise RuntimeError("lvis evaluation: malformed input(s): " + "; ".join(flag_names(flags)))
        rows = np.concatenate(all_rows) if all_rows else np.zeros(0, IE.ROW_DTYPE)
        precision, recall = accumulate(rows, npig_ka, K)
        out = results(precision, recall, freqs)
    return {"stats": summarize(precision, recall, freqs), "results": out, "flags": flags}


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m odise_amd.lvis_eval", description="LVIS segm AP of a results file against an annotation file")
    ap.add_argument("--results", required=True, help="LVIS results json: image_id, category_id, score, segmentation (RLE)")
    ap.add_argument("--gt", required=True, help="LVIS annotation json")
    ap.add_argument("--device", default="gpu", choices=("gpu", "cpu"), help="cpu: the numpy specification alone")
    args = ap.parse_args(argv)
    out = evaluate_files(args.results, args.gt, args.device)
    for name, v in zip(STAT_NAMES, out["stats"]):
        print(f"{name} {float(v):.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
