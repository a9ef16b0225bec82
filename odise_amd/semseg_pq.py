"""Panoptic quality of a semantic segmentation: the specification of `Context.semantic_pq` (csrc/sem_pq.hip) and the front door of the
metric of Mask2Former's tools/evaluate_pq_for_semantic_segmentation.py - the one PQ number of the semantic-only evaluation sets.

The tool scores a label map with panopticapi's rules by reading every class of a picture as ONE stuff segment on either side:

    ground truth   a segment per value of np.unique(gt) other than VOID = ignore_label: id = category = the class, area = its pixels, no crowds
    prediction     a segment per value of np.unique(pred): id = category = the class; a category outside [0, K) is an error there (flag 1
                   here: the picture adds nothing)
    candidates     pairs (g, p) of the (gt, pred) co-occurrence map with both ids among the segments and equal categories, i.e. g == p
    matching       union = area_pred[p] + area_gt[g] - inter - inter[VOID, p]; iou = inter / union; iou > 0.5: tp[cat] += 1, iou[cat] += iou
    fn             every ground-truth segment that was not matched
    fp             every predicted segment that was not matched, unless inter[VOID, p] / area_pred[p] > 0.5
    result         PQStat.pq_average over all K classes with isthing False for each: the rows "All" and "Stuff" are equal

`image_stats_literal` is that, with dictionaries and loops.  Only the diagonal pairs can match, so a picture is a function of four
integer vectors of length K - `image_counts` - and `image_stats` is the rule on them, the form the device computes.  At most one pair per
class and picture matches: iou[c] grows by one addend per picture, and a stream of pictures accumulated in order is bit-identical
between the three.

Ground truth comes in two forms.  The tool's: raw values with `ignore_label`, every other value a class in [0, K) (a value that is
neither would be a segment of an unknown category there; it must not occur).  The device's (`HipSemSegEvaluator`'s contract): int32 with
the ignore label mapped to K, and anything outside [0, K] counts as K.  `map_ignore` turns the first into the second.

    python -m odise_amd.semseg_pq --json-file sem_seg_predictions.json --gt-dir DIR --num-classes K --ignore-label L [--gt-ext .png]

prints the tool's table from a predictions file and a directory of ground-truth label images.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np

from . import coco_rle
from .panoptic_quality import PQStats, pq_average

FLAG_BAD_LABEL = 1          # semseg_eval.FLAG_NAMES: a predicted label outside [0, num_classes)
OFFSET = 2 ** 24
AREA_PRED, AREA_GT, INTER, VOID_PRED = range(4)


def map_ignore(gt, K: int, ignore_label: int) -> np.ndarray:
    """The annotation as the device takes it: int32, ignore_label -> K (everything else unchanged)."""
    g = np.asarray(gt).astype(np.int64)
    return np.where(g == int(ignore_label), K, g).astype(np.int32)


def pred_flags(pred, K: int) -> int:
    p = np.asarray(pred)
    return FLAG_BAD_LABEL if ((p < 0) | (p >= K)).any() else 0


def image_stats_literal(pred, gt, K: int, ignore_label: int, into: Optional[PQStats] = None):
    """One picture the way the tool computes it.  pred: labels in [0, K); gt: classes in [0, K) or ignore_label.  -> (PQStats, flags); a
    picture with a flag adds nothing.  `into`: the statistics of the pictures so far, added to (and returned)."""
    stats = into if into is not None else PQStats(K)
    assert len(stats) == K
    void = int(ignore_label)
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    assert pred.shape == gt.shape
    ids, cnt = np.unique(gt, return_counts=True)
    gt_segments = {int(i): {"category": int(i), "area": int(c)} for i, c in zip(ids, cnt) if int(i) != void}
    assert all(0 <= s["category"] < K for s in gt_segments.values()), "a ground-truth value that is neither a class nor the ignore label"
    ids, cnt = np.unique(pred, return_counts=True)
    pred_segments = {int(i): {"category": int(i), "area": int(c)} for i, c in zip(ids, cnt)}
    if any(not 0 <= s["category"] < K for s in pred_segments.values()):
        return stats, FLAG_BAD_LABEL

    keys, cnt = np.unique(gt * OFFSET + pred, return_counts=True)
    pair_map = {(int(k) // OFFSET, int(k) % OFFSET): int(c) for k, c in zip(keys, cnt)}

    gt_matched, pred_matched = set(), set()
    for (g, p), inter in pair_map.items():
        if g not in gt_segments or p not in pred_segments:
            continue
        if gt_segments[g]["category"] != pred_segments[p]["category"]:
            continue
        union = pred_segments[p]["area"] + gt_segments[g]["area"] - inter - pair_map.get((void, p), 0)
        iou = inter / union
        if iou > 0.5:
            stats.tp[gt_segments[g]["category"]] += 1
            stats.iou[gt_segments[g]["category"]] += iou
            gt_matched.add(g)
            pred_matched.add(p)
    for g, seg in gt_segments.items():
        if g not in gt_matched:
            stats.fn[seg["category"]] += 1
    for p, seg in pred_segments.items():
        if p in pred_matched:
            continue
        if pair_map.get((void, p), 0) / seg["area"] > 0.5:
            continue
        stats.fp[seg["category"]] += 1
    return stats, 0


def image_counts(pred, gt, K: int) -> np.ndarray:
    """int64 [4, K]: area_pred, area_gt, inter, void_pred of one picture.  gt in the device's form (outside [0, K] counts as K = VOID);
    a predicted label outside [0, K) is counted in no row."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    gt = np.asarray(gt).astype(np.int64).reshape(-1)
    assert pred.shape == gt.shape
    gt = np.where((gt < 0) | (gt > K), K, gt)
    ok = (pred >= 0) & (pred < K)
    out = np.zeros((4, K), np.int64)
    out[AREA_PRED] = np.bincount(pred[ok], minlength=K)
    out[AREA_GT] = np.bincount(gt[gt < K], minlength=K)
    out[INTER] = np.bincount(pred[ok & (pred == gt)], minlength=K)
    out[VOID_PRED] = np.bincount(pred[ok & (gt == K)], minlength=K)
    return out


def image_stats(counts, into: Optional[PQStats] = None) -> PQStats:
    """The rule on the four vectors: what one picture adds, class by class."""
    counts = np.asarray(counts, np.int64)
    K = counts.shape[1]
    stats = into if into is not None else PQStats(K)
    assert counts.shape == (4, K) and len(stats) == K
    for c in np.flatnonzero(counts[AREA_PRED] + counts[AREA_GT]):
        area_pred, area_gt, inter, void_pred = (int(v) for v in counts[:, c])
        if inter > 0:
            iou = inter / (area_pred + area_gt - inter - void_pred)
            if iou > 0.5:
                stats.tp[c] += 1
                stats.iou[c] += iou
                continue
        if area_gt > 0:
            stats.fn[c] += 1
        if area_pred > 0 and not void_pred / area_pred > 0.5:
            stats.fp[c] += 1
    return stats


def picture_stats(pred, gt, K: int, into: Optional[PQStats] = None):
    """What `Context.semantic_pq` adds for one picture (gt in the device's form) -> (PQStats, flags); a flagged picture adds nothing."""
    stats = into if into is not None else PQStats(K)
    flags = pred_flags(pred, K)
    if not flags:
        image_stats(image_counts(pred, gt, K), into=stats)
    return stats, flags


def per_class(stats: PQStats) -> list:
    """panopticapi's per-class rows: pq = iou / (tp + fp / 2 + fn / 2), sq = iou / tp, rq = tp / (tp + fp / 2 + fn / 2); zeros for a class
    without a sample."""
    rows = []
    for c in range(len(stats)):
        iou, tp, fp, fn = float(stats.iou[c]), int(stats.tp[c]), int(stats.fp[c]), int(stats.fn[c])
        if tp + fp + fn == 0:
            rows.append({"pq": 0.0, "sq": 0.0, "rq": 0.0})
            continue
        den = tp + 0.5 * fp + 0.5 * fn
        rows.append({"pq": iou / den, "sq": iou / tp if tp != 0 else 0, "rq": tp / den})
    return rows


def results(stats: PQStats) -> dict:
    """The tool's table: {"All": {pq, sq, rq, n}, "Stuff": the same (every class is a stuff class), "per_class": [K] rows}."""
    isthing = [False] * len(stats)
    return {"All": pq_average(stats, isthing, "all"), "Stuff": pq_average(stats, isthing, "stuff"), "per_class": per_class(stats)}


def evaluator_results(stats: PQStats, class_names: Sequence[str]) -> "OrderedDict[str, float]":
    """The keys `HipSemSegEvaluator(pq=True)` appends: PQ, SQ, RQ, then PQ-<name> per class; everything times 100."""
    assert len(class_names) == len(stats)
    table = results(stats)
    res = OrderedDict((k.upper(), 100 * float(table["All"][k])) for k in ("pq", "sq", "rq"))
    for name, row in zip(class_names, table["per_class"]):
        res[f"PQ-{name}"] = 100 * float(row["pq"])
    return res


def tool_miou(conf) -> float:
    """The mIoU the tool prints from its confusion matrix (rows = prediction, the last row / column = the ignore label): tp / union summed
    over the classes that occur in the ground truth, divided by the number of classes that occur on EITHER side."""
    conf = np.asarray(conf, np.int64)
    tp = conf.diagonal()[:-1].astype(np.float64)
    pos_gt = conf[:-1, :-1].sum(axis=0).astype(np.float64)
    pos_pred = conf[:-1, :-1].sum(axis=1).astype(np.float64)
    in_gt = pos_gt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sum(tp[in_gt] / (pos_gt + pos_pred - tp)[in_gt]) / np.sum((pos_gt + pos_pred) > 0))


def format_table(table: dict) -> str:
    """Four lines: a header, a rule, and the rows All and Stuff with PQ / SQ / RQ in percent to one decimal and the class count N."""
    head = f"{'':10s}| {'PQ':>5s}  {'SQ':>5s}  {'RQ':>5s} {'N':>5s}"
    lines = [head, "-" * 38]                                                          # the tool's rule is one dash longer than its header
    for name in ("All", "Stuff"):
        pq, sq, rq = (100 * float(table[name][k]) for k in ("pq", "sq", "rq"))
        lines.append(f"{name:10s}| {pq:5.1f}  {sq:5.1f}  {rq:5.1f} {int(table[name]['n']):5d}")
    return "\n".join(lines)


# ---- the front door: sem_seg_predictions.json + a directory of ground-truth label images -----------------------------------------------
def group_rows(rows) -> "OrderedDict[str, list]":
    """The prediction rows of every picture, keyed by file stem (the base name up to its first dot), pictures and rows in file order."""
    out = OrderedDict()
    for r in rows:
        out.setdefault(os.path.basename(r["file_name"]).split(".")[0], []).append(r)
    return out


def paint(rows, hw, to_contiguous: Optional[dict] = None) -> np.ndarray:
    """int32 [h, w] label map of one picture: zeros, then every row's mask painted with its class in row order (a later row wins).
    to_contiguous: dataset category id -> class, for files written with dataset ids; an id outside the mapping is kept as it is."""
    out = np.zeros(hw, np.int32)
    for r in rows:
        cat = int(r["category_id"])
        if to_contiguous is not None:
            cat = int(to_contiguous.get(cat, cat))
        mask = coco_rle.decode(r["segmentation"])
        assert mask.shape == tuple(hw), (mask.shape, hw)
        out[mask > 0] = cat
    return out


def read_label_image(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).astype(np.int64)


def evaluate_file(ctx, json_file: str, gt_dir: str, K: int, ignore_label: int, gt_ext: str = ".png", to_contiguous: Optional[dict] = None):
    """-> (PQStats summed over the pictures of the file in file order, confusion matrix int64 [(K+1), (K+1)]).  Every picture goes through
    `Context.semantic_pq`; the painting and the confusion matrix of the mIoU line stay on the host."""
    from .panoptic_quality import STAT_DTYPE
    from .semseg_eval import confusion, flag_names
    with open(json_file) as f:
        groups = group_rows(json.load(f))
    stats, flags = ctx.zeros((K,), STAT_DTYPE), ctx.zeros((1,), np.int32)
    conf = np.zeros((K + 1, K + 1), np.int64)
    for stem, rows in groups.items():
        gt = map_ignore(read_label_image(os.path.join(gt_dir, stem + gt_ext)), K, ignore_label)
        pred = paint(rows, gt.shape, to_contiguous)
        ctx.semantic_pq(ctx.to_device(pred), gt=ctx.to_device(gt), K=K, stats=stats, flags=flags)
        if not pred_flags(pred, K):
            conf += confusion(pred, gt, K)
    seen = int(flags.numpy()[0])
    if seen:
        raise RuntimeError("semantic PQ: malformed prediction(s): " + "; ".join(flag_names(seen)))
    return PQStats.from_records(stats.numpy()), conf


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(description="PQ of a semantic segmentation (sem_seg_predictions.json against label images), counted on the device.")
    ap.add_argument("--json-file", required=True, help="sem_seg_predictions.json as HipSemSegEvaluator / SemSegEvaluator write it")
    ap.add_argument("--gt-dir", required=True, help="directory of the ground-truth label images, <file stem><gt-ext>")
    ap.add_argument("--num-classes", type=int, required=True)
    ap.add_argument("--ignore-label", type=int, required=True)
    ap.add_argument("--gt-ext", default=".png")
    ap.add_argument("--id-map", default=None, help="JSON object {dataset category id: class} for files written with dataset ids")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    from .runtime import Context
    to_contiguous = None
    if args.id_map:
        with open(args.id_map) as f:
            to_contiguous = {int(k): int(v) for k, v in json.load(f).items()}
    ctx = Context(args.device)
    try:
        stats, conf = evaluate_file(ctx, args.json_file, args.gt_dir, args.num_classes, args.ignore_label, args.gt_ext, to_contiguous)
    finally:
        ctx.close()
    print(format_table(results(stats)))
    print("")
    print(f"mIoU: {tool_miou(conf)}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
