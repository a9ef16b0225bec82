"""Host restatement of the panoptic quality statistics (numpy): the reference of `Context.panoptic_quality` (csrc/pq.hip) and the metric
arithmetic of COCOPanopticEvaluator.evaluate, which stays on the host.

`image_stats` is panopticapi's `pq_compute_single_core` for one picture, written the way it is written there - `np.unique` over
`gt * 2**24 + pred`, dictionaries and Python loops - with the cases in which that code raises turned into flags.  The rule stands once, in
`_image_stats`; `image_stats` and `image_boundary_stats` both call it, the second with its boundary counts:

    pred area of a segment   its pixels in the predicted map
    inter[g, p]              pixels with ground-truth id g and predicted id p; VOID is id 0 on both sides
    matching                 pairs in ascending (g, p) order with both ids in their tables, iscrowd[g] == 0 and equal categories:
                             union = area_pred[p] + area_gt[g] - inter[g, p] - inter[VOID, p]   (area_gt from the annotation JSON),
                             iou = inter / union (a union <= 0 matches nothing; the reference would divide by it), iou > 0.5: tp, iou
    false negatives          unmatched table rows in table order: a crowd row becomes crowd_of[category] (the last one wins) and counts
                             nothing, every other row counts fn
    false positives          unmatched predictions: skipped when (inter[VOID, p] + inter[crowd_of[cat_p], p]) / area_pred[p] > 0.5

Ids are 24-bit values, as in the PNG files; in a table the first row of an id is the one its pixels belong to (a later row of the same
id, or a row of id 0, has no pixels).

Boundary PQ (`image_boundary_stats`, the reference of `Context.panoptic_quality_boundary`) is the third metric of Cheng et al., "Boundary
IoU" (CVPR 2021): PQ with min(mask IoU, boundary IoU) in place of the mask IoU, both for the match (> 0.5) and for the SQ sum.  This is the
project's restatement of the paper's rule on `pq_compute_single_core`; PARITY WITH THE PUBLISHED boundary-iou PACKAGE IS UNPINNED (the
package was never run beside it).

    radius                   sem_boundary.boundary_radius(H, W) unless the caller gives radius > 0: as the other two boundary measures
    boundary B(s)            the segment's pixels minus their erosion (r 3x3 erosions behind a ring of zeros: the binary
                             instance_eval.mask_boundary of its mask); a pixel of s lies in B(s) when its (2r+1)^2 window leaves the
                             picture or holds a pixel that is not of s.  VOID and ids missing from a table are neighbours like any other
                             and have no boundary of their own that anyone reads; with 2r+1 > min(H, W) every pixel is a boundary pixel
    boundary IoU of (g, p)   the candidates are those of PQ; inter_b = |B(g) & B(p)|,
                             union_b = |B(p)| + |B(g)| - inter_b - |B(p) over ground-truth VOID|  (|B(g)| is counted from the map: the
                             JSON holds no boundary area), b_iou = inter_b / union_b, 0 when union_b <= 0
    matching                 iou_b = min(iou, b_iou) with iou exactly as above (JSON area included); iou_b > 0.5: tp, iou_b - added in
                             ascending (g, p) order onto the running sum
    fn, fp                   follow from this matching by the unchanged rules; the fp skip test still uses mask areas, VOID and the crowd row
    flags                    the same three; a flagged picture adds nothing to either accumulator
"""
from __future__ import annotations

from typing import Sequence

import numpy as np

VOID = 0
OFFSET = 2 ** 24
MAX_GT_SEGMENTS = 254
FLAG_MISSING_ID, FLAG_EMPTY_ROW, FLAG_BAD_CATEGORY = 1, 2, 4
FLAG_NAMES = {FLAG_MISSING_ID: "a predicted id of the map is missing from segments_info",
              FLAG_EMPTY_ROW: "a segments_info row of the prediction has no pixel",
              FLAG_BAD_CATEGORY: "a predicted category is outside [0, num_categories)"}
# odise_pq_stat (include/odise_hip.h)
STAT_DTYPE = np.dtype([("iou", "<f8"), ("tp", "<i8"), ("fp", "<i8"), ("fn", "<i8")])


def rgb2id(rgb: np.ndarray) -> np.ndarray:
    """uint8 [..., 3] as Pillow decodes a panoptic PNG -> int32 ids R + 256 G + 65536 B."""
    rgb = np.asarray(rgb).astype(np.int32)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


class PQStats:
    """(iou, tp, fp, fn) per category; `+` adds category by category (left operand first, which fixes the order of the iou sums)."""

    def __init__(self, num_categories: int):
        self.iou = np.zeros(num_categories, np.float64)
        self.tp = np.zeros(num_categories, np.int64)
        self.fp = np.zeros(num_categories, np.int64)
        self.fn = np.zeros(num_categories, np.int64)

    @classmethod
    def from_records(cls, rec: np.ndarray) -> "PQStats":
        rec = np.asarray(rec, STAT_DTYPE).reshape(-1)
        s = cls(rec.shape[0])
        s.iou[:], s.tp[:], s.fp[:], s.fn[:] = rec["iou"], rec["tp"], rec["fp"], rec["fn"]
        return s

    def to_records(self) -> np.ndarray:
        rec = np.zeros(len(self), STAT_DTYPE)
        rec["iou"], rec["tp"], rec["fp"], rec["fn"] = self.iou, self.tp, self.fp, self.fn
        return rec

    def __len__(self) -> int:
        return self.iou.shape[0]

    def __add__(self, other: "PQStats") -> "PQStats":
        assert len(self) == len(other), (len(self), len(other))
        out = PQStats(len(self))
        out.iou, out.tp, out.fp, out.fn = self.iou + other.iou, self.tp + other.tp, self.fp + other.fp, self.fn + other.fn
        return out

    def __iadd__(self, other: "PQStats") -> "PQStats":
        assert len(self) == len(other), (len(self), len(other))
        self.iou += other.iou
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        return self

    def __eq__(self, other) -> bool:
        """Counts equal and the iou sums bit for bit."""
        return isinstance(other, PQStats) and self.to_records().tobytes() == other.to_records().tobytes()

    def __repr__(self) -> str:
        k = np.flatnonzero(self.tp + self.fp + self.fn)
        return "PQStats(" + ", ".join(f"{c}: iou {self.iou[c]!r} tp {self.tp[c]} fp {self.fp[c]} fn {self.fn[c]}" for c in k) + ")"


def gt_table(gt_segments) -> np.ndarray:
    """int32 [n_gt, 4] rows (id, category_id, iscrowd, area)."""
    return np.asarray(gt_segments, np.int64).reshape(-1, 4).astype(np.int32)


def _image_stats(pan_gt, gt_segments, pan_pred, pred_segments, C: int, into, trace, boundary=None):
    """The one body of the per-picture rule (the module docstring), behind `image_stats` and `image_boundary_stats`.  `boundary`: None, or
    a function of the two id lists of the tables that returns b_iou(g, p); it is called once a picture has no flag, a candidate then
    counts with min(iou, b_iou(g, p)), and `trace` also receives `demoted` and `lowered`."""
    stats = into if into is not None else PQStats(C)
    assert len(stats) == C
    gt_rows = [tuple(int(v) for v in r) for r in np.asarray(gt_segments, np.int64).reshape(-1, 4)]
    pred_rows = [tuple(int(v) for v in r) for r in np.asarray(pred_segments, np.int64).reshape(-1, 3)]
    pan_gt = np.asarray(pan_gt).astype(np.int64).reshape(-1)
    pan_pred = np.asarray(pan_pred).astype(np.int64).reshape(-1)
    assert pan_gt.shape == pan_pred.shape
    gt_row_of, pred_row_of = {}, {}
    for i, r in enumerate(gt_rows):
        if r[0] != VOID:
            gt_row_of.setdefault(r[0], i)
    for i, r in enumerate(pred_rows):
        if r[0] != VOID:
            pred_row_of.setdefault(r[0], i)

    labels, cnt = np.unique(pan_pred, return_counts=True)
    area_pred = {int(l): int(c) for l, c in zip(labels, cnt)}
    flags = 0
    if any(l != VOID and l not in pred_row_of for l in area_pred):
        flags |= FLAG_MISSING_ID
    if any(pred_row_of.get(r[0]) != i or r[0] not in area_pred for i, r in enumerate(pred_rows)):
        flags |= FLAG_EMPTY_ROW
    if any(not 0 <= r[2] < C for r in pred_rows):
        flags |= FLAG_BAD_CATEGORY
    if flags:
        return stats, flags

    keys, cnt = np.unique(pan_gt * OFFSET + pan_pred, return_counts=True)
    inter = {(int(k) // OFFSET, int(k) % OFFSET): int(c) for k, c in zip(keys, cnt)}
    b_iou_of = boundary(list(gt_row_of), list(pred_row_of)) if boundary is not None else None

    gt_matched, pred_matched = set(), set()
    rejected = demoted = lowered = 0
    for (g, p), n in inter.items():                      # np.unique sorts: ascending (g, p)
        if g not in gt_row_of or p not in pred_row_of:
            continue
        gi, pi = gt_row_of[g], pred_row_of[p]
        _, g_cat, g_crowd, g_area = gt_rows[gi]
        if g_crowd == 1 or g_cat != pred_rows[pi][2]:
            continue
        union = area_pred[p] + g_area - n - inter.get((VOID, p), 0)
        if union <= 0:
            continue
        iou = n / union
        b_iou = b_iou_of(g, p) if b_iou_of is not None else iou
        iou_b = min(iou, b_iou)
        if iou_b > 0.5:
            stats.tp[g_cat] += 1
            stats.iou[g_cat] += iou_b
            gt_matched.add(gi)
            pred_matched.add(pi)
            lowered += b_iou < iou
        else:
            rejected += 1
            demoted += iou > 0.5

    crowd_of = {}
    for gi, (g, g_cat, g_crowd, _) in enumerate(gt_rows):
        if gi in gt_matched:
            continue
        if g_crowd == 1:
            crowd_of[g_cat] = gi
            continue
        stats.fn[g_cat] += 1

    skipped_void = skipped_crowd = 0
    for pi, (p, _, p_cat) in enumerate(pred_rows):
        if pi in pred_matched:
            continue
        void = inter.get((VOID, p), 0)
        ign = void
        if p_cat in crowd_of:
            gi = crowd_of[p_cat]
            if gt_row_of.get(gt_rows[gi][0]) == gi:
                ign += inter.get((gt_rows[gi][0], p), 0)
        if ign / area_pred[p] > 0.5:
            if void / area_pred[p] > 0.5:
                skipped_void += 1
            else:
                skipped_crowd += 1
            continue
        stats.fp[p_cat] += 1
    if trace is not None:
        trace.update(rejected=rejected, skipped_void=skipped_void, skipped_crowd=skipped_crowd)
        if boundary is not None:
            trace.update(demoted=int(demoted), lowered=int(lowered))
    return stats, flags


def image_stats(pan_gt, gt_segments, pan_pred, pred_segments, C: int, trace: dict | None = None, into: PQStats | None = None):
    """One picture.  pan_gt / pan_pred: integer id maps of one shape; gt_segments rows (id, category_id, iscrowd, area); pred_segments rows
    (id, isthing, category_id); categories in 0..C-1 on both sides.  -> (PQStats, flags).  Raises nothing: a picture with a flag adds
    nothing.  `into`: the statistics of the pictures so far, added to pair by pair (and returned) - the way the evaluator's one PQStat
    runs through a stream of pictures, which is not the same floating-point sum as adding per-picture totals.  `trace` (optional dict)
    receives what happened on the way: candidates rejected at iou <= 0.5, false positives skipped through VOID alone and through a crowd
    region."""
    return _image_stats(pan_gt, gt_segments, pan_pred, pred_segments, C, into, trace)


def segment_boundaries(pan, table, radius=None) -> np.ndarray:
    """uint8 [H, W]: 1 where a pixel lies on the boundary B(s) of its own segment, for the segments whose ids `table` lists; pixels of id 0
    and of ids absent from the table are 0.  Literal: one binary mask per id through instance_eval.mask_boundary (the segments are
    disjoint, so their boundaries are too).  radius None (or <= 0): sem_boundary.boundary_radius(H, W)."""
    from .instance_eval import mask_boundary
    pan = np.asarray(pan).astype(np.int64)
    assert pan.ndim == 2, pan.shape
    out = np.zeros(pan.shape, np.uint8)
    for i in dict.fromkeys(int(v) for v in np.asarray(table, np.int64).reshape(-1)):
        if i != VOID:
            out |= mask_boundary((pan == i)[None], radius)[0]
    return out


def image_boundary_stats(pan_gt, gt_segments, pan_pred, pred_segments, C: int, radius=None, into: PQStats | None = None,
                         trace: dict | None = None):
    """`image_stats` with min(iou, boundary iou) in place of iou (the rule: the module docstring).  pan_gt / pan_pred must be [H, W] maps.
    -> (PQStats, flags); `into` as there.  `trace` receives, beside the three counts of `image_stats` (rejected: candidates with
    iou_b <= 0.5), `demoted`, the pairs with iou > 0.5 >= iou_b, and `lowered`, the pairs matched with b_iou < iou."""
    map_gt, map_pred = np.asarray(pan_gt).astype(np.int64), np.asarray(pan_pred).astype(np.int64)
    assert map_gt.ndim == 2 and map_gt.shape == map_pred.shape, (map_gt.shape, map_pred.shape)

    def boundary(gt_ids, pred_ids):
        """The boundary counts of the picture: pixels of B(g), of B(p), of B(p) over VOID, of both -> b_iou(g, p)."""
        pan_gt, pan_pred = map_gt.reshape(-1), map_pred.reshape(-1)
        on_gt = segment_boundaries(map_gt, gt_ids, radius).reshape(-1) != 0
        on_pred = segment_boundaries(map_pred, pred_ids, radius).reshape(-1) != 0
        labels, cnt = np.unique(pan_gt[on_gt], return_counts=True)
        b_area_gt = {int(l): int(c) for l, c in zip(labels, cnt)}
        labels, cnt = np.unique(pan_pred[on_pred], return_counts=True)
        b_area_pred = {int(l): int(c) for l, c in zip(labels, cnt)}
        labels, cnt = np.unique(pan_pred[on_pred & (pan_gt == VOID)], return_counts=True)
        b_void = {int(l): int(c) for l, c in zip(labels, cnt)}
        both = on_gt & on_pred
        keys, cnt = np.unique(pan_gt[both] * OFFSET + pan_pred[both], return_counts=True)
        b_inter = {(int(k) // OFFSET, int(k) % OFFSET): int(c) for k, c in zip(keys, cnt)}

        def b_iou(g, p):
            n_b = b_inter.get((g, p), 0)
            union_b = b_area_pred.get(p, 0) + b_area_gt.get(g, 0) - n_b - b_void.get(p, 0)
            return n_b / union_b if union_b > 0 else 0.0
        return b_iou
    return _image_stats(map_gt, gt_segments, map_pred, pred_segments, C, into, trace, boundary)


def pq_average(stats: PQStats, isthing: Sequence[bool], which: str = "all") -> dict:
    """panopticapi's PQStat.pq_average over the categories of one kind ("all", "things", "stuff") that have a sample (tp + fp + fn > 0):
    pq = iou / (tp + fp / 2 + fn / 2), sq = iou / tp (0 without a tp), rq = tp / (tp + fp / 2 + fn / 2), averaged; `n` = how many.
    Without any such category the averages are 0 (the reference divides by n)."""
    assert which in ("all", "things", "stuff"), which
    assert len(isthing) == len(stats), (len(isthing), len(stats))
    pq = sq = rq = 0.0
    n = 0
    for c in range(len(stats)):
        if which != "all" and bool(isthing[c]) != (which == "things"):
            continue
        iou, tp, fp, fn = float(stats.iou[c]), int(stats.tp[c]), int(stats.fp[c]), int(stats.fn[c])
        if tp + fp + fn == 0:
            continue
        n += 1
        pq += iou / (tp + 0.5 * fp + 0.5 * fn)
        sq += iou / tp if tp != 0 else 0
        rq += tp / (tp + 0.5 * fp + 0.5 * fn)
    return {"pq": pq / n if n else 0.0, "sq": sq / n if n else 0.0, "rq": rq / n if n else 0.0, "n": n}


def results(stats: PQStats, isthing: Sequence[bool]) -> dict:
    """The dict of COCOPanopticEvaluator.evaluate: PQ / SQ / RQ over all, thing (_th) and stuff (_st) categories, times 100."""
    out = {}
    for suffix, which in (("", "all"), ("_th", "things"), ("_st", "stuff")):
        avg = pq_average(stats, isthing, which)
        for k in ("pq", "sq", "rq"):
            out[k.upper() + suffix] = 100 * avg[k]
    return out


def boundary_results(stats: PQStats, isthing: Sequence[bool]) -> dict:
    """`results` of the Boundary PQ statistics (`image_boundary_stats`) under their own names: BPQ / BSQ / BRQ and the _th / _st variants."""
    return {"B" + k: v for k, v in results(stats, isthing).items()}


def flag_names(flags: int) -> list:
    return [f"bit {b.bit_length() - 1}: {FLAG_NAMES[b]}" for b in sorted(FLAG_NAMES) if flags & b]
