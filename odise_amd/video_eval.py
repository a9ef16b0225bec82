"""Host restatement of video instance segmentation AP (YouTube-VIS; numpy): the reference of `Context.video_eval_frame` /
`Context.video_eval_finish` (csrc/video_eval.hip), and `python -m odise_amd.video_eval --results results.json --gt instances.json`.

The evaluator is the one of mask2former_video/data_video/ytvis_eval.py (datasets/ytvis_api/ytvoseval.py), which is COCOeval with two
changes; everything else - thresholds, the row record, the walk, `accumulate`, `summarize`, `results` - is odise_amd/instance_eval.py's,
with a video standing where a picture stands and a track where a detection stands:

    sequence IoU     (computeIoU -> iou_seq) of predicted track d and ground-truth track g over the frames of one video:
                     inter = sum_f |d_f & g_f|, union = sum_f |d_f | g_f|; a frame where only one of the two has a mask adds that mask's
                     area to the union, one where neither has adds nothing.  With A_d, A_g the per-frame pixel counts (0 where absent)
                     iou = inter / (sum A_d + sum A_g - inter), one double division of exact integers, 0 when the denominator is 0.
                     iscrowd does NOT enter the IoU: the reference builds the list and never uses it.
    areas            a predicted track's avg_area is the mean of its non-zero per-frame pixel counts, 0 without one (ytvos.py loadRes);
                     a ground-truth track's is the same mean over the annotation's own `areas` list (the file's floats).
    ranges           [0, 1e10], [0, 128^2], [128^2, 256^2], [256^2, 1e10], ends included.
    walk             evaluateVid is evaluateImg: maxDet 100, descending score in a stable order, non-ignored ground truths first (ignored
                     = crowd or avg_area outside the range), a matched non-crowd ground truth skipped, the stop at the first ignored one
                     once a non-ignored match is held, best = min(t, 1 - 1e-10) moving on >=, an unmatched track ignored when its own
                     avg_area lies outside the range.  The crowd bit acts here only.

The rule is restated from ytvoseval.py and pinned to hand-worked videos (tests/test_video_eval_cpu.py); parity with the reference
evaluator is UNPINNED: pycocotools is no dependency of this project and no test runs the two side by side.

`Counts` is the device's accumulator restated: per-frame sums through slot tables, which is what `sequence_iou` is built on."""
from __future__ import annotations

import argparse
import json
import sys
from typing import Dict, Optional, Sequence

import numpy as np

from . import coco_poly
from . import instance_eval as IE

VIDEO_AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 128 ** 2), (128 ** 2, 256 ** 2), (256 ** 2, 1e5 ** 2))   # ytvoseval.Params.setDetParams
MAX_TRACKS, MAX_GT = IE.MAX_DETECTIONS, IE.MAX_GT
FLAG_BAD_RUNS, FLAG_BAD_CLASS, FLAG_BAD_GT, FLAG_BAD_POLYGON, FLAG_SHARED_SLOT = 1, 2, 4, 8, 16
FLAG_NAMES = {**IE.FLAG_NAMES, FLAG_SHARED_SLOT: "two detections of one frame share a track, or two annotations of one frame share a ground-truth "
                                                 "track: both were added, their union was not formed"}


def flag_names(flags: int) -> list:
    return [name for bit, name in FLAG_NAMES.items() if flags & bit]


# ---- sums -----------------------------------------------------------------------------------------------------------------------------------
class Counts:
    """odise_video_eval_state on the host: inter int64 [max_tracks, max_gt], area_d int64 [max_tracks], area_g int64 [max_gt], frames_d
    int32 [max_tracks]."""

    def __init__(self, max_tracks: int, max_gt: int):
        self.inter = np.zeros((max_tracks, max_gt), np.int64)
        self.area_d, self.area_g = np.zeros(max_tracks, np.int64), np.zeros(max_gt, np.int64)
        self.frames_d = np.zeros(max_tracks, np.int32)

    def add_frame(self, det_masks, det_slot, gt_masks, gt_slot) -> int:
        """One frame (odise_hip_video_eval_frame): det_masks [n, h, w] (nonzero = 1; only the detections below the count of the table)
        with their tracks det_slot [n], gt_masks [m, h, w] with their tracks gt_slot [m]; a slot outside the range is skipped.  Returns
        flag 16 when a slot is used twice on one side (both masks are added all the same), else 0."""
        d, g = np.asarray(det_masks) != 0, np.asarray(gt_masks) != 0
        det_slot, gt_slot = np.asarray(det_slot, np.int64).reshape(-1), np.asarray(gt_slot, np.int64).reshape(-1)
        assert len(det_slot) == len(d) and len(gt_slot) == len(g), (len(det_slot), len(d), len(gt_slot), len(g))
        T, G = self.inter.shape
        ok_d = [i for i in range(len(d)) if 0 <= det_slot[i] < T]
        ok_g = [j for j in range(len(g)) if 0 <= gt_slot[j] < G]
        for i in ok_d:
            a = int(np.count_nonzero(d[i]))
            self.area_d[det_slot[i]] += a
            self.frames_d[det_slot[i]] += 1 if a > 0 else 0
            for j in ok_g:
                self.inter[det_slot[i], gt_slot[j]] += int(np.count_nonzero(d[i] & g[j]))
        for j in ok_g:
            self.area_g[gt_slot[j]] += int(np.count_nonzero(g[j]))
        shared = len(set(det_slot[ok_d].tolist())) < len(ok_d) or len(set(gt_slot[ok_g].tolist())) < len(ok_g)
        return FLAG_SHARED_SLOT if shared else 0

    def iou(self, n_tracks: Optional[int] = None, n_gt: Optional[int] = None) -> np.ndarray:
        """float64 [n_tracks, n_gt]: inter / (area_d + area_g - inter) as one double division of exact integers, 0 where that is 0."""
        n = self.inter.shape[0] if n_tracks is None else n_tracks
        m = self.inter.shape[1] if n_gt is None else n_gt
        out = np.zeros((n, m), np.float64)
        for s in range(n):
            for j in range(m):
                i = int(self.inter[s, j])
                u = int(self.area_d[s]) + int(self.area_g[j]) - i
                out[s, j] = float(np.float64(i) / np.float64(u)) if u != 0 else 0.0
        return out

    def avg_area(self, n_tracks: Optional[int] = None) -> np.ndarray:
        """float64 [n_tracks]: area_d / frames_d, 0 without a frame (the mean of a track's non-zero pixel counts)."""
        n = self.inter.shape[0] if n_tracks is None else n_tracks
        return np.asarray([float(np.float64(self.area_d[s]) / np.float64(self.frames_d[s])) if self.frames_d[s] else 0.0 for s in range(n)], np.float64)


def _frame_masks(tracks, f: int, hw):
    """-> (masks bool [k, h, w] of the tracks that have a mask in frame f, their indices)."""
    idx = [i for i, t in enumerate(tracks) if t[f] is not None]
    m = np.stack([np.asarray(tracks[i][f]) != 0 for i in idx]) if idx else np.zeros((0,) + tuple(hw), bool)
    return m, idx


def sequence_counts(dt_tracks, gt_tracks) -> Counts:
    """The sums of one video: every track is a list of [h, w] arrays (nonzero = 1) or None, one entry per frame."""
    c = Counts(len(dt_tracks), len(gt_tracks))
    tracks = list(dt_tracks) + list(gt_tracks)
    if not tracks:
        return c
    frames = len(tracks[0])
    assert all(len(t) == frames for t in tracks), "every track needs one entry per frame"
    hw = next((np.asarray(m).shape for t in tracks for m in t if m is not None), (0, 0))
    for f in range(frames):
        d, di = _frame_masks(dt_tracks, f, hw)
        g, gi = _frame_masks(gt_tracks, f, hw)
        c.add_frame(d, di, g, gi)
    return c


def sequence_iou(dt_tracks, gt_tracks) -> np.ndarray:
    """float64 [n_dt, n_gt]: ytvoseval.py iou_seq of every pair of tracks."""
    return sequence_counts(dt_tracks, gt_tracks).iou()


def avg_area(areas) -> float:
    """ytvos.py's avg_area: the mean of the entries of `areas` that are neither None nor 0, 0 without one."""
    l = [a for a in areas if a]
    return float(np.array(l).mean()) if l else 0.0


def area_outside(area: float, a: int) -> bool:
    return bool(area < VIDEO_AREA_RNG[a][0] or area > VIDEO_AREA_RNG[a][1])


def row_area(area: float) -> int:
    """What a row shows of an avg_area: truncated and clamped to int32."""
    return int(min(area, 2147483647.0))


def gt_track_rows(gt_tracks, to_contiguous: Dict[int, int]) -> np.ndarray:
    """The ground-truth tracks of a video (dicts with category_id, iscrowd and either avg_area or areas) -> int32 [n_gt, 3] = contiguous
    category | iscrowd | bits 0..3: avg_area outside range a, the table `image_rows` takes for a picture."""
    rows = np.zeros((len(gt_tracks), 3), np.int32)
    for i, t in enumerate(gt_tracks):
        area = float(t["avg_area"]) if "avg_area" in t else avg_area(t["areas"])
        rows[i] = (to_contiguous[int(t["category_id"])], int(t.get("iscrowd", 0)), sum(1 << a for a in range(4) if area_outside(area, a)))
    return rows


def pack_segmentations(segmentations, hw):
    """One frame's ground-truth masks (RLE dicts with compressed or uncompressed counts, or lists of polygons on a picture of hw =
    (h, w)) as the frame call takes them -> (runs uint32, offsets int64 [n + 1], xy float64, poly_offsets int64 [n_poly + 1] in
    vertices, gt_polys int32 [n + 1]): the mask part of `instance_eval.gt_rows(..., polygons=True)`, without its table.  A polygon
    mask has an empty run range.  A malformed polygon raises ValueError."""
    runs, offsets, xy, poly_offsets, gt_polys = [], [0], [], [0], [0]
    for seg in segmentations:
        cnts = np.zeros(0, np.int64)
        if isinstance(seg, dict):
            cnts = IE.annotation_counts(seg)
        else:
            for poly in seg:
                poly = coco_poly.check_polygon(poly)
                xy.append(poly)
                poly_offsets.append(poly_offsets[-1] + poly.size // 2)
        runs.append(np.asarray(cnts, np.uint32))
        offsets.append(offsets[-1] + len(cnts))
        gt_polys.append(len(poly_offsets) - 1)
    return ((np.concatenate(runs) if runs else np.zeros(0, np.uint32)), np.asarray(offsets, np.int64),
            (np.concatenate(xy) if xy else np.zeros(0, np.float64)), np.asarray(poly_offsets, np.int64), np.asarray(gt_polys, np.int32))


# ---- evaluateVid ----------------------------------------------------------------------------------------------------------------------------
def rows_from_counts(counts: Counts, scores, classes, gt_table, video: int = 0, iou_thrs=IE.IOU_THRS, num_categories=None):
    """evaluateVid on the sums of a video (odise_hip_video_eval_finish) -> (rows IE.ROW_DTYPE [n_tracks] in descending score, flags).
    Track s has scores[s] and classes[s]; gt_table: `gt_track_rows`.  A video that raises a flag (2, 4) has no rows."""
    scores, classes = np.asarray(scores, np.float32).reshape(-1), np.asarray(classes, np.int64).reshape(-1)
    table = np.asarray(gt_table, np.int64).reshape(-1, 3)
    n, n_gt = len(scores), len(table)
    assert n <= MAX_TRACKS and n <= counts.inter.shape[0] and len(classes) == n and n_gt <= counts.inter.shape[1], (n, n_gt, counts.inter.shape)
    flags = IE._table_flags(n, classes, table, num_categories)
    if flags:
        return np.zeros(0, IE.ROW_DTYPE), flags
    area = counts.avg_area(n)
    outside = [[area_outside(float(area[s]), a) for a in range(4)] for s in range(n)]
    shown = np.asarray([row_area(float(x)) for x in area], np.int64)
    return IE._walk(n, scores, classes, table, counts.iou(n, n_gt), shown, outside, video, iou_thrs), 0


def video_rows(dt_tracks, scores, classes, gt_tracks, gt_table, video: int = 0, iou_thrs=IE.IOU_THRS, num_categories=None):
    """evaluateVid of one video -> (rows IE.ROW_DTYPE [n] in descending score with `image` = video, flags): dt_tracks / gt_tracks as in
    `sequence_counts`, at most 100 predicted tracks."""
    return rows_from_counts(sequence_counts(dt_tracks, gt_tracks), scores, classes, gt_table, video, iou_thrs, num_categories)


# ---- the front door -------------------------------------------------------------------------------------------------------------------------
def _decode(seg, h: int, w: int) -> Optional[np.ndarray]:
    """uint8 [h, w] of one frame's segmentation: None, an RLE dict (compressed or uncompressed counts) or a list of polygons."""
    if not seg:
        return None
    cnts = IE.annotation_counts(seg) if isinstance(seg, dict) else coco_poly.annotation_to_counts(seg, h, w)
    return IE.decode_runs(cnts, h, w)


def _chunks(tracks, to_contiguous):
    """The predicted tracks of a video as the evaluator sees them: per category the 100 best by score (stable), then groups of whole
    categories of at most MAX_TRACKS tracks each - categories are matched apart, so a video may be walked in several parts."""
    by_cat: Dict[int, list] = {}
    for t in tracks:
        by_cat.setdefault(to_contiguous[int(t["category_id"])], []).append(t)
    out, cur = [], []
    for cat in sorted(by_cat):
        ts = by_cat[cat]
        order = np.argsort([-float(t["score"]) for t in ts], kind="mergesort")[:MAX_TRACKS]
        ts = [ts[i] for i in sorted(order.tolist())]
        if len(cur) + len(ts) > MAX_TRACKS:
            out.append(cur)
            cur = []
        cur = cur + ts
    return out + [cur] if cur or not out else out


def evaluate_files(results_path: str, gt_path: str, device: str = "cpu", ctx=None) -> dict:
    """-> {"stats": the 12 COCO numbers, "results": detectron2's dict, "flags"} of a YTVIS results file (instances_to_coco_json_video:
    video_id, score, category_id, segmentations = one compressed RLE or null per frame) against a YTVIS annotation file.  device "cpu":
    this module alone; "gpu": HipVideoInstanceEvaluator on U8 frames decoded here, on `ctx` (None: the process-wide context)."""
    with open(gt_path) as f:
        gt = json.load(f)
    with open(results_path) as f:
        res = json.load(f)
    cats = sorted(gt["categories"], key=lambda c: c["id"])
    to_contiguous = {int(c["id"]): k for k, c in enumerate(cats)}
    names = [str(c.get("name", c["id"])) for c in cats]
    K = len(cats)
    videos = sorted(gt["videos"], key=lambda v: v["id"])
    gt_by, dt_by = {}, {}
    for a in gt["annotations"]:
        gt_by.setdefault(a["video_id"], []).append(a)
    for r in res:
        dt_by.setdefault(r["video_id"], []).append(r)
    ev = None
    if device != "cpu":
        from .runtime import default_context
        from .video_seg_eval import HipVideoInstanceEvaluator
        ev = HipVideoInstanceEvaluator(ctx if ctx is not None else default_context(), to_contiguous, names)
    all_rows, npig, flags = [], np.zeros((K, 4), np.int64), 0
    for vi, v in enumerate(videos):
        h, w, T = int(v["height"]), int(v["width"]), int(v.get("length", len(v.get("file_names", []))))
        gts = gt_by.get(v["id"], [])
        for t in gts:
            if "areas" not in t and "avg_area" not in t:
                t["areas"] = [None if not s else int(np.count_nonzero(_decode(s, h, w))) for s in t["segmentations"]]
            assert len(t["segmentations"]) == T, (v["id"], len(t["segmentations"]), T)
        table = gt_track_rows(gts, to_contiguous)
        npig += IE.npig(table, K)
        g_tracks = None if ev else [[_decode(s, h, w) for s in t["segmentations"]] for t in gts]
        for ci, chunk in enumerate(_chunks(dt_by.get(v["id"], []), to_contiguous)):
            scores = [float(t["score"]) for t in chunk]
            classes = [to_contiguous[int(t["category_id"])] for t in chunk]
            assert all(len(t["segmentations"]) == T for t in chunk), f"video {v['id']}: a result without one entry per frame"
            if ev:
                ev.begin_video(vi, gts, count_gt=ci == 0)
                for f in range(T):
                    masks = np.zeros((max(len(chunk), 1), h, w), np.uint8)
                    for i, t in enumerate(chunk):
                        m = _decode(t["segmentations"][f], h, w)
                        if m is not None:
                            masks[i] = m
                    ev.process_frame(f, (h, w), np.arange(len(masks), dtype=np.int32) if chunk else np.full(1, -1, np.int32),
                                     masks=ev.ctx.to_device(masks))
                ev.end_video(scores, classes)
            else:
                d_tracks = [[_decode(s, h, w) for s in t["segmentations"]] for t in chunk]
                rows, fl = video_rows(d_tracks, scores, classes, g_tracks, table, vi, num_categories=K)
                flags |= fl
                all_rows.append(rows)
    if ev:
        out = ev.evaluate()["segm"]
        precision, recall = ev.precision, ev.recall
    else:
        if flags:
            raise RuntimeError("video instance evaluation: malformed input(s): " + "; ".join(flag_names(flags)))
        rows = np.concatenate(all_rows) if all_rows else np.zeros(0, IE.ROW_DTYPE)
        precision, recall = IE.accumulate(rows, npig, K)
        out = IE.results(precision, recall, names)
    return {"stats": IE.summarize(precision, recall), "results": out, "flags": flags}


_STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m odise_amd.video_eval", description="YouTube-VIS AP of a results file against an annotation file")
    ap.add_argument("--results", required=True, help="YTVIS results json: video_id, score, category_id, segmentations (compressed RLE or null per frame)")
    ap.add_argument("--gt", required=True, help="YTVIS annotation json")
    ap.add_argument("--device", default="gpu", choices=("gpu", "cpu"), help="cpu: the numpy specification alone")
    args = ap.parse_args(argv)
    out = evaluate_files(args.results, args.gt, args.device)
    for name, v in zip(_STAT_NAMES, out["stats"]):
        print(f"{name} {float(v):.6f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
