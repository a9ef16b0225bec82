"""A thing keeps its colour from frame to frame: `VisualizationDemo.run_on_video` (demo/demo.py:201-243) -> detectron2
`VideoVisualizer.draw_panoptic_seg_predictions` / `draw_instance_predictions` -> `_assign_colors`, the mask-IoU path.

This module holds the numpy restatement of the rule - the reference the device trackers (csrc/track.hip: odise_hip_track_frame;
csrc/inst_track.hip: odise_hip_inst_track_frame) are held to byte for byte (tests/test_gpu_track.py, tests/test_gpu_inst_track.py), itself
pinned to a literal sequential formulation (tests/test_track_cpu.py, tests/test_inst_track_cpu.py) - and the host twins of
`HipVideoVisualizer.draw_panoptic_seg_predictions` and `HipVideoVisualizer.draw_instance_predictions`.

The rule (include/odise_hip.h states it in full): the instances of a frame are the thing rows that are the first row of their id, have an
id > 0 and own a pixel, in table-row order (`ColorTracker`), or the entries of an instance selection whose score reaches `min_score` and
whose mask has a pixel, in table order (`InstanceColorTracker`: these masks may overlap).  Every live instance takes the first maximum
of its IoU row against them (0 where the categories differ); if that IoU is above 0.5 and no earlier live instance chose the same new one,
the new instance inherits its colour and the old one leaves the list, otherwise the old one loses one ttl and stays while ttl > 0.  New
instances without a colour take the next one of a fixed pool (detectron2 draws a random one).  The live list is the frame's instances,
then the surviving old ones, in order.

Mask-IoU matching of instances is detectron2's path for a `_DetectedInstance` without a box.  It is not what the reference's
run_on_video shows on this model: its instances carry pred_boxes of zeros, box IoU is 0 / 0, and every instance gets a fresh colour in
every frame.

`BoxColorTracker` is the FIRST path of `_assign_colors`, for instances that carry boxes (csrc/box_track.hip: odise_hip_box_track_frame;
tests/test_box_track_cpu.py, tests/test_gpu_box_track.py): the same walk with an instance being an entry whose score passes and whose box
is finite with a positive width and height, the IoU that of the two boxes (instance_eval.box_iou on their XYWH form) and the threshold
0.6.  `_LiveList._step` takes the IoU source and the threshold as parameters; the two mask trackers pass the defaults.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .visualize import (BOX_ALPHA256, LARGE_AREA, SMALL_AREA, _fallback_color, _row_of_id, _table, default_box_width, draw_labels, draw_texts,
                        instance_anchors, instance_anchors_boxes, instance_colors, instance_edge_colors, instance_order, instance_order_boxes,
                        instance_overlay, instance_overlay_boxes, instance_texts, panoptic_overlay, segment_anchors, segment_colors)

TRACK_ROW_DTYPE = np.dtype([("frame", np.int32), ("id", np.int32), ("category", np.int32), ("area", np.int32), ("ttl", np.int32),
                            ("rgb", np.int32), ("pad0", np.int32), ("pad1", np.int32)])   # odise_track_row, 32 bytes
assert TRACK_ROW_DTYPE.itemsize == 32
MAX_TTL = 8                 # retained frames of the device tracker
POOL_COLORS = 74            # detectron2 VideoVisualizer max_num_instances
MAX_INSTANCES = 100         # topk limit of the device instance tracker


def default_pool(n: int = POOL_COLORS) -> np.ndarray:
    return np.array([_fallback_color(k) for k in range(n)], np.uint8).reshape(n, 3)


def frame_instances(pred_ids, segments) -> list:
    """[(table row, id, category, bool mask)] of a frame, in table-row order."""
    pred_ids = np.asarray(pred_ids)
    segments = _table(segments)
    rows = _row_of_id(segments)
    out = []
    for r, (i, isthing, cat) in enumerate(segments):
        if not isthing or rows.get(int(i)) != r:
            continue
        mask = pred_ids == i
        if mask.any():
            out.append((r, int(i), int(cat), mask))
    return out


def selection_instances(classes, scores, masks, min_score: float = 0.0) -> list:
    """[(table index, table index, class, bool mask)] of an instance selection: the entries with score >= min_score (scores None: all)
    whose mask has a pixel - the `kept` rule of odise_hip_instance_draw - in table order."""
    masks = np.asarray(masks) != 0
    out = []
    for i, mask in enumerate(masks):
        if scores is not None and not np.float32(scores[i]) >= np.float32(min_score):
            continue
        if mask.any():
            out.append((i, i, int(classes[i]), mask))
    return out


def pack_rgb(c) -> int:
    return int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16)


def match_winners(iou, threshold: float = 0.5) -> tuple:
    """iou float64 [live, new] -> (choice, winner), the order-free form of the matching that the device runs: choice[o] = the first
    maximum of row o when it is above `threshold` (0.5 for masks, 0.6 for boxes), else -1; winner[j] = the smallest o with choice[o] == j.  Live row o is matched iff
    winner[choice[o]] == o - exactly the rows the sequential walk matches, since a row is refused there only when an earlier row took
    its choice."""
    iou = np.asarray(iou, np.float64)
    choice = [int(np.argmax(row)) if row.size and row.max() > threshold else -1 for row in iou]
    winner = {}
    for o, j in enumerate(choice):
        if j >= 0 and j not in winner:
            winner[j] = o
    return choice, winner


def _mask_iou(o: dict, mask, area: int) -> np.float64:
    inter = int((o["mask"] & mask).sum())
    return np.float64(inter) / np.float64(o["area"] + area - inter)


class _LiveList:
    """What both trackers are: the ttl, the pool and its counter, the live list and one step of the rule on a frame's instances."""

    def __init__(self, ttl: int = MAX_TTL, pool=None):
        if not 1 <= int(ttl) <= MAX_TTL:
            raise ValueError(f"ttl {ttl} outside 1..{MAX_TTL}")
        self.ttl = int(ttl)
        self.pool = default_pool() if pool is None else np.ascontiguousarray(np.asarray(pool, np.uint8).reshape(-1, 3))
        if len(self.pool) < 1:
            raise ValueError("an empty colour pool")
        self.reset()

    def reset(self) -> None:
        self.live, self.counter, self.frame, self.hw = [], 0, 0, None
        self.last_iou = np.zeros((0, 0), np.float64)

    def live_rows(self) -> np.ndarray:
        out = np.zeros(len(self.live), TRACK_ROW_DTYPE)
        for k, o in enumerate(self.live):
            out[k] = (o["frame"], o["id"], o["category"], o["area"], o["ttl"], o["rgb"], 0, 0)
        return out

    def _check_size(self, hw) -> None:
        if self.hw is None:
            self.hw = tuple(hw)
        if tuple(hw) != self.hw:
            raise ValueError(f"a {tuple(hw)} frame for a tracker of {self.hw}")

    def _step(self, new: list, out: np.ndarray, iou_of=None, area_of=None, threshold: float = 0.5) -> np.ndarray:
        """new: the frame's instances [(row of `out`, id, category, shape)]; their rows of `out` are recoloured.  A shape is a bool mask
        (the default: area = its pixels, IoU = the division of the two integer counts) or whatever `area_of(shape)` and
        `iou_of(live row, shape, area of shape)` read; a match needs an IoU above `threshold`."""
        area_of = area_of or (lambda m: int(m.sum()))
        iou_of = iou_of or _mask_iou
        area = [area_of(m) for _, _, _, m in new]
        iou = np.zeros((len(self.live), len(new)), np.float64)
        for a, o in enumerate(self.live):
            for b, (_, _, cat, mask) in enumerate(new):
                if cat == o["category"]:
                    iou[a, b] = iou_of(o, mask, area[b])
        self.last_iou = iou
        choice, winner = match_winners(iou, threshold)
        rgb = [None] * len(new)
        for b, a in winner.items():
            rgb[b] = self.live[a]["rgb"]
        survivors = []
        for a, o in enumerate(self.live):
            if choice[a] >= 0 and winner[choice[a]] == a:
                continue
            o["ttl"] -= 1
            if o["ttl"] > 0:
                survivors.append(o)
        for b in range(len(new)):
            if rgb[b] is None:
                rgb[b] = pack_rgb(self.pool[self.counter % len(self.pool)])
                self.counter += 1
        fresh = []
        for b, (r, i, cat, mask) in enumerate(new):
            out[r] = (rgb[b] & 255, (rgb[b] >> 8) & 255, (rgb[b] >> 16) & 255)
            fresh.append({"frame": self.frame, "id": i, "category": cat, "area": area[b], "ttl": self.ttl, "rgb": rgb[b], "mask": mask.copy()})
        self.live = fresh + survivors
        self.frame += 1
        return out


class ColorTracker(_LiveList):
    """`assign(pred_ids, segments, colors) -> colors` per frame.  `live` is the list after the last frame (dicts with frame, id, category,
    area, ttl, rgb, mask), `last_iou` the float64 [live before the frame, instances of the frame] matrix of the last frame."""

    def assign(self, pred_ids, segments, colors: Optional[np.ndarray] = None) -> np.ndarray:
        """pred_ids int [H,W], segments rows (id, isthing, category), colors uint8 [n,3] (what the rows have so far; zeros when not
        given) -> uint8 [n,3]: the rows of the frame's instances recoloured, every other row as it came."""
        pred_ids = np.asarray(pred_ids)
        segments = _table(segments)
        self._check_size(pred_ids.shape)
        out = np.zeros((len(segments), 3), np.uint8) if colors is None else np.array(colors, np.uint8).reshape(len(segments), 3)
        return self._step(frame_instances(pred_ids, segments), out)


class InstanceColorTracker(_LiveList):
    """`assign(classes, scores, masks, min_score, colors) -> colors` per frame, for instance masks that may overlap (the restatement of
    odise_hip_inst_track_frame).  `live` / `last_iou` / `live_rows()` as ColorTracker's; a live row's id is its table index."""

    def assign(self, classes, scores, masks, min_score: float = 0.0, colors: Optional[np.ndarray] = None) -> np.ndarray:
        """classes int [n], scores float [n] (None: no score test), masks bool [n,h,w], colors uint8 [m >= n,3] by table index (zeros [n,3]
        when not given) -> the same with the rows of the frame's instances recoloured, every other row as it came."""
        masks = np.asarray(masks) != 0
        if masks.ndim != 3 or len(classes) != len(masks) or len(masks) > MAX_INSTANCES:
            raise ValueError(f"masks {masks.shape} for {len(classes)} classes (at most {MAX_INSTANCES} instances [n,h,w])")
        self._check_size(masks.shape[1:])
        out = np.zeros((len(masks), 3), np.uint8) if colors is None else np.array(colors, np.uint8).reshape(-1, 3)
        if len(out) < len(masks):
            raise ValueError(f"{len(out)} colours for {len(masks)} instances")
        return self._step(selection_instances(classes, scores, masks, min_score), out)


BOX_IOU_THRESHOLD = 0.6     # detectron2 _assign_colors: 0.6 for instances with boxes, 0.5 for masks


def box_instances(classes, scores, boxes, min_score: float = 0.0) -> list:
    """[(table index, table index, class, float32 [4] XYXY)] of an instance selection with boxes: the entries with score >= min_score
    (scores None: all) whose box is finite and has x1 > x0 and y1 > y0, in table order."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    out = []
    for i, b in enumerate(boxes):
        if scores is not None and not np.float32(scores[i]) >= np.float32(min_score):
            continue
        if np.isfinite(b).all() and b[2] > b[0] and b[3] > b[1]:
            out.append((i, i, int(classes[i]), b.copy()))
    return out


def _xywh(b) -> np.ndarray:
    """XYXY float32 -> XYWH float64, the differences taken in double"""
    b = np.asarray(b, np.float32).astype(np.float64)
    return np.array([b[0], b[1], b[2] - b[0], b[3] - b[1]], np.float64)


def _box_area(b) -> int:
    """(int32) of the box's w * h (the double product), at most 2^31 - 1"""
    x = _xywh(b)
    return int(min(x[2] * x[3], 2147483647.0))


def _box_iou(o: dict, box, area: int) -> np.float64:
    from .instance_eval import box_iou
    return box_iou(_xywh(o["mask"])[None], _xywh(box)[None])[0, 0]


class BoxColorTracker(_LiveList):
    """`assign(classes, scores, boxes, min_score, colors) -> colors` per frame, for instances that carry boxes: the first path of
    _assign_colors, box IoU above 0.6 (the restatement of odise_hip_box_track_frame).  The IoU is instance_eval.box_iou (maskApi.c bbIou)
    of the two boxes as XYWH - the geometric IoU; detectron2 itself, as far as it can be read, hands XYXY rows to that function.
    `live` / `last_iou` / `live_rows()` as ColorTracker's; a live row's id is its table index, its area (int32) of its box's w * h, and
    its box is under the key "mask"."""

    def assign(self, classes, scores, boxes, min_score: float = 0.0, colors: Optional[np.ndarray] = None) -> np.ndarray:
        """classes int [n], scores float [n] (None: no score test), boxes float32 [n,4] XYXY, colors uint8 [m >= n,3] by table index
        (zeros [n,3] when not given) -> the same with the rows of the frame's instances recoloured, every other row as it came."""
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        if len(classes) != len(boxes) or len(boxes) > MAX_INSTANCES:
            raise ValueError(f"{len(boxes)} boxes for {len(classes)} classes (at most {MAX_INSTANCES} instances)")
        out = np.zeros((len(boxes), 3), np.uint8) if colors is None else np.array(colors, np.uint8).reshape(-1, 3)
        if len(out) < len(boxes):
            raise ValueError(f"{len(out)} colours for {len(boxes)} instances")
        return self._step(box_instances(classes, scores, boxes, min_score), out, _box_iou, _box_area, BOX_IOU_THRESHOLD)


def draw_panoptic_seg_predictions(image, pred_ids, segments, tracker: ColorTracker, metadata=None, alpha256: int = 128, edge_rgb=(0, 0, 0),
                                  small_area: int = SMALL_AREA, large_area: int = LARGE_AREA, labels: bool = True) -> np.ndarray:
    """`draw_panoptic_seg` with the tracker's colours for things: what HipVideoVisualizer.draw_panoptic_seg_predictions returns, computed
    by the restatement (labels=False: the picture before the names are drawn)."""
    segments = _table(segments)
    colors = tracker.assign(pred_ids, segments, segment_colors(segments, metadata))
    pic = panoptic_overlay(image, pred_ids, segments, colors, alpha256, edge_rgb)
    if not labels:
        return pic
    return draw_labels(pic, segment_anchors(pred_ids, segments, small_area, large_area), segments, metadata)


def draw_instance_predictions(image, masks, classes, scores, tracker, metadata=None, alpha256: int = 128, min_score: float = 0.0,
                              labels: bool = True, boxes=None, box_width: Optional[int] = None, box_alpha256: int = BOX_ALPHA256) -> np.ndarray:
    """visualize.draw_instance_predictions with the tracker's colours (and the outlines derived from them): what
    HipVideoVisualizer.draw_instance_predictions returns, computed by the restatement (labels=False: before the texts are drawn).
    tracker: an InstanceColorTracker, or with boxes float32 [n,4] XYXY (boxes=True of the device call) a BoxColorTracker."""
    if boxes is not None:
        h, w = np.asarray(image).shape[:2]
        bw = default_box_width(h, w) if box_width is None else int(box_width)
        colors = tracker.assign(classes, scores, boxes, min_score, instance_colors(classes, metadata))
        pic = instance_overlay_boxes(image, masks, boxes, colors, instance_edge_colors(colors), alpha256, scores, min_score, bw, box_alpha256)
        if not labels:
            return pic
        anchors, order = instance_anchors_boxes(masks, boxes, scores, min_score), instance_order_boxes(masks, boxes, scores, min_score)
        kept = sorted((i for i in range(len(anchors)) if order[i] >= 0), key=lambda i: order[i])
        return draw_texts(pic, anchors[kept], instance_texts(classes, scores, metadata))
    colors = tracker.assign(classes, scores, masks, min_score, instance_colors(classes, metadata))
    pic = instance_overlay(image, masks, colors, instance_edge_colors(colors), alpha256, scores, min_score)
    if not labels:
        return pic
    anchors = instance_anchors(masks, scores, min_score)
    order = instance_order(masks, scores, min_score)
    kept = sorted((i for i in range(len(anchors)) if order[i] >= 0), key=lambda i: order[i])
    return draw_texts(pic, anchors[kept], instance_texts(classes, scores, metadata))
