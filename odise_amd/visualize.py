"""Drawing a panoptic result: `VisualizationDemo.run_on_image` (demo/demo.py:173-199) -> detectron2 `Visualizer.draw_panoptic_seg`.

The per-pixel work - the pieces of a segment, where its label goes, the colour blend and the outlines - runs on the device
(csrc/vis.hip: odise_hip_connected_components / odise_hip_segment_anchors / odise_hip_panoptic_overlay) on the panoptic record as it lies
in HBM; glyphs are drawn on the host with Pillow.  This module holds

* the numpy restatement of the three rules, written literally: the reference the device is held to (tests/test_gpu_visualize.py), itself
  pinned to scipy.ndimage.label, np.median and a per-pixel loop (tests/test_visualize_cpu.py);
* `segment_colors`: which colour a table row gets;
* `HipVisualizer.draw_panoptic_seg`.

The rules are detectron2's (a stuff label at the median pixel of the segment's largest 8-connected component and of every other
component above `large_area`, nothing for a segment whose largest component is below `small_area`; a thing label at the median pixel of
its mask).  NO pixel parity with detectron2's matplotlib rendering is claimed: the rules are its rules, the rasterisation - integer
blend, one-pixel outlines along 4-neighbour id changes, Pillow's default font - is this project's.
"""
from __future__ import annotations

import colorsys
from typing import Optional, Sequence

import numpy as np

SMALL_AREA = 1000       # detectron2 _SMALL_OBJECT_AREA_THRESH
LARGE_AREA = 120000     # detectron2 _LARGE_MASK_AREA_THRESH

ANCHOR_DTYPE = np.dtype([("segment_row", np.int32), ("area", np.int32), ("x2", np.int32), ("y2", np.int32),
                         ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32)])   # odise_anchor_row, 32 bytes
assert ANCHOR_DTYPE.itemsize == 32


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def connected_roots(labels) -> np.ndarray:
    """labels int [H,W] -> int32 [H,W]: the smallest row-major index among the pixels joined to p by 8-neighbour steps over equal
    labels; -1 where labels <= 0.  A flood fill from every pixel that has no root yet, in row-major order (so the seed is the minimum)."""
    labels = np.asarray(labels)
    H, W = labels.shape
    roots = np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in range(W):
            l = labels[y, x]
            if l <= 0 or roots[y, x] >= 0:
                continue
            seed = y * W + x
            roots[y, x] = seed
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                        if roots[ny, nx] < 0 and labels[ny, nx] == l:
                            roots[ny, nx] = seed
                            stack.append((ny, nx))
    return roots


def _table(segments) -> np.ndarray:
    return np.asarray(segments, np.int64).reshape(-1, 3)


def _row_of_id(segments: np.ndarray) -> dict:
    rows = {}
    for r, (i, _, _) in enumerate(segments):
        if i > 0 and int(i) not in rows:          # the first row of an id counts
            rows[int(i)] = r
    return rows


def _anchor(row: int, mask: np.ndarray) -> tuple:
    ys, xs = np.nonzero(mask)
    my, mx = np.median(np.stack([ys, xs]), axis=1)
    return (row, len(ys), int(round(2 * mx)), int(round(2 * my)), int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def segment_anchors(pred_ids, segments, small_area: int = SMALL_AREA, large_area: int = LARGE_AREA) -> np.ndarray:
    """pred_ids int [H,W], segments rows (id, isthing, category) -> ANCHOR_DTYPE records in ascending (segment_row, root) order."""
    pred_ids = np.asarray(pred_ids)
    segments = _table(segments)
    rows = _row_of_id(segments)
    roots = None
    out = []
    for r, (i, isthing, _) in enumerate(segments):
        if rows.get(int(i)) != r:
            continue
        mask = pred_ids == i
        if not mask.any():
            continue
        if isthing:
            out.append(_anchor(r, mask))
            continue
        if roots is None:
            roots = connected_roots(pred_ids)
        comp, areas = np.unique(roots[mask], return_counts=True)          # ascending root = the order the components are met in
        largest = int(np.argmax(areas))                                   # the first of equal areas
        if areas[largest] < small_area:
            continue
        for k, c in enumerate(comp):
            if k == largest or areas[k] > large_area:
                out.append(_anchor(r, roots == c))
    return np.array(out, ANCHOR_DTYPE) if out else np.zeros((0,), ANCHOR_DTYPE)


def panoptic_overlay(image, pred_ids, segments, colors, alpha256: int = 128, edge_rgb=(0, 0, 0)) -> np.ndarray:
    """image uint8 [H,W,3] -> uint8 [H,W,3]: pixels of a table row blended with the row's colour, outlined where a 4-neighbour inside
    the picture has another id; everything else untouched."""
    image = np.asarray(image, np.uint8)
    ids = np.asarray(pred_ids).astype(np.int64)
    segments = _table(segments)
    colors = np.asarray(colors, np.int64).reshape(-1, 3)
    assert 0 <= alpha256 <= 256
    row = np.full(ids.shape, -1, np.int64)
    for i, r in _row_of_id(segments).items():
        row[ids == i] = r
    known = row >= 0
    edge = np.zeros(ids.shape, bool)
    edge[:, 1:] |= ids[:, 1:] != ids[:, :-1]
    edge[:, :-1] |= ids[:, :-1] != ids[:, 1:]
    edge[1:, :] |= ids[1:, :] != ids[:-1, :]
    edge[:-1, :] |= ids[:-1, :] != ids[1:, :]
    blend = (image.astype(np.int64) * (256 - alpha256) + colors[np.where(known, row, 0)] * alpha256 + 128) >> 8 if len(colors) else image
    out = np.where(known[..., None], blend, image)
    out = np.where((known & edge)[..., None], np.asarray(edge_rgb, np.int64), out)
    return out.astype(np.uint8)


# ---- the restatement: instances and semantic results (csrc/vis_inst.hip) ----------------------------------------------------------------
def _kept(masks, scores, min_score) -> np.ndarray:
    """bool [n]: score >= min_score (float32, as the device compares) and a pixel in the mask; no scores: every non-empty mask."""
    masks = np.asarray(masks) != 0
    kept = masks.reshape(len(masks), -1).any(axis=1) if len(masks) else np.zeros(0, bool)
    if scores is not None:
        kept &= np.asarray(scores, np.float32)[:len(masks)] >= np.float32(min_score)
    return kept


def instance_anchors(masks, scores=None, min_score: float = 0.0, topk: Optional[int] = None) -> np.ndarray:
    """masks [n,H,W] (nonzero = 1) -> ANCHOR_DTYPE [topk], one row per table index: (i, area, twice the median column / row, bounding
    box) of a kept instance, (-1, 0, ..) otherwise and past n."""
    masks = np.asarray(masks) != 0
    topk = len(masks) if topk is None else int(topk)
    out = np.zeros(topk, ANCHOR_DTYPE)
    out["segment_row"] = -1
    for i, k in enumerate(_kept(masks, scores, min_score)):
        if k:
            out[i] = _anchor(i, masks[i])
    return out


def instance_order(masks, scores=None, min_score: float = 0.0, topk: Optional[int] = None) -> np.ndarray:
    """int32 [topk]: the position of instance i in the draw order (descending area, ties by ascending index), -1 when it is not kept."""
    masks = np.asarray(masks) != 0
    topk = len(masks) if topk is None else int(topk)
    kept = _kept(masks, scores, min_score)
    area = masks.reshape(len(masks), -1).sum(axis=1) if len(masks) else np.zeros(0, np.int64)
    out = np.full(topk, -1, np.int32)
    for rank, i in enumerate(sorted((i for i in range(len(masks)) if kept[i]), key=lambda i: (-int(area[i]), i))):
        out[i] = rank
    return out


def instance_overlay(image, masks, colors, edge_colors, alpha256: int = 128, scores=None, min_score: float = 0.0) -> np.ndarray:
    """image uint8 [H,W,3] -> uint8 [H,W,3]: the kept instances in draw order, one over the other; a pixel of a mask with a 4-neighbour
    inside the picture that is outside the mask takes the instance's edge colour, any other pixel of the mask is blended with its colour."""
    out = np.asarray(image, np.uint8).astype(np.int64)
    masks = np.asarray(masks) != 0
    colors, edge_colors = np.asarray(colors, np.int64).reshape(-1, 3), np.asarray(edge_colors, np.int64).reshape(-1, 3)
    assert 0 <= alpha256 <= 256
    order = instance_order(masks, scores, min_score)
    for i in sorted((i for i in range(len(masks)) if order[i] >= 0), key=lambda i: order[i]):
        m = masks[i]
        edge = np.zeros(m.shape, bool)
        edge[:, 1:] |= ~m[:, :-1]
        edge[:, :-1] |= ~m[:, 1:]
        edge[1:, :] |= ~m[:-1, :]
        edge[:-1, :] |= ~m[1:, :]
        blend = (out * (256 - alpha256) + colors[i] * alpha256 + 128) >> 8
        out = np.where((m & ~edge)[..., None], blend, out)
        out = np.where((m & edge)[..., None], edge_colors[i], out)
    return out.astype(np.uint8)


# ---- the restatement: instances that carry boxes (odise_hip_instance_draw_boxes: overlay_instances(boxes=, masks=)) ----------------------
BOX_ALPHA256 = 128


def default_box_width(h: int, w: int) -> int:
    """A quarter of detectron2's default font size max(sqrt(h * w) // 90, 10) - its box line width is font_size / 3, drawn by
    matplotlib in points - rounded, at least one pixel."""
    return max(1, round(max(float(np.sqrt(h * w)) // 90, 10) / 4))


def _boxes32(boxes, n: int) -> np.ndarray:
    return np.asarray(boxes, np.float32).reshape(-1, 4)[:n]


def _box_trunc(v) -> int:
    """A float member toward zero, within +-2^29 (what the device keeps of it)"""
    return int(np.trunc(np.clip(np.float32(v), -536870912.0, 536870912.0)))


def _box_area32(b) -> np.float32:
    return np.float32(np.float32(b[2] - b[0]) * np.float32(b[3] - b[1]))      # the float product of the float differences


def _kept_boxes(masks, boxes, scores, min_score) -> np.ndarray:
    """`_kept`, and the box is finite with a positive width and height"""
    kept = _kept(masks, scores, min_score)
    for i, b in enumerate(_boxes32(boxes, len(kept))):
        kept[i] &= bool(np.isfinite(b).all() and b[2] > b[0] and b[3] > b[1])
    return kept


def instance_order_boxes(masks, boxes, scores=None, min_score: float = 0.0, topk: Optional[int] = None) -> np.ndarray:
    """int32 [topk]: the position of instance i in the draw order with boxes (descending BOX area as the float product, ties by
    ascending index), -1 when it is not kept."""
    masks = np.asarray(masks) != 0
    topk = len(masks) if topk is None else int(topk)
    kept, b = _kept_boxes(masks, boxes, scores, min_score), _boxes32(boxes, len(masks))
    out = np.full(topk, -1, np.int32)
    for rank, i in enumerate(sorted((i for i in range(len(masks)) if kept[i]), key=lambda i: (-float(_box_area32(b[i])), i))):
        out[i] = rank
    return out


def instance_anchors_boxes(masks, boxes, scores=None, min_score: float = 0.0, topk: Optional[int] = None, small_area: int = SMALL_AREA) -> np.ndarray:
    """ANCHOR_DTYPE [topk], one row per table index: (i, mask pixels, twice the label position, the box truncated to integers) of a kept
    instance, (-1, 0, ..) otherwise and past n.  The label goes to the box corner (x0, y0); for a box below small_area or lower than 40
    rows to (x1, y0) when the box reaches the last five rows of the picture, else to (x0, y1)."""
    masks = np.asarray(masks) != 0
    topk = len(masks) if topk is None else int(topk)
    h = masks.shape[1] if masks.ndim == 3 else 0
    kept, bb = _kept_boxes(masks, boxes, scores, min_score), _boxes32(boxes, len(masks))
    out = np.zeros(topk, ANCHOR_DTYPE)
    out["segment_row"] = -1
    for i in range(len(masks)):
        if not kept[i]:
            continue
        b = bb[i]
        x0, y0, x1, y1 = (_box_trunc(v) for v in b)
        tx, ty = x0, y0
        if _box_area32(b) < np.float32(small_area) or np.float32(b[3] - b[1]) < np.float32(40):
            if b[3] >= np.float32(h - 5):
                tx = x1
            else:
                ty = y1
        out[i] = (i, int(masks[i].sum()), 2 * tx, 2 * ty, x0, y0, x1, y1)
    return out


def instance_overlay_boxes(image, masks, boxes, colors, edge_colors, alpha256: int = 128, scores=None, min_score: float = 0.0, box_width: int = 1,
                           box_alpha256: int = BOX_ALPHA256) -> np.ndarray:
    """`instance_overlay` with boxes: the kept instances in box order; each first blends its frame - the pixels of its box (truncated,
    clipped to the picture) within box_width of one of the four sides - with its colour at box_alpha256, then lays its mask."""
    out = np.asarray(image, np.uint8).astype(np.int64)
    H, W = out.shape[:2]
    masks = np.asarray(masks) != 0
    colors, edge_colors = np.asarray(colors, np.int64).reshape(-1, 3), np.asarray(edge_colors, np.int64).reshape(-1, 3)
    assert 0 <= alpha256 <= 256 and 0 <= box_alpha256 <= 256 and box_width >= 1
    order, bb = instance_order_boxes(masks, boxes, scores, min_score), _boxes32(boxes, len(masks))
    ys, xs = np.mgrid[0:H, 0:W]
    for i in sorted((i for i in range(len(masks)) if order[i] >= 0), key=lambda i: order[i]):
        x0, y0, x1, y1 = (_box_trunc(v) for v in bb[i])
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        inside = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        side = (xs < x0 + box_width) | (xs >= x1 - box_width) | (ys < y0 + box_width) | (ys >= y1 - box_width)
        out = np.where((inside & side)[..., None], (out * (256 - box_alpha256) + colors[i] * box_alpha256 + 128) >> 8, out)
        m = masks[i]
        edge = np.zeros(m.shape, bool)
        edge[:, 1:] |= ~m[:, :-1]
        edge[:, :-1] |= ~m[:, 1:]
        edge[1:, :] |= ~m[:-1, :]
        edge[:-1, :] |= ~m[1:, :]
        blend = (out * (256 - alpha256) + colors[i] * alpha256 + 128) >> 8
        out = np.where((m & ~edge)[..., None], blend, out)
        out = np.where((m & edge)[..., None], edge_colors[i], out)
    return out.astype(np.uint8)


def semantic_record(labels, K: int, max_segments: Optional[int] = None) -> np.ndarray:
    """labels int [H,W] -> int32 [H*W + 1 + 3*MAX_SEGMENTS]: ids | n | rows (id, 0, category), id = category + 1, rows by descending
    pixel count (ties: the smaller category), at most MAX_SEGMENTS of them; a label outside [0, K) or without a row has id 0."""
    from ._lib import MAX_SEGMENTS
    cap = MAX_SEGMENTS if max_segments is None else int(max_segments)
    labels = np.asarray(labels).astype(np.int64)
    counts = np.bincount(labels[(labels >= 0) & (labels < K)].reshape(-1), minlength=K)
    rows = sorted((c for c in range(K) if counts[c] > 0), key=lambda c: (-int(counts[c]), c))[:cap]
    ids = np.zeros(labels.shape, np.int32)
    table = np.zeros(1 + 3 * cap, np.int32)
    table[0] = len(rows)
    for r, c in enumerate(rows):
        ids[labels == c] = c + 1
        table[1 + 3 * r:4 + 3 * r] = (c + 1, 0, c)
    return np.concatenate([ids.reshape(-1), table])


def sem_labels(labels_or_sem_seg) -> np.ndarray:
    """int labels [H,W] as they are; scores [K,H,W] -> their arg-max (the first maximum, as np.argmax and the device take it)."""
    a = np.asarray(labels_or_sem_seg)
    return a.argmax(axis=0).astype(np.int32) if a.ndim == 3 else a


# ---- colours --------------------------------------------------------------------------------------------------------------------------
def _meta(metadata, key, default=None):
    if metadata is None:
        return default
    v = metadata.get(key) if isinstance(metadata, dict) else getattr(metadata, key, None)
    return default if v is None else v


def _fallback_color(k: int) -> tuple:
    r, g, b = colorsys.hsv_to_rgb((k * 0.61803398875) % 1.0, 0.65, 0.95)
    return int(r * 255), int(g * 255), int(b * 255)


def _jitter(color, segment_id: int) -> tuple:
    """A per-segment-id offset of up to +-24 per channel (detectron2 jitters instance colours randomly; here it is a function of the id)."""
    x = (int(segment_id) * 2654435761) & 0xFFFFFFFF
    return tuple(int(min(255, max(0, int(c) + ((x >> (8 * k)) & 0xFF) % 49 - 24))) for k, c in enumerate(color))


def segment_colors(segments, metadata=None) -> np.ndarray:
    """uint8 [n,3], one colour per table row: the metadata's `stuff_colors[category]` for stuff, its `thing_colors[category]` with a
    deterministic per-segment-id jitter for things; a category the metadata has no colour for gets one from a fixed hue sequence."""
    segments = _table(segments)
    stuff, thing = _meta(metadata, "stuff_colors", []), _meta(metadata, "thing_colors", [])
    out = np.zeros((len(segments), 3), np.uint8)
    for r, (i, isthing, cat) in enumerate(segments):
        table = thing if isthing else stuff
        base = tuple(table[cat]) if 0 <= cat < len(table) else _fallback_color(int(cat))
        out[r] = _jitter(base, i) if isthing else base
    return out


def instance_colors(classes, metadata=None) -> np.ndarray:
    """uint8 [n,3], by table index: the metadata's `thing_colors[class]` (or the fixed hue sequence) with the `_jitter` of the index."""
    thing = _meta(metadata, "thing_colors", [])
    out = np.zeros((len(classes), 3), np.uint8)
    for i, cat in enumerate(classes):
        cat = int(cat)
        out[i] = _jitter(tuple(thing[cat]) if 0 <= cat < len(thing) else _fallback_color(cat), i)
    return out


def instance_edge_colors(colors) -> np.ndarray:
    """uint8 [n,3]: the outline of a mask colour - the colour at 3/10 of its brightness when it is light (channel sum >= 384), moved
    7/10 of the way to white when it is dark."""
    c = np.asarray(colors, np.int64).reshape(-1, 3)
    light = c.sum(axis=1, keepdims=True) >= 384
    return np.where(light, c * 3 // 10, 255 - (255 - c) * 3 // 10).astype(np.uint8)


def instance_texts(classes, scores, metadata=None) -> list:
    """detectron2 _create_text_labels: "<class> <score in percent>%"."""
    thing = _meta(metadata, "thing_classes", [])
    return [f"{thing[int(c)] if 0 <= int(c) < len(thing) else f'class {int(c)}'} {float(s) * 100:.0f}%" for c, s in zip(classes, scores)]


def segment_names(segments, metadata=None) -> list:
    segments = _table(segments)
    stuff, thing = _meta(metadata, "stuff_classes", []), _meta(metadata, "thing_classes", [])
    names = []
    for _, isthing, cat in segments:
        table = thing if isthing and 0 <= cat < len(thing) else stuff
        names.append(str(table[cat]) if 0 <= cat < len(table) else f"class {int(cat)}")
    return names


def draw_labels(picture: np.ndarray, anchors: np.ndarray, segments, metadata=None) -> np.ndarray:
    """Class names at the anchors, centred on them (detectron2 centres a thing's label on the mask median when no box is drawn, and a
    stuff label on its component's): white text on a dark plate, Pillow's default font."""
    return draw_texts(picture, anchors, segment_names(segments, metadata))


def draw_texts(picture: np.ndarray, anchors: np.ndarray, texts: Sequence[str]) -> np.ndarray:
    """texts[segment_row] centred on every anchor: white on a dark plate, Pillow's default font."""
    from PIL import Image, ImageDraw, ImageFont
    img = Image.fromarray(np.ascontiguousarray(picture, np.uint8))
    draw = ImageDraw.Draw(img)
    font = ImageFont.load_default()
    for a in anchors:
        text = texts[int(a["segment_row"])]
        cx, cy = a["x2"] / 2.0, a["y2"] / 2.0
        l, t, r, b = draw.textbbox((0, 0), text, font=font)
        x, y = cx - (r - l) / 2.0 - l, cy - (b - t) / 2.0 - t
        draw.rectangle([x + l - 2, y + t - 1, x + r + 2, y + b + 1], fill=(0, 0, 0))
        draw.text((x, y), text, fill=(255, 255, 255), font=font)
    return np.asarray(img)


def draw_panoptic_seg(image, pred_ids, segments, metadata=None, alpha256: int = 128, edge_rgb=(0, 0, 0), small_area: int = SMALL_AREA,
                      large_area: int = LARGE_AREA) -> np.ndarray:
    """The host path from end to end: what HipVisualizer.draw_panoptic_seg returns, computed by the restatement."""
    segments = _table(segments)
    pic = panoptic_overlay(image, pred_ids, segments, segment_colors(segments, metadata), alpha256, edge_rgb)
    return draw_labels(pic, segment_anchors(pred_ids, segments, small_area, large_area), segments, metadata)


def draw_sem_seg(image, labels_or_sem_seg, K: int, metadata=None, alpha256: int = 128, edge_rgb=(0, 0, 0), small_area: int = SMALL_AREA,
                 large_area: int = LARGE_AREA) -> np.ndarray:
    """The host twin of HipVisualizer.draw_sem_seg: the semantic record drawn as a panoptic result whose rows are all stuff."""
    from ._lib import MAX_SEGMENTS
    labels = sem_labels(labels_or_sem_seg)
    rec = semantic_record(labels, K)
    npix = labels.size
    n = int(rec[npix])
    return draw_panoptic_seg(image, rec[:npix].reshape(labels.shape), rec[npix + 1:npix + 1 + 3 * n].reshape(n, 3), metadata, alpha256, edge_rgb,
                             small_area, large_area)


def draw_instance_predictions(image, masks, classes, scores, metadata=None, alpha256: int = 128, min_score: float = 0.0, boxes=None,
                              box_width: Optional[int] = None, box_alpha256: int = BOX_ALPHA256) -> np.ndarray:
    """The host twin of HipVisualizer.draw_instance_predictions: masks [n,H,W], classes / scores [n]; boxes float32 [n,4] XYXY (None:
    the instances carry none) are drawn as frames, order the instances and anchor the texts."""
    colors = instance_colors(classes, metadata)
    if boxes is not None:
        h, w = np.asarray(image).shape[:2]
        bw = default_box_width(h, w) if box_width is None else int(box_width)
        pic = instance_overlay_boxes(image, masks, boxes, colors, instance_edge_colors(colors), alpha256, scores, min_score, bw, box_alpha256)
        anchors = instance_anchors_boxes(masks, boxes, scores, min_score)
        order = instance_order_boxes(masks, boxes, scores, min_score)
    else:
        pic = instance_overlay(image, masks, colors, instance_edge_colors(colors), alpha256, scores, min_score)
        anchors = instance_anchors(masks, scores, min_score)
        order = instance_order(masks, scores, min_score)
    kept = sorted((i for i in range(len(anchors)) if order[i] >= 0), key=lambda i: order[i])
    return draw_texts(pic, anchors[kept], instance_texts(classes, scores, metadata))


class HipVisualizer:
    """`Visualizer(image, metadata).draw_panoptic_seg(panoptic_seg, segments_info)` for a result that is still on the device.

    No pixel parity with detectron2's matplotlib rendering is claimed: the rules (which pixels belong to a label, where it goes) are
    its rules; the rasterisation is this project's."""

    def __init__(self, ctx, metadata=None, alpha: float = 0.5, edge_rgb=(0, 0, 0), small_area: int = SMALL_AREA, large_area: int = LARGE_AREA,
                 max_anchors: int = 256):
        self.ctx, self.metadata = ctx, metadata
        self.alpha256 = int(round(alpha * 256))
        self.edge_rgb, self.small_area, self.large_area, self.max_anchors = tuple(edge_rgb), int(small_area), int(large_area), int(max_anchors)

    def draw_panoptic_seg(self, image_dev, record_dev, hw) -> np.ndarray:
        """image_dev uint8 [h,w,3] and the panoptic record int32 [h*w | 1 | 3*MAX_SEGMENTS] on the device -> host uint8 [h,w,3].
        Overlay and anchors on the device, one read-back of the picture and the anchor rows (the table travels first: its rows choose
        the colours), the names drawn at the anchors."""
        from ._lib import MAX_SEGMENTS, split_record
        ctx = self.ctx
        ids, table = split_record(record_dev, hw)
        tail = table.numpy()
        n = min(max(int(tail[0]), 0), MAX_SEGMENTS)
        segments = tail[1:1 + 3 * n].reshape(n, 3)
        colors = ctx.to_device(np.ascontiguousarray(segment_colors(segments, self.metadata).reshape(-1, 3)) if n else np.zeros((1, 3), np.uint8))
        pic = ctx.panoptic_overlay(image_dev, ids, table, colors, self.alpha256, self.edge_rgb)
        anchors, count = ctx.segment_anchors(ids, table, self.small_area, self.large_area, self.max_anchors)
        picture, rows, found = pic.numpy(), anchors.numpy(), int(count.numpy()[0])
        return draw_labels(picture, rows[:min(found, self.max_anchors)], segments, self.metadata)


    def draw_sem_seg(self, image_dev, labels_or_sem_seg, K: Optional[int] = None) -> np.ndarray:
        """`draw_sem_seg(predictions["sem_seg"].argmax(0))`: labels int32 [h,w] (the fused arg-max map; needs K) or sem_seg float32
        [K,h,w] on the device -> host uint8 [h,w,3].  odise_hip_semantic_record turns the result into a record of stuff rows, which is
        drawn as a panoptic one."""
        h, w = labels_or_sem_seg.shape[-2:]
        return self.draw_panoptic_seg(image_dev, self.ctx.semantic_record(labels_or_sem_seg, K), (h, w))

    def _instance_draw(self, out_hw, topk, boxes: bool, box_width, box_alpha256, **kw) -> dict:
        """ctx.instance_draw, or with boxes: odise_hip_instance_boxes of the same selection, then ctx.instance_draw_boxes (nothing is
        read back between them)."""
        if not boxes:
            return self.ctx.instance_draw(out_hw, topk, **kw)
        bx = self.ctx.instance_boxes(out_hw, topk, kw.get("table_row"), b=kw.get("b", 0), pad_hw=kw.get("pad_hw", (0, 0)), img_hw=kw.get("img_hw", (0, 0)))
        bw = default_box_width(int(out_hw[0]), int(out_hw[1])) if box_width is None else int(box_width)
        return self.ctx.instance_draw_boxes(out_hw, topk, bx, bw, box_alpha256, self.small_area, **kw)

    def draw_instance_predictions(self, image_dev, b, table_row, scores_row, topk, pad_hw, img_hw, out_hw, min_score: float = 0.0,
                                  boxes: bool = False, box_width: Optional[int] = None, box_alpha256: int = BOX_ALPHA256) -> np.ndarray:
        """`draw_instance_predictions(predictions["instances"])` for the selection of image b of the last head forward, as it lies on the
        device (table_row int32 [1 + 2 topk], scores_row float32 [topk]) -> host uint8 [h,w,3].  The table and the scores travel first
        (their classes choose colours and texts), the masks never do: overlay, anchors and order on the device, one read-back, then
        "<class> <score>%" at the anchors, in draw order.  boxes=True: the instances carry the boxes of their masks
        (odise_hip_instance_boxes) and are drawn as detectron2 draws instances with boxes (odise_hip_instance_draw_boxes)."""
        ctx, topk = self.ctx, int(topk)
        table, scores = table_row.numpy().reshape(-1), scores_row.numpy().reshape(-1)
        n = min(max(int(table[0]), 0), topk)
        classes = table[1 + topk:1 + topk + n]
        colors = np.zeros((topk, 3), np.uint8)
        colors[:n] = instance_colors(classes, self.metadata)
        res = self._instance_draw(out_hw, topk, boxes, box_width, box_alpha256, table_row=table_row, scores_row=scores_row, b=b, pad_hw=pad_hw,
                                  img_hw=img_hw, min_score=min_score, image=image_dev, colors=ctx.to_device(colors),
                                  edge_colors=ctx.to_device(instance_edge_colors(colors)), alpha256=self.alpha256)
        picture, anchors, order = res["out"].numpy(), res["anchors"].numpy(), res["order"].numpy()
        kept = sorted((i for i in range(n) if order[i] >= 0), key=lambda i: order[i])
        return draw_texts(picture, anchors[kept], instance_texts(classes, scores[:n], self.metadata))


class HipVideoVisualizer(HipVisualizer):
    """detectron2 `VideoVisualizer(metadata)` for results that are still on the device: `draw_panoptic_seg_predictions` per frame, with
    the colours of things carried from frame to frame by the library's tracker (odise_hip_track_frame; the rule: odise_amd/video.py).
    `draw_instance_predictions` does the same for the overlapping masks of the instance head (odise_hip_inst_track_frame; mask IoU,
    detectron2's rule for instances without a box - the reference's zero boxes give every instance a fresh colour in every frame).
    `draw_sem_seg` is HipVisualizer's per-picture call: semantic maps are not tracked."""

    def __init__(self, ctx, metadata=None, ttl: int = 8, pool=None, **kwargs):
        super().__init__(ctx, metadata, **kwargs)
        self.ttl, self.pool, self.tracker, self.inst_tracker, self.box_tracker = int(ttl), pool, None, None, None

    def reset(self) -> None:
        for t in (self.tracker, self.inst_tracker, self.box_tracker):
            if t is not None:
                t.reset()

    def close(self) -> None:
        for t in (self.tracker, self.inst_tracker, self.box_tracker):
            if t is not None:
                t.close()
        self.tracker, self.inst_tracker, self.box_tracker = None, None, None

    def _draw_tracked_boxes(self, frame_dev, b, table_row, scores_row, topk, pad_hw, img_hw, hw, min_score, labels, box_width, box_alpha256):
        """Per frame on the device, nothing read back in between: odise_hip_instance_boxes, the box tracker, odise_hip_instance_draw_boxes"""
        ctx = self.ctx
        if self.box_tracker is None:
            self.box_tracker = ctx.box_track_create(topk, self.ttl, self.pool)
        if self.box_tracker.topk != topk:
            raise ValueError(f"a frame of {topk} instances for a tracker of {self.box_tracker.topk}")
        table, scores = table_row.numpy().reshape(-1), scores_row.numpy().reshape(-1)
        n = min(max(int(table[0]), 0), topk)
        classes = table[1 + topk:1 + topk + n]
        host_colors = np.zeros((topk, 3), np.uint8)
        host_colors[:n] = instance_colors(classes, self.metadata)
        colors, edges = ctx.to_device(host_colors), ctx.to_device(instance_edge_colors(host_colors))
        bx = ctx.instance_boxes(hw, topk, table_row, b=b, pad_hw=pad_hw, img_hw=img_hw)
        ctx.box_track_frame(self.box_tracker, bx, table_row, scores_row, min_score, colors, edges)
        bw = default_box_width(*hw) if box_width is None else int(box_width)
        want = ("out", "anchors", "order") if labels else ("out",)
        res = ctx.instance_draw_boxes(hw, topk, bx, bw, box_alpha256, self.small_area, table_row=table_row, scores_row=scores_row, b=b, pad_hw=pad_hw,
                                      img_hw=img_hw, min_score=min_score, image=frame_dev, colors=colors, edge_colors=edges, alpha256=self.alpha256,
                                      want=want)
        if not labels:
            return res["out"].numpy()
        picture, anchors, order = res["out"].numpy(), res["anchors"].numpy(), res["order"].numpy()
        kept = sorted((i for i in range(n) if order[i] >= 0), key=lambda i: order[i])
        return draw_texts(picture, anchors[kept], instance_texts(classes, scores[:n], self.metadata))

    def draw_instance_predictions(self, frame_dev, b, table_row, scores_row, topk, pad_hw, img_hw, out_hw, min_score: float = 0.0,
                                  labels: bool = True, boxes: bool = False, box_width: Optional[int] = None,
                                  box_alpha256: int = BOX_ALPHA256, track_boxes: Optional[bool] = None) -> np.ndarray:
        """HipVisualizer.draw_instance_predictions with the colours of the library's instance tracker: the fill and outline colours of the
        frame's instances are written on the device and drawn from there; the masks never travel (labels=False: the picture before the
        texts are drawn).  The tracker is made at the first frame, for its size and its topk; another size or topk is an error.
        boxes=True: the instances carry the boxes of their masks, the colours come from the BOX tracker (odise_hip_box_track_frame: box
        IoU above 0.6, detectron2's first path; no pixels are retained) and the boxes are drawn.  track_boxes=False with boxes=True
        draws the boxes and keeps the colours of the mask tracker."""
        ctx, topk = self.ctx, int(topk)
        h, w = int(out_hw[0]), int(out_hw[1])
        if boxes and (track_boxes is None or track_boxes):
            return self._draw_tracked_boxes(frame_dev, b, table_row, scores_row, topk, pad_hw, img_hw, (h, w), min_score, labels, box_width, box_alpha256)
        if self.inst_tracker is None:
            self.inst_tracker = ctx.inst_track_create((h, w), topk, self.ttl, self.pool)
        if self.inst_tracker.hw != (h, w) or self.inst_tracker.topk != topk:
            raise ValueError(f"a {h}x{w} frame of {topk} instances for a tracker of {self.inst_tracker.hw[0]}x{self.inst_tracker.hw[1]} "
                             f"and {self.inst_tracker.topk}")
        table, scores = table_row.numpy().reshape(-1), scores_row.numpy().reshape(-1)
        n = min(max(int(table[0]), 0), topk)
        classes = table[1 + topk:1 + topk + n]
        host_colors = np.zeros((topk, 3), np.uint8)
        host_colors[:n] = instance_colors(classes, self.metadata)          # what a row has before the tracker; drawn rows are rewritten
        colors, edges = ctx.to_device(host_colors), ctx.to_device(instance_edge_colors(host_colors))
        ctx.inst_track_frame(self.inst_tracker, table_row, scores_row, b=b, pad_hw=pad_hw, img_hw=img_hw, min_score=min_score, colors=colors,
                             edge_colors=edges)
        want = ("out", "anchors", "order") if labels else ("out",)
        res = self._instance_draw((h, w), topk, boxes, box_width, box_alpha256, table_row=table_row, scores_row=scores_row, b=b, pad_hw=pad_hw,
                                  img_hw=img_hw, min_score=min_score, image=frame_dev, colors=colors, edge_colors=edges, alpha256=self.alpha256, want=want)
        if not labels:
            return res["out"].numpy()
        picture, anchors, order = res["out"].numpy(), res["anchors"].numpy(), res["order"].numpy()
        kept = sorted((i for i in range(n) if order[i] >= 0), key=lambda i: order[i])
        return draw_texts(picture, anchors[kept], instance_texts(classes, scores[:n], self.metadata))

    def draw_panoptic_seg_predictions(self, frame_dev, record_dev, hw, labels: bool = True) -> np.ndarray:
        """frame_dev uint8 [h,w,3] and the frame's panoptic record on the device -> host uint8 [h,w,3] (labels=False: before the names
        are drawn).  The table travels first (its rows choose the stuff colours and the names); the map never does: the tracker, the
        overlay and the anchors read it where it lies.  The tracker is made at the first frame's size; another size is an error."""
        from ._lib import MAX_SEGMENTS, split_record
        ctx = self.ctx
        h, w = int(hw[0]), int(hw[1])
        ids, table = split_record(record_dev, hw)   # checks the size before a tracker is made
        if self.tracker is None:
            self.tracker = ctx.track_create((h, w), self.ttl, self.pool)
        if self.tracker.hw != (h, w):
            raise ValueError(f"a {h}x{w} frame for a tracker of {self.tracker.hw[0]}x{self.tracker.hw[1]}")
        tail = table.numpy()
        n = min(max(int(tail[0]), 0), MAX_SEGMENTS)
        segments = tail[1:1 + 3 * n].reshape(n, 3)
        host_colors = np.zeros((MAX_SEGMENTS, 3), np.uint8)
        host_colors[:n] = segment_colors(segments, self.metadata)
        colors = ctx.track_frame(self.tracker, ids, table, ctx.to_device(host_colors))
        pic = ctx.panoptic_overlay(frame_dev, ids, table, colors, self.alpha256, self.edge_rgb)
        if not labels:
            return pic.numpy()
        anchors, count = ctx.segment_anchors(ids, table, self.small_area, self.large_area, self.max_anchors)
        picture, rows, found = pic.numpy(), anchors.numpy(), int(count.numpy()[0])
        return draw_labels(picture, rows[:min(found, self.max_anchors)], segments, self.metadata)
