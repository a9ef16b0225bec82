"""Polygon annotations to COCO run lengths on the host (numpy): pycocotools' `annToRLE` - maskApi.c `rleFrPoly` for every polygon,
`rleMerge` as a union - restated, the reference of `Context.polygon_rle` / `odise_hip_instance_eval_poly` (csrc/poly.hip).

`polygon_counts` is rleFrPoly the way it is written there, loop by loop, in Python floats (C doubles) and ints; `int()` truncates toward
zero as the C cast does.  `polygon_mask` is the second, independent formulation, the one the device uses: every crossing toggles one
position of the column-major order and the mask is the running XOR of the toggles - nothing is sorted, no zero run is folded - written
with numpy arrays per edge.  tests/test_polygon_cpu.py holds the two against each other.

A zero-length edge (two equal consecutive vertices after scaling) has the slope 0 / 0 in maskApi.c; its single point shares its x with
both neighbours, so the y computed from that slope is never read.  Here it is 0.
"""
from __future__ import annotations

import math

import numpy as np

from . import coco_rle

SCALE = 5.0
MAX_COORD = float(1 << 26)          # 5 x + .5 must fit a C int (odise_hip_polygon_rle flag 8)


def check_polygon(xy) -> np.ndarray:
    """float64 [2 k] of a polygon given as a flat list x0 y0 x1 y1 ..; ValueError for an odd length, fewer than three vertices, or a
    coordinate that is NaN or beyond 2^26."""
    p = np.asarray(xy, np.float64).reshape(-1)
    if p.size % 2 or p.size < 6:
        raise ValueError(f"a polygon is a flat list of at least three x, y pairs (got {p.size} numbers)")
    if not (np.abs(p) <= MAX_COORD).all():
        raise ValueError("a polygon coordinate is NaN or larger than 2^26 in magnitude")
    return p


def _scaled(xy):
    p = check_polygon(xy)
    k = p.size // 2
    x = [int(SCALE * float(p[2 * j]) + .5) for j in range(k)]
    y = [int(SCALE * float(p[2 * j + 1]) + .5) for j in range(k)]
    return x + [x[0]], y + [y[0]], k


def polygon_counts(xy, h: int, w: int) -> np.ndarray:
    """maskApi.c rleFrPoly: the uncompressed counts (int64) of one polygon on an h x w picture."""
    x, y, k = _scaled(xy)
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = float(ye - ys) / dx if dx else math.nan
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(0 if dx == 0 else int(ys + s * t + .5))
        else:
            s = float(xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    a = []
    for j in range(1, len(u)):
        if u[j] != u[j - 1]:
            xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
            xd = (xd + .5) / SCALE - .5
            if math.floor(xd) != xd or xd < 0 or xd > w - 1:
                continue
            yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
            yd = (yd + .5) / SCALE - .5
            if yd < 0:
                yd = 0.0
            elif yd > h:
                yd = float(h)
            yd = math.ceil(yd)
            a.append(int(xd) * h + int(yd))
    a.append(h * w)
    a.sort()
    p = 0
    for j in range(len(a)):
        t = a[j]
        a[j] -= p
        p = t
    b = [a[0]]
    j = 1
    while j < len(a):
        if a[j] > 0:
            b.append(a[j])
            j += 1
        else:
            j += 1
            if j < len(a):
                b[-1] += a[j]
                j += 1
    return np.asarray(b, np.int64)


def polygon_toggles(xy, h: int, w: int) -> np.ndarray:
    """uint8 [h * w + 1]: the parity of the crossings at every position of the column-major order (position h * w: past the picture)."""
    x, y, k = _scaled(xy)
    tog = np.zeros(h * w + 1, np.uint8)
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        n = max(dx, dy)
        if n == 0:
            continue
        wide = dx >= dy
        flip = (wide and xs > xe) or (not wide and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        t = np.arange(n + 1, dtype=np.int64)
        if flip:
            t = n - t
        tf = t.astype(np.float64)
        if wide:
            s = np.float64(ye - ys) / np.float64(dx)
            u, v = t + xs, (np.float64(ys) + s * tf + .5).astype(np.int64)          # multiply and add rounded separately
        else:
            s = np.float64(xe - xs) / np.float64(dy)
            v, u = t + ys, (np.float64(xs) + s * tf + .5).astype(np.int64)
        step = np.flatnonzero(u[1:] != u[:-1]) + 1
        if not step.size:
            continue
        xd = np.where(u[step] < u[step - 1], u[step], u[step] - 1).astype(np.float64)
        xd = (xd + .5) / SCALE - .5
        ok = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
        yd = np.minimum(v[step], v[step - 1]).astype(np.float64)
        yd = np.ceil(np.clip((yd + .5) / SCALE - .5, 0, h))
        pos = xd[ok].astype(np.int64) * h + yd[ok].astype(np.int64)
        np.bitwise_xor.at(tog, pos, 1)
    return tog


def polygon_mask(xy, h: int, w: int) -> np.ndarray:
    """uint8 [h, w] mask of one polygon: the running XOR of `polygon_toggles`."""
    tog = polygon_toggles(xy, h, w)
    return (np.cumsum(tog[: h * w], dtype=np.int64) & 1).astype(np.uint8).reshape((h, w), order="F")


def merge_counts(list_of_counts, h: int, w: int) -> np.ndarray:
    """rleMerge with intersect = 0: the counts of the union of several run-length masks (none: the empty mask)."""
    cover = np.zeros(h * w + 1, np.int64)
    for cnts in list_of_counts:
        c = np.asarray(cnts, np.int64).reshape(-1)
        if int(c.sum()) != h * w:
            raise ValueError(f"run lengths sum to {int(c.sum())}, the picture has {h * w} pixels")
        ends = np.cumsum(c)
        np.add.at(cover, ends[0::2][: len(ends[1::2])], 1)                            # a run of ones starts where a run of zeros ends
        np.add.at(cover, ends[1::2], -1)
    flat = (np.cumsum(cover[: h * w]) > 0).astype(np.uint8)
    return coco_rle.mask_counts(flat.reshape((h, w), order="F"))


def annotation_to_counts(segmentation, h: int, w: int) -> np.ndarray:
    """pycocotools' annToRLE as uncompressed counts: a list of polygons is rasterised and merged, an RLE dict passes through (`counts` a
    list of run lengths, or a compressed string / bytes)."""
    if isinstance(segmentation, dict):
        c = segmentation["counts"]
        if isinstance(c, (bytes, bytearray)):
            c = c.decode("utf-8")
        return coco_rle.string_to_counts(c) if isinstance(c, str) else np.asarray(c, np.int64)
    polys = [check_polygon(p) for p in segmentation]
    if len(polys) == 1:
        return polygon_counts(polys[0], h, w)
    return merge_counts([polygon_counts(p, h, w) for p in polys], h, w)


def pack_polygons(annotations_polys):
    """[[polygon, ..] per annotation] -> (xy float64, poly_offsets int64 [n_poly + 1] in vertices, ann_polys int32 [n_ann + 1]): the
    arguments of odise_hip_polygon_rle.  Malformed polygons raise ValueError."""
    xy, offs, ann = [], [0], [0]
    for polys in annotations_polys:
        for p in polys:
            p = check_polygon(p)
            xy.append(p)
            offs.append(offs[-1] + p.size // 2)
        ann.append(len(offs) - 1)
    return (np.concatenate(xy) if xy else np.zeros(0, np.float64)), np.asarray(offs, np.int64), np.asarray(ann, np.int32)
