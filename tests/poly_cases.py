"""Crafted polygons of the rasterisation tests (tests/test_polygon_cpu.py, tests/test_gpu_polygon.py): per picture size a list of
annotations (each a list of polygons, a polygon a flat list x0 y0 x1 y1 ..) that take rleFrPoly through every branch an edge can take,
and the host reference of each, computed once."""
import functools
import math
from fractions import Fraction

import numpy as np

from odise_amd import coco_poly as P
from odise_amd import coco_rle as R

SIZES = [(1, 1), (5, 6), (64, 64), (70, 45), (129, 3), (96, 80)]          # 70: h % 64 != 0; 129 x 3: three words a column; 96 x 80: inst_cases
RANDOM_HW, RANDOM_N = (37, 29), 2000

HAND = {   # the two fixtures of the issue, on 5 x 6: polygon -> the mask's rows
    "rectangle": ([1, 1, 4, 1, 4, 3, 1, 3], ["000000", "011100", "011100", "000000", "000000"]),
    "triangle": ([0.5, 0.5, 5.5, 0.5, 3, 4.5], ["000000", "011110", "001100", "001100", "000000"]),
}


def rect_poly(y0, y1, x0, x1):
    """The polygon that decodes to inst_cases.rect(y0, y1, x0, x1): pycocotools' half-open rectangle."""
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def reverse(poly):
    p = np.asarray(poly, np.float64).reshape(-1, 2)[::-1]
    return [float(v) for v in p.reshape(-1)]


def shapes(h, w):
    """name -> polygon, scaled to the picture."""
    s = {}
    x0, x1, y0, y1 = math.floor(w / 4), math.ceil(3 * w / 4), math.floor(h / 4), math.ceil(3 * h / 4)
    s["rect_int"] = rect_poly(y0, y1, x0, x1)
    s["rect_half"] = rect_poly(y0 + .5, y1 + .5, x0 + .5, x1 + .5)
    s["rect_int_cw"] = reverse(s["rect_int"])
    s["rect_half_cw"] = reverse(s["rect_half"])
    m = min(h, w)
    s["tri_diag"] = [.2 * m, .2 * m, .8 * m, .8 * m, .2 * m, .8 * m]       # dx == dy, then a horizontal and a vertical edge
    s["tri_diag_cw"] = reverse(s["tri_diag"])
    s["tri_skew"] = [.3 * w, .2 * h, .9 * w, .35 * h, .45 * w, .95 * h]     # dx > dy, dx < dy, dx < dy in both directions over the two windings
    s["tri_skew_cw"] = reverse(s["tri_skew"])
    s["tri_flat"] = [.1 * w, .6 * h, .9 * w, .5 * h, .5 * w, .7 * h]        # shallow edges: dx > dy going right and going left
    s["tri_flat_cw"] = reverse(s["tri_flat"])
    s["out_left"] = [-3.7, .3 * h, .5 * w, .1 * h, .4 * w, .9 * h]
    s["out_right"] = [w + 4.2, .5 * h, .3 * w, .2 * h, .5 * w, .8 * h]
    s["out_top"] = [.5 * w, -5.5, .9 * w, .6 * h, .1 * w, .5 * h]
    s["out_bottom"] = [.5 * w, h + 6.3, .1 * w, .4 * h, .8 * w, .3 * h]
    s["around"] = [-2, -3, w + 2, -3, w + 3, h + 2, -1.5, h + 2.5]          # every vertex outside: the whole picture
    s["beside"] = [w + 1, 1, w + 9, 2, w + 5, h]                            # every vertex outside: nothing
    s["negative"] = [-0.25, -0.1, .6 * w, -0.1, .6 * w, .6 * h, -0.25, .6 * h]   # (int)(5 x + .5) truncates toward zero
    s["below"] = [w / 3, h / 2, w + 3, h / 2, w + 3, h + 4, w / 3, h + 4]   # crossings clamp to y == h in middle columns and in the last
    s["in_a_pixel"] = [min(2, w - 1) + .1, min(2, h - 1) + .1, min(2, w - 1) + .4, min(2, h - 1) + .1, min(2, w - 1) + .2, min(2, h - 1) + .4]
    r = s["rect_int"]
    s["collinear_repeated"] = [r[0], r[1], (r[0] + r[2]) / 2, r[1], r[2], r[3], r[2], r[3], r[4], r[5], r[4], r[5], r[4], r[5], r[6], r[7],
                               r[6], (r[7] + r[1]) / 2]
    s["bow_tie"] = [.1 * w, .1 * h, .9 * w, .9 * h, .9 * w, .1 * h, .1 * w, .9 * h]
    return s


def long_edge(h, w):
    """One edge of more than 1024 points (250 pixels, 1250 points): it starts and ends far outside the picture."""
    return [-100, .1 * h, 150, .7 * h, .4 * w, h + 20]


def circle(h, w, n=1500):
    """1500 vertices on a circle: more edges than one chunk of the edge scan, most of them of zero length after scaling."""
    a = np.arange(n) * (2 * np.pi / n)
    return [float(v) for v in np.stack([.5 * w + .35 * min(h, w) * np.cos(a), .5 * h + .35 * min(h, w) * np.sin(a)], 1).reshape(-1)]


# ---- the FMA case -------------------------------------------------------------------------------------------------------------------------
def _v_separate(ys, s, t):
    return int(ys + s * t + .5)


def _v_fused(ys, s, t):
    """(int)(fma(s, t, ys) + .5): the product enters the first sum unrounded."""
    return int(float(Fraction(s) * t + ys) + .5)


def _row(v):
    return math.ceil((v + .5) / 5 - .5)


@functools.lru_cache(None)
def fma_edges(limit=4):
    """Edges (dx, dy, t, ys), dx > dy > 0, walked left to right and FALLING (ys -> ys - dy, so the sum cancels and the rounding of the
    product shows), at whose point t a fused ys + s t + .5 truncates to another v than the separately rounded one AND the two v fall
    into different pixel rows.  Exact search with fractions over every edge of dx <= 120 that fits a 64 x 64 picture; s t + .5 is a whole
    number in exact arithmetic only where 2 dy t / dx is odd, and nowhere else can the two roundings straddle a truncation boundary."""
    found = []
    for dx in range(2, 121):
        for dy in range(1, dx):
            s = -float(dy) / dx
            for t in range(1, dx):
                if (2 * dy * t) % dx or not ((2 * dy * t) // dx) & 1:
                    continue
                top = (2 * dy * t // dx + 1) // 2                            # s t + .5 = 1 - top
                for ys in range(max(top, dy), min(top + 60, 300)):           # v = ys - top + 1 or one less; the edge stays at y >= 0
                    a, b = _v_separate(ys, s, t), _v_fused(ys, s, t)
                    if a != b and _row(a) != _row(b):
                        found.append((dx, dy, t, ys))
                        break
                if len(found) >= limit:
                    return tuple(found)
    return tuple(found)


def fma_polygons():
    """A triangle per edge of `fma_edges`: the edge starts where point t is the right end of a counted crossing (u - 1 = 5 m + 2); the
    edge falls, so the point's v is the smaller of the pair and decides the crossing's row."""
    out = []
    for dx, dy, t, ys in fma_edges():
        xs = 10 + (3 - t) % 5
        out.append([xs / 5, ys / 5, (xs + dx) / 5, (ys - dy) / 5, (xs + dx) / 5, (ys + 20) / 5])
    return out


# ---- the case set -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def annotations(h, w):
    """[[polygon, ..] per annotation] of a picture size: every shape alone, the unions, an annotation without polygons."""
    s = shapes(h, w)
    anns = [[p] for p in s.values()]
    anns.append([s["rect_int"], s["tri_skew"], s["bow_tie"]])              # three overlapping
    anns.append([rect_poly(0, h / 3, 0, w / 3), rect_poly(h / 2, h, w / 2, w)])   # two disjoint
    anns.append([])                                                         # none
    if (h, w) == (96, 80):
        anns += [[long_edge(h, w)], [circle(h, w)], [circle(h, w), long_edge(h, w)]]
    if (h, w) == (64, 64):
        anns += [[p] for p in fma_polygons()]
    return anns


@functools.lru_cache(None)
def random_annotations():
    """2000 polygons of 3..8 vertices with float coordinates that reach a little outside a 37 x 29 picture; every fifth on whole numbers."""
    g = np.random.default_rng(11)
    h, w = RANDOM_HW
    out = []
    for i in range(RANDOM_N):
        k = int(g.integers(3, 9))
        p = g.random((k, 2)) * (w + 8, h + 8) - 4
        if i % 5 == 0:
            p = np.round(p)
        out.append([[float(v) for v in p.reshape(-1)]])
    return out


@functools.lru_cache(None)
def reference(h, w, random=False):
    """(counts, strings, areas) of `annotations(h, w)` (or the random set) through the literal host formulation."""
    anns = random_annotations() if random else annotations(h, w)
    counts = [P.annotation_to_counts(a, h, w) for a in anns]
    return counts, [R.counts_to_string(c) for c in counts], [int(c[1::2].sum()) for c in counts]
