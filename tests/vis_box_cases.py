"""Instance masks WITH boxes for the box-drawing tests (tests/test_visualize_boxes_cpu.py, tests/test_gpu_visualize_boxes.py): the
shapes of tests/vis_inst_cases.py - 1 x 1, 64 x 64 (one tile, exactly full), 70 x 45 and 130 x 33 (ragged tiles, two and three word rows),
200 x 37 with 100 masks (two chunks of staged masks) - and what boxes add: boxes that are not tight to their masks, a box crossing a tile
edge, a box leaving the picture, frames 1 and 3 wide and wider than the box, frame alphas 0 / 128 / 256, equal box areas, a frame in a tile
no mask touches, and a label on either side of each small-box condition.  The references (odise_amd.visualize, the restatement) are
computed once per case and shared."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from odise_amd import instance_eval as IE
from odise_amd import visualize as V
from vis_inst_cases import _blob_masks, _scores


@dataclass
class BoxCase:
    name: str
    masks: np.ndarray                     # bool [topk,H,W]
    boxes: np.ndarray                     # float32 [topk,4] XYXY
    scores: Optional[np.ndarray] = None
    min_score: float = 0.0
    n: Optional[int] = None               # the table's count (None: no table)
    box_width: int = 1
    box_alpha256: int = 128
    small_area: int = 1000
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def topk(self):
        return len(self.masks)

    @property
    def hw(self):
        return self.masks.shape[1:]

    def count(self):
        return self.topk if self.n is None else self.n

    def live_scores(self):
        return None if self.scores is None else self.scores[:self.count()]

    def table(self):
        if self.n is None:
            return None
        t = np.zeros(1 + 2 * self.topk, np.int32)
        t[0] = self.n
        t[1:1 + self.topk] = np.arange(self.topk)
        return t

    def image(self):
        h, w = self.hw
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)

    def colors(self):
        return np.random.default_rng(self.topk).integers(0, 256, (self.topk, 3), dtype=np.uint8)

    def edge_colors(self):
        return np.random.default_rng(self.topk + 1000).integers(0, 256, (self.topk, 3), dtype=np.uint8)

    def _memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def anchors(self):
        return self._memo("anchors", lambda: V.instance_anchors_boxes(self.masks[:self.count()], self.boxes, self.live_scores(), self.min_score, self.topk,
                                                                      self.small_area))

    def order(self):
        return self._memo("order", lambda: V.instance_order_boxes(self.masks[:self.count()], self.boxes, self.live_scores(), self.min_score, self.topk))

    def overlay(self):
        return self._memo("overlay", lambda: V.instance_overlay_boxes(self.image(), self.masks[:self.count()], self.boxes, self.colors(), self.edge_colors(), 128,
                                                                      self.live_scores(), self.min_score, self.box_width, self.box_alpha256))


def loose(masks, seed, grow=4):
    """the tight boxes of the masks, each side moved by up to `grow` pixels either way (fractions included): not tight, some leave the picture"""
    rng = np.random.default_rng(seed)
    b = IE.mask_boxes(masks).astype(np.float32)
    return (b + rng.integers(-4 * grow, 4 * grow + 1, b.shape).astype(np.float32) / 4).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = []
    one = np.ones((1, 1, 1), bool)
    out.append(BoxCase("one_pixel", one, np.array([[0, 0, 1, 1]], np.float32)))
    out.append(BoxCase("one_pixel_wide_frame", one, np.array([[-2, -2, 3, 3]], np.float32), box_width=7, box_alpha256=256))
    for (h, w), bw, ba in (((64, 64), 1, 128), ((70, 45), 3, 256), ((130, 33), 1, 0), ((200, 37), 3, 128)):
        m = _blob_masks(h * 100 + w, 5, h, w)
        out.append(BoxCase(f"tight_{h}x{w}", m, IE.mask_boxes(m), _scores(h + w, 5), 0.2, box_width=bw, box_alpha256=ba))
        out.append(BoxCase(f"loose_{h}x{w}", m, loose(m, h + w), _scores(h + w, 5), 0.2, n=5, box_width=bw, box_alpha256=ba, small_area=300))
        # filled rectangles with their tight boxes: the box area is the pixel count, so the box order is the mask order
        rng = np.random.default_rng(h + 7 * w)
        r = np.zeros((6, h, w), bool)
        for i in range(5):                                # the sixth stays empty
            y0, x0 = int(rng.integers(0, h - 1)), int(rng.integers(0, w - 1))
            r[i, y0:y0 + int(rng.integers(1, h)), x0:x0 + int(rng.integers(1, w))] = True
        r[4] = r[1]                                       # equal areas
        out.append(BoxCase(f"rects_{h}x{w}", r, IE.mask_boxes(r), None, 0.0, box_width=bw, box_alpha256=0))
    m = _blob_masks(1, 3, 20, 30)
    out.append(BoxCase("n0", m, IE.mask_boxes(m), _scores(1, 3), 0.0, n=0))
    m = _blob_masks(2, 3, 33, 70)
    out.append(BoxCase("n1", m, np.array([[60, 2, 69.5, 30], [0, 0, 70, 33], [0, 0, 70, 33]], np.float32), _scores(2, 3), 0.0, n=1, box_width=3))
    many = np.zeros((100, 200, 37), bool)
    y, x = np.mgrid[0:200, 0:37]
    rng = np.random.default_rng(7)
    for i in range(100):
        cy, cx, r = 100 + rng.integers(-80, 81), 18 + rng.integers(-10, 11), (6, 9, 9, 14, 20)[i % 5]
        many[i] = (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    many[41] = many[17]
    bx = IE.mask_boxes(many)
    bx[63] = bx[17] + np.float32(3)                       # equal box areas at another place, and two equal boxes (17, 41)
    out.append(BoxCase("n100", many, bx, _scores(3, 100), 0.1, n=100, box_width=3))
    # 130 x 150: six tiles.  Boxes crossing tile edges, leaving the picture, in a tile no mask touches, narrower than twice the frame
    sp = np.zeros((8, 130, 150), bool)
    sp[:, 2:6, 2:6] = True                                # every mask lives in the first tile
    sb = np.array([[50, 50, 80, 80],                      # over the corner of four tiles
                   [100, 70, 148, 120],                   # tiles no mask touches
                   [-20.5, -7.25, 30, 40],                # leaves at the top left
                   [120, 100, 400, 300],                  # leaves at the bottom right
                   [70, 10, 74, 60],                      # 4 wide, frame 3: all frame
                   [10, 100, 10, 120],                    # no width: not kept
                   [20, 70, 60, 110],                     # 40 x 40 ...
                   [90, 5, 130, 45]], np.float32)         # ... and again: equal areas
    out.append(BoxCase("frames", sp, sb, None, 0.0, box_width=3, box_alpha256=256))
    out.append(BoxCase("frames_thin", sp, sb, None, 0.0, n=8, box_width=1, box_alpha256=128))
    out.append(BoxCase("frames_huge_width", sp, sb, None, 0.0, box_width=1 << 30, box_alpha256=128))
    # where the label goes: h = 130, small_area 1000.  area >= 1000 and 40 high: the corner; 39 high; area 999.75; and each of the two
    # again with y1 on either side of h - 5 = 125
    lb = np.array([[10, 10, 35, 50], [10, 10, 140, 49], [10, 10, 34.99375, 50], [10, 90, 35, 130], [10, 86, 140, 125], [10, 85.5, 140, 124.5],
                   [10, 100, 20, 125], [10, 100, 20, 124.75]], np.float32)
    out.append(BoxCase("labels", sp, lb, None, 0.0, box_width=1))
    nf = sb.copy()
    nf[0, 2], nf[1, 0], nf[2, 3] = np.nan, np.inf, -np.inf
    out.append(BoxCase("non_finite", sp, nf, None, 0.0, box_width=3))
    return {c.name: c for c in out}


def hand_cases():
    """Two hand-worked pictures: (masks, boxes, ..., anchors as tuples, order, picture)"""
    a = np.zeros((2, 4, 6), bool)
    a[0, 1, 1] = True
    a[1, 3, 5] = True
    # box 0 = columns 0..3, rows 0..2 (area 12), frame 1: all of it but (1,1), (1,2); its mask pixel (1,1) is an edge pixel.  box 1 =
    # columns 4..5, rows 2..3 (area 4), all frame; its mask pixel (3,5) -> edge colour.  Frame alpha 256: the colour itself.  h - 5 < 0
    # <= y1: small boxes (small_area 5 > 4, and lower than 40 rows) put the label at (x1, y0).
    ha = dict(masks=a, boxes=np.array([[0, 0, 4, 3], [4.5, 2.25, 6, 4]], np.float32), scores=None, min_score=0.0, image=np.full((4, 6, 3), 100, np.uint8),
              colors=[(200, 0, 0), (0, 0, 200)], edge_colors=[(1, 2, 3), (4, 5, 6)], alpha256=128, box_width=1, box_alpha256=256, small_area=5,
              anchors=[(0, 1, 8, 0, 0, 0, 4, 3), (1, 1, 12, 4, 4, 2, 6, 4)], order=[0, 1],
              picture=[[(200, 0, 0)] * 4 + [(100, 100, 100)] * 2,
                       [(200, 0, 0), (1, 2, 3), (100, 100, 100), (200, 0, 0), (100, 100, 100), (100, 100, 100)],
                       [(200, 0, 0)] * 4 + [(0, 0, 200)] * 2,
                       [(100, 100, 100)] * 4 + [(0, 0, 200), (4, 5, 6)]])
    b = np.zeros((2, 50, 3), bool)
    b[0, 0, 0] = True                                     # one pixel, a box over the whole picture: 3 x 50 = 150 >= small_area 150, 50 high
    b[1, 49, 2] = True                                    # the larger MASK does not matter: box 1 is 2 x 2
    b[1, 48, 2] = True
    pic = np.zeros((50, 3, 3), np.uint8)
    pic[:, 0] = pic[:, 2] = pic[0] = pic[49] = (20, 40, 60)            # frame alpha 128 of (40, 80, 120) over black: (c * 128 + 128) >> 8
    pic[0, 0] = (9, 9, 9)                                              # mask 0's pixel: an edge
    pic[48, 1] = (20, 40, 60)                                          # box 1 = columns 1..2, rows 48..49, colour (0, 0, 0): blends to
    pic[49, 1] = (10, 20, 30)                                          # half of what is there: (20 * 128 + 128) >> 8 = 10, ...
    pic[48, 2] = pic[49, 2] = (7, 7, 7)                                # mask 1: two edge pixels
    pic[48, 1] = (0, 0, 0)                                             # (48, 1) was black (inside box 0's interior): stays black
    hb = dict(masks=b, boxes=np.array([[0, 0, 3, 50], [1, 48, 3, 50]], np.float32), scores=np.array([0.5, 0.9], np.float32), min_score=0.5,
              image=np.zeros((50, 3, 3), np.uint8), colors=[(40, 80, 120), (0, 0, 0)], edge_colors=[(9, 9, 9), (7, 7, 7)], alpha256=256, box_width=1,
              box_alpha256=128, small_area=150,
              anchors=[(0, 1, 0, 0, 0, 0, 3, 50), (1, 2, 6, 96, 1, 48, 3, 50)], order=[0, 1], picture=pic.tolist())
    return [ha, hb]
