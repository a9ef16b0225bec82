"""Frame sequences for the colour tracker (odise_amd/video.py ColorTracker, csrc/track.hip) and what the restatement makes of them.

A case is a list of frames (ids int32 [H,W], table int32 [n,3] rows (id, isthing, category)) with a ttl and a colour pool.  `expected(case)`
runs ColorTracker over it once and keeps, per frame: the colours (of the pre-filled rows), the live rows after the frame and the IoU matrix
of the frame.  Sizes: 37 x 53 (odd width; the GPU test also uploads these one int32 past a 16-byte boundary), 64 x 64, and one 20-frame
sequence at 96 x 128.

Two things the rule cannot show on real masks, and where they are tested instead: the instances of a frame are disjoint, and an IoU above
0.5 with a live mask needs more than half of that mask's pixels, so ONE live row can never have two new instances above 0.5 - neither a
"second-best above 0.5" nor an arg-max tie above 0.5 exists.  `taken_best` and `tie` below are the nearest real sequences (second-best
and tie at or below 0.5); the matrix-level rule for the impossible ones is pinned on hand-written IoU matrices in tests/test_track_cpu.py.
"""
import functools

import numpy as np

from odise_amd import video as VD

SMALL, SQUARE, LONG = (37, 53), (64, 64), (96, 128)
STUFF = (1, 0, 7)                       # the background row most cases carry: id 1, stuff, category 7


def paint(hw, rects, fill=1):
    """rects (id, y0, x0, y1, x1), half-open, painted in order over a map of `fill`."""
    ids = np.full(hw, fill, np.int32)
    for i, y0, x0, y1, x1 in rects:
        ids[y0:y1, x0:x1] = i
    return ids


def table(*rows):
    return np.array(rows, np.int32).reshape(-1, 3)


class Case:
    def __init__(self, name, hw, frames, ttl=8, pool=None):
        self.name, self.hw, self.frames, self.ttl = name, hw, frames, ttl
        self.pool = VD.default_pool() if pool is None else np.asarray(pool, np.uint8).reshape(-1, 3)
        for ids, tab in frames:
            assert ids.shape == hw and ids.dtype == np.int32 and tab.dtype == np.int32 and len(tab) <= 100


def prefill(n=100):
    """What the caller put into `colors` before the call: a distinct triple per row."""
    r = np.arange(n)
    return np.stack([200 + r % 50, r, 255 - r], axis=1).astype(np.uint8)


def band(hw, x0, x1, thing=(5, 1, 2), y0=3, y1=7, extra=()):
    """one thing as a band of rows y0..y1 over columns x0..x1, on the stuff background"""
    return paint(hw, [(thing[0], y0, x0, y1, x1)] + list(extra)), table(STUFF, thing)


def background(hw):
    return paint(hw, []), table(STUFF)


def _gone(hw, ttl, gap):
    """a thing, `gap` frames without it, the thing again"""
    return [band(hw, 4, 14)] + [background(hw)] * gap + [band(hw, 4, 14)]


def _hundred(t):
    """100 things in 3 x 3 cells of a 20 x 20 grid, frame t: layout 0 in the cells (even row, even column), layout 1 in (odd, odd), by
    turns - they share no pixel - and categories that turn with t, so a frame does not match the same layout two, four.. frames back
    either: nothing ever matches and the live list fills to 8 x 100 rows"""
    layout = t & 1
    ids = np.zeros(SQUARE, np.int32)
    rows = []
    for k in range(100):
        cy, cx = 2 * (k // 10) + layout, 2 * (k % 10) + layout
        ids[3 * cy:3 * cy + 3, 3 * cx:3 * cx + 3] = k + 1
        rows.append((k + 1, 1, (k + t) % 9))
    return ids, table(*rows)


def _long():
    """20 frames at 96 x 128: three things at different speeds over two stuff regions; one leaves for a while, one changes category once"""
    rng = np.random.default_rng(20)
    frames = []
    for t in range(20):
        rects = [(2, 48, 0, 96, 128)]                                                   # second stuff region
        rows = [STUFF, (2, 0, 9)]
        rects.append((10, 10, 5 + 3 * t, 40, 45 + 3 * t))                               # fast, always matched
        rows.append((10, 1, 0))
        if not 6 <= t < 11:                                                             # away for five frames, back with its colour
            rects.append((11, 50, 60 + t, 80, 100 + t))
            rows.append((11, 1, 1))
        rects.append((12, 70, 10, 90, 40 + int(rng.integers(0, 4))))                    # jitters in width
        rows.append((12, 1, 2 if t != 13 else 3))                                       # another category for one frame: a new colour twice
        if t % 7 == 3:                                                                  # a short-lived thing
            rects.append((13, 0, 100, 8, 128))
            rows.append((13, 1, 0))
        frames.append((paint(LONG, rects), table(*rows)))
    return frames


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    # a thing moving two pixels a frame: 12 frames, across the ring wrap (iou 10 / 14)
    add("moving", SMALL, [band(SMALL, 2 + 2 * t, 14 + 2 * t) for t in range(12)])
    add("moving_square", SQUARE, [band(SQUARE, 2 + 2 * t, 14 + 2 * t) for t in range(12)])
    # IoU exactly 1/2 (areas 6 and 6, 4 in common) is no match; 5 in common is
    add("iou_half", SQUARE, [band(SQUARE, 0, 6, y0=0, y1=1), band(SQUARE, 2, 8, y0=0, y1=1)])
    add("iou_above_half", SQUARE, [band(SQUARE, 0, 6, y0=0, y1=1), band(SQUARE, 1, 7, y0=0, y1=1)])
    add("iou_half_small", SMALL, [band(SMALL, 0, 6, y0=0, y1=1), band(SMALL, 2, 8, y0=0, y1=1), band(SMALL, 3, 9, y0=0, y1=1)])
    # the same pixels under another category
    add("category", SQUARE, [band(SQUARE, 4, 14), band(SQUARE, 4, 14, thing=(5, 1, 3))])
    # two live rows claim one new instance: A (cols 0..9), then B (cols 4..13, iou 6/14 with A: no match) -> live [B, A]; N (cols 2..11) has
    # iou 8/12 with both: B, earlier in the list, gives its colour and A loses one ttl
    add("two_claim", SQUARE, [band(SQUARE, 0, 10), band(SQUARE, 4, 14), band(SQUARE, 2, 12)])
    add("two_claim_small", SMALL, [band(SMALL, 0, 10), band(SMALL, 4, 14), band(SMALL, 2, 12)])
    # the best new instance of a live row is taken and it does not fall back on its second-best: live [B, A] as above, then N1 (cols 2..11,
    # both rows' best at 32 / 48, to B) and N2 (cols 12..15: 8 / 48 with B, nothing with A) - A stays unmatched, N2 takes a new colour
    add("taken_best", SQUARE, [band(SQUARE, 0, 10), band(SQUARE, 4, 14),
                               (paint(SQUARE, [(5, 3, 2, 7, 12), (6, 3, 12, 7, 16)]), table(STUFF, (5, 1, 2), (6, 1, 2)))])
    # an arg-max tie: the live row (cols 0..11) meets two new instances of 4 columns each, both iou 16 / 48; the first maximum is the lower one
    add("tie", SQUARE, [band(SQUARE, 0, 12), (paint(SQUARE, [(8, 3, 0, 7, 4), (9, 3, 8, 7, 12)]), table(STUFF, (9, 1, 2), (8, 1, 2)))])
    # away for ttl - 1 frames: the colour returns (ttl is down to 1); away for ttl frames: a new colour
    for ttl, gap in ((8, 7), (8, 8), (3, 2), (3, 3), (1, 0), (1, 1)):
        add(f"gone{gap}_ttl{ttl}", SMALL if ttl == 8 else SQUARE, _gone(SMALL if ttl == 8 else SQUARE, ttl, gap), ttl=ttl)
    # more than one retained map: A (frame 0, cols 0..9) is unmatched for two frames while C lives elsewhere; D (frame 3, cols 6..15) overlaps
    # A's pixels without matching it; N (frame 4, cols 1..10) matches A from three frames back (9 / 11), not D (5 / 15)
    other = [(6, 20, 30, 26, 40)]
    tab2 = table(STUFF, (5, 1, 2), (6, 1, 2))
    add("three_back", SQUARE, [(paint(SQUARE, [(5, 3, 0, 7, 10)] + other), tab2), (paint(SQUARE, other), tab2), (paint(SQUARE, other), tab2),
                               (paint(SQUARE, [(5, 3, 6, 7, 16)] + other), tab2), (paint(SQUARE, [(5, 3, 1, 7, 11)] + other), tab2)])
    # 100 things a frame, two layouts that never match: the live list climbs to its cap of 800 rows and stays there, in order
    add("hundred", SQUARE, [_hundred(t) for t in range(11)])
    # table edge cases: none of these rows may be recoloured
    edge_ids = paint(SQUARE, [(5, 3, 4, 7, 14), (30, 10, 0, 12, 5), (0, 20, 0, 22, 9), (-4, 24, 0, 26, 9), (9, 30, 0, 34, 8), (12, 40, 0, 44, 8)])
    edge_tab = table(STUFF, (5, 1, 2),
                     (6, 1, 2),      # a thing row without a pixel
                     (5, 1, 4),      # a second row of id 5: the first one counts
                     (0, 1, 2),      # id 0
                     (-4, 1, 2),     # a negative id (the map has such pixels)
                     (9, 0, 3),      # stuff
                     (12, 0, 3), (12, 1, 2))   # a thing row behind a stuff row of the same id: not the first row of its id
    # id 30 of the map has no row
    add("table_edges", SQUARE, [(edge_ids, edge_tab), (edge_ids, edge_tab)])
    # an empty frame and an all-stuff frame: every live row loses one ttl
    add("empty_frame", SQUARE, [band(SQUARE, 4, 14), (np.zeros(SQUARE, np.int32), table()), band(SQUARE, 4, 14)])
    add("all_stuff", SMALL, [band(SMALL, 4, 14), (paint(SMALL, [(2, 0, 0, 5, 53)]), table(STUFF, (2, 0, 9))), band(SMALL, 4, 14)])
    # a pool of three colours: the counter wraps
    five = [(10 + k, 2 + 6 * k, 2, 6 + 6 * k, 12) for k in range(5)]
    tab5 = table(STUFF, *[(10 + k, 1, 2) for k in range(5)])
    shifted = [(i, y0, x0 + 20, y1, x1 + 20) for i, y0, x0, y1, x1 in five]
    add("pool3", SMALL, [(paint(SMALL, five), tab5), (paint(SMALL, shifted), tab5), (paint(SMALL, shifted), tab5)],
        pool=[(255, 0, 0), (0, 255, 0), (0, 0, 255)])
    add("long", LONG, _long())
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = cases()[name]
    tracker = VD.ColorTracker(case.ttl, case.pool)
    frames = []
    for ids, tab in case.frames:
        n_before = len(tracker.live)
        colors = prefill()
        colors[:len(tab)] = tracker.assign(ids, tab, colors[:len(tab)])
        frames.append({"colors": colors, "live": tracker.live_rows(), "iou": tracker.last_iou.copy(), "n_before": n_before})
    return frames


def expected(case):
    """per frame: colors uint8 [100,3] (prefill() with the instances recoloured), live rows after the frame, iou of the frame; computed
    once per case and shared - do not modify"""
    return _expected(case.name)
