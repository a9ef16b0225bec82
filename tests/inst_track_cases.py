"""Frame sequences for the instance-mask colour tracker (odise_amd/video.py InstanceColorTracker, csrc/inst_track.hip) and what the
restatement makes of them.

A frame is (classes int32 [n], scores float32 [n], masks bool [n,h,w]) with n <= topk; a case adds the size, topk, ttl, min_score and the
pool.  `expected(case)` runs InstanceColorTracker over it once and keeps, per frame: the colours (of the pre-filled rows), the live rows
after the frame and the IoU matrix of the frame.  `device_frame` lays a frame out as the library takes it: [topk,h,w] masks whose entries
past n are FULL masks with a passing score (the count alone must keep them out), the table n | query index | class.

Sizes are the smallest at which the packed layout ([n][w][ceil(h / 64)] words, bit = row) can go wrong: 1 x 1; 64 x 64 (one word row,
exactly full); 70 x 45 (two word rows, a ragged tail of six); 130 x 33 (three word rows); 200 x 37 with 100 masks (four word rows, more
than one tile of new masks and, once the list has filled, every tile of live rows).  Unlike the things of a panoptic map these masks
overlap, so one live row CAN have two new instances above 0.5 (`tie`) and two instances of one frame can claim the same successor
(`two_claim`).
"""
import functools

import numpy as np

from odise_amd import video as VD


def rect(hw, y0, x0, y1, x1):
    m = np.zeros(hw, bool)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    return m


def frame(hw, items):
    """items: (class, score, mask) -> (classes, scores, masks)"""
    n = len(items)
    masks = np.zeros((n,) + tuple(hw), bool)
    for k, (_, _, m) in enumerate(items):
        masks[k] = m
    return np.array([c for c, _, _ in items], np.int32), np.array([s for _, s, _ in items], np.float32), masks


class Case:
    def __init__(self, name, hw, topk, ttl, frames, min_score=0.5, pool=None):
        self.name, self.hw, self.topk, self.ttl, self.frames, self.min_score = name, tuple(hw), topk, ttl, frames, float(min_score)
        self.pool = VD.default_pool() if pool is None else np.asarray(pool, np.uint8).reshape(-1, 3)
        for classes, scores, masks in frames:
            assert masks.shape[1:] == self.hw and masks.dtype == bool and len(classes) == len(scores) == len(masks) <= topk


def prefill(n):
    """What the caller put into `colors` before the call: a distinct triple per row."""
    r = np.arange(n)
    return np.stack([200 + r % 50, r, 255 - r], axis=1).astype(np.uint8)


def device_frame(case, t, dtype=np.uint8):
    """-> (masks dtype [topk,h,w], table int32 [1 + 2 topk], scores float32 [topk])"""
    classes, scores, masks = case.frames[t]
    n, topk = len(masks), case.topk
    dense = np.ones((topk,) + case.hw, dtype)
    dense[:n] = masks.astype(dtype) * (3 if dtype == np.float32 else 1)       # any nonzero value is a pixel
    table = np.zeros(1 + 2 * topk, np.int32)
    table[0] = n
    table[1:1 + topk] = np.arange(topk)[::-1]                                  # query indices: not read on the dense route
    table[1 + topk:1 + topk + n] = classes
    table[1 + topk + n:] = classes[0] if n else 0                              # a class that would match, past the count
    full = np.ones(topk, np.float32)
    full[:n] = scores
    return dense, table, full


def _moving(hw, T, step=2, cls=2, size=(4, 12), y0=3):
    return [frame(hw, [(cls, 0.9, rect(hw, y0, 2 + step * t, y0 + size[0], 2 + step * t + size[1]))]) for t in range(T)]


def _gone(hw, ttl, gap):
    """A and B in frame 0; `gap` frames of something else (an empty selection, then a far-away mask); A again; B one frame later."""
    A, B, far = rect(hw, 0, 0, hw[0], 1), rect(hw, hw[0] - 3, hw[1] - 4, hw[0], hw[1]), rect(hw, hw[0] // 2, hw[1] // 2, hw[0] // 2 + 2, hw[1] // 2 + 3)
    between = [frame(hw, []) if k % 2 == 0 else frame(hw, [(5, 0.9, far)]) for k in range(gap)]
    return [frame(hw, [(1, 0.9, A), (1, 0.8, B)])] + between + [frame(hw, [(1, 0.9, A)]), frame(hw, [(1, 0.9, B)])] + _moving(hw, 5, 1, 3, (2, 5), 1)


def _never(hw, T, n=100):
    """n disjoint two-row strips whose classes turn with the frame (period 9 > 8 retained frames): nothing ever matches."""
    out = []
    for t in range(T):
        out.append(frame(hw, [((k + t) % 9, 0.9, rect(hw, 2 * k, 3 + k % 5, 2 * k + 2, 20 + k % 7)) for k in range(n)]))
    return out


def _random(hw, topk, T, seed, classes=3):
    rng = np.random.default_rng(seed)
    H, W = hw
    k0 = max(1, topk * 3 // 4)
    boxes = [[int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, H // 2 + 2)), int(rng.integers(1, W // 2 + 2)), int(rng.integers(0, classes))]
             for _ in range(k0)]
    out = []
    for _ in range(T):
        items = []
        for b in boxes:
            b[0] += int(rng.integers(-2, 3))
            b[1] += int(rng.integers(-2, 3))
            if rng.random() < 0.8:
                cls = b[4] if rng.random() < 0.9 else (b[4] + 1) % classes
                items.append((cls, float(rng.random()), rect(hw, b[0], b[1], b[0] + b[2], b[1] + b[3])))   # may fall outside: an empty mask
        order = rng.permutation(len(items))
        out.append(frame(hw, [items[k] for k in order][:topk]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    one, sq, two, three, big = (1, 1), (64, 64), (70, 45), (130, 33), (200, 37)
    px = np.ones(one, bool)
    # the only pixel: there, there (matched), gone, there again (ttl 1: a new colour), under another class, below the score
    add("one_pixel", one, 1, 1, [frame(one, [(0, 0.9, px)]), frame(one, [(0, 0.9, px)]), frame(one, [(0, 0.9, ~px)]), frame(one, [(0, 0.9, px)]),
                                  frame(one, [(1, 0.9, px)]), frame(one, [(1, 0.2, px)]), frame(one, []), frame(one, [(1, 0.5, px)])])
    add("moving", sq, 7, 3, _moving(sq, 10))
    add("moving_tall", three, 7, 8, _moving(three, 10, size=(100, 12), y0=20))                    # a mask over all three word rows
    # heavily overlapping masks of one class: seven nested / shifted rectangles that drift together
    add("overlap_one_class", sq, 7, 3, [frame(sq, [(4, 0.9, rect(sq, 5 + k, 3 + 2 * k + t, 50 + k, 30 + 2 * k + t)) for k in range(7)]) for t in range(9)])
    # equal masks under different classes: IoU 0 between them; the successor of class 1 is entry 1, not the equal mask of class 0 before it
    M = rect(two, 60, 4, 69, 30)
    add("equal_masks_other_class", two, 7, 3, [frame(two, [(1, 0.9, M)]), frame(two, [(0, 0.9, M), (1, 0.9, M)]), frame(two, [(1, 0.9, M), (0, 0.9, M), (2, 0.9, M)])] +
        [frame(two, [(2, 0.9, M)])] * 5)
    # IoU exactly 1/2 (six pixels each, four in common, the column crosses the word boundary at row 64) is no match; five in common is
    col = lambda y: rect(two, y, 7, y + 6, 8)
    add("iou_half", two, 7, 3, [frame(two, [(1, 0.9, col(60))]), frame(two, [(1, 0.9, col(62))]), frame(two, [(1, 0.9, col(63))]), frame(two, [(1, 0.9, col(64))])] +
        _moving(two, 4, 1, 1, (1, 6), 69))
    # two equal maxima in a row: the live mask meets two copies of itself; the first takes its colour, the second a new one
    L = rect(sq, 10, 10, 14, 13)
    add("tie", sq, 7, 3, [frame(sq, [(1, 0.9, L)]), frame(sq, [(0, 0.9, L), (1, 0.9, L), (1, 0.8, L)]), frame(sq, [(1, 0.9, L), (1, 0.9, L)])] + _moving(sq, 5))
    # two live rows of ONE frame choose one instance: the earlier list position gives its colour, the other loses a ttl
    A, B, N = rect(sq, 3, 0, 7, 10), rect(sq, 3, 1, 7, 11), rect(sq, 3, 0, 7, 11)
    add("two_claim", sq, 7, 3, [frame(sq, [(2, 0.9, A), (2, 0.9, B)]), frame(sq, [(2, 0.9, N)]), frame(sq, [(2, 0.9, B), (2, 0.9, A)])] + _moving(sq, 5))
    # unseen for ttl - 1 frames, matched in the last one it can be; the other comes one frame too late
    for ttl, hw in ((1, sq), (3, three), (8, two)):
        add(f"gone_ttl{ttl}", hw, 7, ttl, _gone(hw, ttl, ttl - 1)[:12])
    # an empty frame (masks without a pixel), a frame of n = 0
    add("empty_frames", two, 7, 3, _moving(two, 3) + [frame(two, [(2, 0.9, np.zeros(two, bool))] * 3), frame(two, [])] + _moving(two, 4)[2:] + [frame(two, [])] * 3)
    # entries below min_score (one exactly at it: kept) and empty masks between kept ones
    E = np.zeros(sq, bool)
    keep = lambda t: [(1, 0.9, rect(sq, 0, t, 9, t + 9)), (1, 0.49, rect(sq, 0, t, 9, t + 9)), (1, 0.9, E), (2, 0.5, rect(sq, 20, t, 29, t + 9)),
                      (2, 0.1, rect(sq, 20, t, 29, t + 9)), (1, 0.9, E), (1, 0.7, rect(sq, 40, t, 49, t + 9))]
    add("min_score_and_holes", sq, 7, 3, [frame(sq, keep(t)) for t in range(8)])
    # every live row of a class no new instance has: all tiles leave on the class test, every IoU is 0, every colour new
    add("class_free", sq, 7, 8, [frame(sq, [(t, 0.9, rect(sq, 5, 5 + k, 40, 30 + k)) for k in range(7)]) for t in range(9)])
    # the list driven to its cap: 100 instances x 8 frames that never match
    add("cap", big, 100, 8, _never(big, 10))
    add("pool3", sq, 7, 3, _random(sq, 7, 8, 3), pool=[(255, 0, 0), (0, 255, 0), (0, 0, 255)])
    add("random_ragged", two, 7, 3, _random(two, 7, 12, 1), min_score=0.3)
    add("random_single", three, 1, 8, _random(three, 1, 8, 5, classes=1), min_score=0.1)
    add("random_hundred", big, 100, 8, _random(big, 100, 8, 2, classes=4), min_score=0.2)
    return {c.name: c for c in out}


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = cases()[name]
    tracker = VD.InstanceColorTracker(case.ttl, case.pool)
    frames = []
    for classes, scores, masks in case.frames:
        n_before = len(tracker.live)
        colors = tracker.assign(classes, scores, masks, case.min_score, prefill(case.topk))
        frames.append({"colors": colors, "live": tracker.live_rows(), "iou": tracker.last_iou.copy(), "n_before": n_before})
    return frames


def expected(case):
    """per frame: colors uint8 [topk,3] (prefill(topk) with the instances recoloured), live rows after the frame, iou of the frame;
    computed once per case and shared - do not modify"""
    return _expected(case.name)
