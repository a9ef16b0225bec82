"""Box sequences for the box colour tracker (odise_amd/video.py BoxColorTracker, csrc/box_track.hip) and what the restatement makes of
them.

A frame is (classes int32 [n], scores float32 [n], boxes float32 [n,4] XYXY) with n <= topk; a case adds topk, ttl, min_score and the
pool.  `expected(case)` runs BoxColorTracker over it once and keeps, per frame: the colours (of the pre-filled rows), the live rows after
the frame and the IoU matrix of the frame.  `device_frame` lays a frame out as the library takes it: [topk,4] boxes whose rows past n are
a valid box with a passing score and a class that would match (the count alone must keep them out), the table n | query index | class.

There are no pixels, so the sizes that matter are topk 1 / 7 / 100 and ttl 1 / 3 / 8; the crafted cases sit on the rule's edges: an IoU of
exactly 3/5 (no match: the threshold is strict) and 7/11, a class mismatch, two live rows choosing one box, two equal maxima in one row,
a row matched in the last frame its ttl allows and one a frame too late, the list at its cap of 800, boxes without area and with
non-finite members, fractional boxes, frames of n = 0.
"""
import functools

import numpy as np

from odise_amd import video as VD

NAN, INF = float("nan"), float("inf")


def frame(items):
    """items: (class, score, (x0, y0, x1, y1)) -> (classes, scores, boxes)"""
    return (np.array([c for c, _, _ in items], np.int32), np.array([s for _, s, _ in items], np.float32),
            np.array([b for _, _, b in items], np.float32).reshape(-1, 4))


class Case:
    def __init__(self, name, topk, ttl, frames, min_score=0.5, pool=None):
        self.name, self.topk, self.ttl, self.frames, self.min_score = name, topk, ttl, frames, float(min_score)
        self.pool = VD.default_pool() if pool is None else np.asarray(pool, np.uint8).reshape(-1, 3)
        for classes, scores, boxes in frames:
            assert boxes.shape == (len(classes), 4) and boxes.dtype == np.float32 and len(classes) == len(scores) <= topk


def prefill(n):
    """What the caller put into `colors` before the call: a distinct triple per row."""
    r = np.arange(n)
    return np.stack([200 + r % 50, r, 255 - r], axis=1).astype(np.uint8)


def device_frame(case, t):
    """-> (boxes float32 [topk,4], table int32 [1 + 2 topk], scores float32 [topk])"""
    classes, scores, boxes = case.frames[t]
    n, topk = len(boxes), case.topk
    full = np.tile(np.array([0, 0, 50, 50], np.float32), (topk, 1))
    full[:n] = boxes
    table = np.zeros(1 + 2 * topk, np.int32)
    table[0] = n
    table[1:1 + topk] = np.arange(topk)[::-1]
    table[1 + topk:1 + topk + n] = classes
    table[1 + topk + n:] = classes[0] if n else 0
    sc = np.ones(topk, np.float32)
    sc[:n] = scores
    return full, table, sc


def _moving(T, step=1, cls=2, wh=(12, 8), y0=3):
    return [frame([(cls, 0.9, (2 + step * t, y0, 2 + step * t + wh[0], y0 + wh[1]))]) for t in range(T)]


def _gone(gap):
    """A and B in frame 0; `gap` frames of something else; A again (the last frame its ttl allows when gap = ttl - 1); B a frame later."""
    A, B, far = (0, 0, 10, 10), (30, 30, 44, 41), (100, 100, 103, 102)
    between = [frame([]) if k % 2 == 0 else frame([(5, 0.9, far)]) for k in range(gap)]
    return [frame([(1, 0.9, A), (1, 0.8, B)])] + between + [frame([(1, 0.9, A)]), frame([(1, 0.9, B)])] + _moving(3, 1, 3)


def _never(T, n=100):
    """n boxes whose classes turn with the frame (period 9 > 8 retained frames): nothing ever matches."""
    return [frame([((k + t) % 9, 0.9, (k, 2 * k, k + 20, 2 * k + 9)) for k in range(n)]) for t in range(T)]


def _random(topk, T, seed, classes=3, frac=False):
    rng = np.random.default_rng(seed)
    k0 = max(1, topk * 3 // 4)
    state = [[float(rng.integers(0, 60)), float(rng.integers(0, 60)), float(rng.integers(1, 30)), float(rng.integers(1, 30)), int(rng.integers(0, classes))]
             for _ in range(k0)]
    out = []
    for _ in range(T):
        items = []
        for b in state:
            b[0] += float(rng.integers(-2, 3)) * (0.37 if frac else 1.0)
            b[1] += float(rng.integers(-2, 3)) * (0.61 if frac else 1.0)
            if rng.random() < 0.8:
                cls = b[4] if rng.random() < 0.9 else (b[4] + 1) % classes
                w = b[2] if rng.random() < 0.95 else 0.0                       # now and then a box without width
                items.append((cls, float(rng.random()), (b[0], b[1], b[0] + w, b[1] + b[3])))
        order = rng.permutation(len(items))
        out.append(frame([items[k] for k in order][:topk]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    unit = (0, 0, 1, 1)
    add("one_box", 1, 1, [frame([(0, 0.9, unit)]), frame([(0, 0.9, unit)]), frame([(0, 0.9, (0, 0, 0, 1))]), frame([(0, 0.9, unit)]),
                          frame([(1, 0.9, unit)]), frame([(1, 0.2, unit)]), frame([]), frame([(1, 0.5, unit)])])
    add("moving", 7, 3, _moving(9))
    # IoU exactly 3/5 (4 x 1 boxes one apart: 3 of 5 columns in common) is no match, 7/11 (9 x 1, two apart) is
    add("iou_threshold", 7, 3, [frame([(1, 0.9, (0, 0, 4, 1))]), frame([(1, 0.9, (1, 0, 5, 1))]), frame([(1, 0.9, (1, 0, 5, 1))]),
                                frame([(1, 0.9, (0, 5, 9, 6))]), frame([(1, 0.9, (2, 5, 11, 6))]), frame([(1, 0.9, (2, 5, 11, 6)), (1, 0.9, (0, 0, 4, 1))])])
    # equal boxes under different classes: IoU 0 between them
    M = (4, 60, 30, 69)
    add("class_mismatch", 7, 3, [frame([(1, 0.9, M)]), frame([(0, 0.9, M), (1, 0.9, M)]), frame([(1, 0.9, M), (0, 0.9, M), (2, 0.9, M)])] + [frame([(2, 0.9, M)])] * 3)
    # two equal maxima in a row: the first takes the colour, the second a new one
    L = (10, 10, 13, 14)
    add("tie", 7, 3, [frame([(1, 0.9, L)]), frame([(0, 0.9, L), (1, 0.9, L), (1, 0.8, L)]), frame([(1, 0.9, L), (1, 0.9, L)])] + _moving(3))
    # two live rows of ONE frame choose one box: the earlier list position gives its colour, the other loses a ttl
    A, B, N = (0, 3, 20, 13), (1, 3, 21, 13), (0, 3, 21, 13)
    add("two_claim", 7, 3, [frame([(2, 0.9, A), (2, 0.9, B)]), frame([(2, 0.9, N)]), frame([(2, 0.9, B), (2, 0.9, A)])] + _moving(3))
    for ttl in (1, 3, 8):
        add(f"gone_ttl{ttl}", 7, ttl, _gone(ttl - 1))
    # boxes without area, turned round, with NaN and infinite members, below the score (one exactly at it: kept), between kept ones
    bad = lambda t: [(1, 0.9, (t, 0, t + 9, 9)), (1, 0.49, (t, 0, t + 9, 9)), (1, 0.9, (5, 5, 5, 9)), (2, 0.5, (t, 20, t + 9, 29)), (1, 0.9, (5, 9, 9, 5)),
                     (1, 0.9, (NAN, 0, t + 9, 9)), (1, 0.7, (t, 40, INF, 49))]
    add("bad_boxes", 7, 3, [frame(bad(t)) for t in range(6)] + [frame([(1, 0.9, (0, 0, NAN, NAN))] * 2), frame([])])
    add("empty_frames", 7, 3, _moving(3) + [frame([(2, 0.9, (0, 0, 0, 0))] * 3), frame([])] + _moving(5)[3:] + [frame([])] * 2)
    # fractional members (the area of a row is the truncated product; 0.5 x 0.5 is an instance of area 0) and a huge box
    add("fractional", 7, 3, [frame([(1, 0.9, (0.25, 0.25, 0.75, 0.75)), (1, 0.9, (10.5, 3.25, 30.125, 9.75)), (2, 0.9, (-1e6, -1e6, 1e6, 1e6))]),
                             frame([(1, 0.9, (0.25, 0.25, 0.75, 0.8125)), (1, 0.9, (11.5, 3.25, 31.125, 9.75)), (2, 0.9, (-1e6, -1e6, 1e6, 1e6 + 64))]),
                             frame([(2, 0.9, (-3e5, -3e5, 3e5, 3e5))])])
    add("cap", 100, 8, _never(10))
    add("pool3", 7, 3, _random(7, 8, 3), pool=[(255, 0, 0), (0, 255, 0), (0, 0, 255)])
    add("random_single", 1, 8, _random(1, 8, 5, classes=1), min_score=0.1)
    add("random_hundred", 100, 8, _random(100, 8, 2, classes=4), min_score=0.2)
    add("random_fractional", 7, 3, _random(7, 10, 9, frac=True), min_score=0.3)
    return {c.name: c for c in out}


def random_sequences(count=300):
    """Seeded random sequences for the CPU pin: (topk, ttl, frames)"""
    for seed in range(count):
        topk, ttl = (1, 7, 100)[seed % 3] if seed % 10 else 100, (1, 3, 8)[(seed // 3) % 3]
        yield min(topk, 12), ttl, _random(min(topk, 12), 6, 1000 + seed, frac=bool(seed % 2))


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = cases()[name]
    tracker = VD.BoxColorTracker(case.ttl, case.pool)
    frames = []
    for classes, scores, boxes in case.frames:
        n_before = len(tracker.live)
        colors = tracker.assign(classes, scores, boxes, case.min_score, prefill(case.topk))
        frames.append({"colors": colors, "live": tracker.live_rows(), "iou": tracker.last_iou.copy(), "n_before": n_before})
    return frames


def expected(case):
    """per frame: colors uint8 [topk,3] (prefill(topk) with the instances recoloured), live rows after the frame, iou of the frame;
    computed once per case and shared - do not modify"""
    return _expected(case.name)
