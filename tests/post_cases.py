"""Crafted inputs of the post-processing tests (tests/test_post_reference_cpu.py asserts their margins from the float64 reference alone,
tests/test_gpu_postprocess.py runs them on the device).  A case is a dict: Q, K, h4, w4, img (h, w), out (h, w), logits [Q, h4, w4] fp32
(fp16-representable), mask_cls [Q, K+1] fp32, thing (set of class ids), object_mask_threshold, overlap_threshold.

Exact geometries (output = image, padded size = 4 x logits): the logits are multiples of 1/8 in [-6, 6] and the x4 taps multiples of 1/8, so
every interpolated value is a multiple of 1/512, exact in fp32 and float64 alike.
"""
import functools

import numpy as np

import post_reference as R

# name -> (h4, w4, image (h, w), output (h, w)).  A tile of the tiled pixel pass is 256 pixels of one output row.
GEOMETRIES = {
    "x4_w256": (8, 64, (32, 256), (32, 256)),      # ow % 32 == 0, one full tile per row
    "x4_w288": (8, 72, (32, 288), (32, 288)),      # ow % 32 == 0, one full and one partial tile
    "x4_ragged": (8, 72, (30, 285), (30, 285)),    # image smaller than the pad, ow % 4 != 0
    "x4_w276": (8, 72, (32, 276), (32, 276)),      # ow % 4 == 0, ow % 32 != 0
    "up": (8, 16, (30, 61), (45, 100)),            # generic: up-scaling, non-square
    "down": (8, 16, (30, 61), (17, 40)),           # generic: down-scaling
}
EXACT = ("x4_w256", "x4_w288", "x4_ragged", "x4_w276")


def things_of(K):
    return set(range(0, K, 2))                     # even classes are things


def exact_logits(rng, Q, h4, w4, lo=-6.0, hi=6.0):
    """Blobby multiples of 1/8 in [lo, hi]: a per-query sign pattern of cell blocks times a random magnitude per cell."""
    sign = np.where(rng.random((Q, (h4 + 1) // 2, (w4 + 3) // 4)) < min(0.35, 2.0 / Q), 1.0, -1.0).repeat(2, 1).repeat(4, 2)[:, :h4, :w4]
    mag = rng.integers(1, int(hi * 8) + 1, (Q, h4, w4)) / 8.0
    return np.clip(sign * mag, lo, hi).astype(np.float32)


def generic_logits(rng, Q, h4, w4):
    sign = np.where(rng.random((Q, (h4 + 1) // 2, (w4 + 3) // 4)) < min(0.35, 2.0 / Q), 1.0, -1.0).repeat(2, 1).repeat(4, 2)[:, :h4, :w4]
    return (sign * rng.uniform(0.5, 6.0, (Q, h4, w4))).astype(np.float16).astype(np.float32)


def label_cls(rng, Q, K, null_share=0.15, peak=(1.5, 5.0)):
    """mask_cls rows with one raised class each (the null class for some) over uniform noise: distinct real-valued scores per query."""
    z = rng.uniform(-1.0, 1.0, (Q, K + 1))
    lab = rng.integers(0, K, Q)
    lab[rng.random(Q) < null_share] = K
    z[np.arange(Q), lab] = np.log(K + 1.0) + rng.uniform(*peak, Q)
    return z.astype(np.float32)


def make(name, Q, K, geom, seed, dup=True, **kw):
    h4, w4, img, out = GEOMETRIES[geom]
    rng = np.random.default_rng(seed)
    logits = exact_logits(rng, Q, h4, w4) if geom in EXACT else generic_logits(rng, Q, h4, w4)
    cls = label_cls(rng, Q, K)
    cls[0, K] = -4.0                                                       # query 0 (and its duplicate) is never null and has the highest score
    cls[0, min(K - 1, 3)] = np.log(K + 1.0) + 8.0
    if K >= 8:
        lead = np.arange(1, Q, 10)                                         # every tenth query raises class 2, so that the twin columns lead the arg-max somewhere
        cls[lead, :K] = np.minimum(cls[lead, :K], 1.0)
        cls[lead, 2], cls[lead, K] = np.log(K + 1.0) + 3.0 + 0.01 * lead, -4.0
        corner = (slice(None), slice(0, h4 // 2), slice(0, w4 // 8))           # ... and does in a corner that query 1 holds alone
        logits[corner] = -np.abs(logits[corner])
        logits[1, :h4 // 2, :w4 // 8] *= -1.0
        cls[:, 5] = cls[:, 2]                                              # a duplicated class column: the semantic arg-max takes the first
    if dup and Q >= 4:                                                     # an exact tie: query Q-2 repeats query 0 (same logits, same mask_cls row)
        logits[Q - 2], cls[Q - 2] = logits[0], cls[0]
    c = {"name": name, "Q": Q, "K": K, "geom": geom, "h4": h4, "w4": w4, "img": img, "out": out, "logits": logits, "mask_cls": cls,
         "thing": things_of(K), "object_mask_threshold": 0.0, "overlap_threshold": 0.5, "dup": (0, Q - 2) if dup and Q >= 4 else None, "twin": (2, 5) if K >= 8 else None}
    c.update(kw)                                                           # (0.5: of up to 300 overlapping random masks few keep 80 % of their area)
    return c


@functools.lru_cache(maxsize=None)
def sweep():
    """Every (Q, K, geometry) the issue names, at the smallest shapes: name -> case."""
    rows = [("q7_k3", 7, 3, "x4_w256"), ("q20_k133", 20, 133, "x4_w288"), ("q100_k133_ragged", 100, 133, "x4_ragged"),
            ("q100_k133", 100, 133, "x4_w288"), ("q101_k133", 101, 133, "x4_w288"), ("q104_k164", 104, 164, "x4_w288"),
            ("q100_k164_w276", 100, 164, "x4_w276"), ("q150_k847", 150, 847, "x4_w276"), ("q300_k1203", 300, 1203, "x4_w256"),
            ("q20_k133_up", 20, 133, "up"), ("q100_k164_down", 100, 164, "down"), ("q7_k3_up", 7, 3, "up")]
    return {n: make(n, q, k, g, 1000 + i) for i, (n, q, k, g) in enumerate(rows)}


@functools.lru_cache(maxsize=None)
def reference(name, topk=100, panoptic_on=True):
    c = all_cases()[name]
    pad = (4 * c["h4"], 4 * c["w4"])
    return R.postprocess(c["mask_cls"], c["logits"], pad, c["img"], c["out"], c["K"], c["thing"], c["object_mask_threshold"], c["overlap_threshold"],
                         topk, panoptic_on)


# ---- crafted decision cases (Q small, 32 x 64 pixels) ---------------------------------------------------------------------------------
def _regions(Q, h4, w4, boxes, rng, inside=(2.0, 6.0)):
    """logits: query q positive inside boxes[q] = (y0, y1, x0, x1) (cells), negative outside; random multiples of 1/8 so that the blended
    border pixels of different rows differ."""
    lg = -rng.integers(int(inside[0] * 8), int(inside[1] * 8) + 1, (Q, h4, w4)) / 8.0
    for q, b in enumerate(boxes):
        if b is not None:
            y0, y1, x0, x1 = b
            lg[q, y0:y1, x0:x1] *= -1.0
    return lg.astype(np.float32)


def _cls_rows(K, labels, scores):
    """mask_cls whose softmax has probability scores[q] at labels[q] and the rest spread evenly."""
    z = np.zeros((len(labels), K + 1))
    for q, (l, s) in enumerate(zip(labels, scores)):
        z[q, l] = np.log(s / (1.0 - s) * K)
    return z.astype(np.float32)


def _small(name, K, boxes, labels, scores, thing, seed=7, h4=8, w4=16, **kw):
    rng = np.random.default_rng(seed)
    Q = len(labels)
    c = {"name": name, "Q": Q, "K": K, "geom": "x4_small", "h4": h4, "w4": w4, "img": (4 * h4, 4 * w4), "out": (4 * h4, 4 * w4),
         "logits": _regions(Q, h4, w4, boxes, rng), "mask_cls": _cls_rows(K, labels, scores), "thing": set(thing), "object_mask_threshold": 0.0,
         "overlap_threshold": 0.8, "dup": None}
    c.update(kw)
    return c


def _columns(n, h4=8, w4=16):
    """n disjoint boxes side by side."""
    step = w4 // n
    return [(0, h4, i * step, (i + 1) * step) for i in range(n)]


def _overlap_pair(target_delta):
    """Query 0 (thing, score .7) owns a box; query 1 (higher score) covers part of it.  Query 1's score is tuned by bisection on the float64
    reference until query 0's mask_area / original_area is exactly 4/5 (target_delta = 0) or one pixel short of it (-1)."""
    K = 3
    for seed in range(200):
        rng = np.random.default_rng(500 + seed)
        boxes = [(0, 8, 2, 12), (0, 8, 8, 16), None, None]
        lg = _regions(4, 8, 16, boxes, rng)
        lg[0, :, 8:12] = rng.integers(1, 17, (8, 4)) / 8.0                 # both weak where they overlap: the owner depends on the scores
        lg[1, :, 8:12] = rng.integers(1, 17, (8, 4)) / 8.0
        mask = R.upsample(lg, (32, 64), (32, 64), (32, 64))
        orig = int((R.sigmoid(mask[0]) >= 0.5).sum())
        if orig % 5:
            continue
        want = orig * 4 // 5 + target_delta
        lo, hi = 0.05, 0.999
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            cls = _cls_rows(K, [0, 2, K, K], [0.7, mid, 0.9, 0.9])
            area = int(R.panoptic(cls, mask, K, {0, 2}, 0.0, 0.8)["counts"][0, 0])
            if area == want:
                return {"name": f"overlap_{'equal' if target_delta == 0 else 'below'}", "Q": 4, "K": K, "geom": "x4_small", "h4": 8, "w4": 16,
                        "img": (32, 64), "out": (32, 64), "logits": lg, "mask_cls": cls, "thing": {0, 2}, "object_mask_threshold": 0.0,
                        "overlap_threshold": 0.8, "dup": None, "expect_ratio": (want, orig)}
            if area > want:
                lo = mid                                                   # query 1 must win more pixels: raise its score
            else:
                hi = mid
    raise AssertionError("no overlap case found")


@functools.lru_cache(maxsize=None)
def decisions():
    K = 6
    thing = {0, 2, 4}
    col4 = _columns(4)
    cases = [
        _small("all_null", K, col4, [K] * 4, [0.9, 0.8, 0.7, 0.6], thing),
        _small("all_below_threshold", K, col4, [0, 1, 2, 3], [0.5, 0.45, 0.4, 0.35], thing, object_mask_threshold=0.6),
        # two score levels 1e-3 apart with the threshold between them: queries 0 and 2 stay
        _small("threshold_between", K, col4, [0, 1, 2, 3], [0.601, 0.600, 0.601, 0.600], thing, object_mask_threshold=0.6005),
        # query 1 is kept but query 0 (same box, higher score, stronger logits everywhere is not guaranteed: same logits) takes every pixel
        _small("kept_loses_all", K, [col4[0], col4[0], col4[2], col4[3]], [0, 2, 4, 1], [0.9, 0.5, 0.8, 0.7], thing),
        # stuff classes 1 and 3, thing classes 0, 2, 4: two stuff queries of class 1 -> one row; two thing queries of class 2 -> two rows
        _small("stuff_merges_things_do_not", K, _columns(8)[:6], [1, 2, 1, 2, 3, 0], [0.9, 0.85, 0.8, 0.75, 0.7, 0.65], thing),
        _overlap_pair(0), _overlap_pair(-1),
    ]
    c = cases[3]
    c["logits"][1] = c["logits"][0]                                        # same mask, lower score: loses every pixel
    # exactly 100 surviving segments at Q = 100, and 120 candidates at Q = 120 (more than the record holds)
    for Q in (100, 120):
        rng = np.random.default_rng(40 + Q)
        h4, w4 = 8, 64
        cells = [(y, x) for y in range(0, 8, 2) for x in range(0, 64, 2)][:Q]           # one 2 x 2 cell block (8 x 8 pixels) per query
        boxes = [(y, y + 2, x, x + 2) for y, x in cells]
        labels = [(2 * q) % 16 for q in range(Q)]                                      # things only: every query is a segment
        cc = {"name": f"segments_{Q}", "Q": Q, "K": 16, "geom": "x4_w256", "h4": h4, "w4": w4, "img": (32, 256), "out": (32, 256),
              "logits": _regions(Q, h4, w4, boxes, rng, inside=(4.0, 6.0)), "mask_cls": _cls_rows(16, labels, 0.8 + 0.1 * rng.random(Q)),
              "thing": set(range(0, 16, 2)) - ({14} if Q == 120 else set()), "object_mask_threshold": 0.0, "overlap_threshold": 0.8, "dup": None}
        cases.append(cc)
    return {c["name"]: c for c in cases}


# ---- instance head -----------------------------------------------------------------------------------------------------------------
def level_cls(Q, K, seed, copies=()):
    """mask_cls whose Q*K class probabilities are distinct levels 2e-3 apart (relative), in a random arrangement; the null column evens
    out the row sums, so the softmax leaves the levels as they are.  copies: (src, dst) rows made identical afterwards (exact ties)."""
    rng = np.random.default_rng(seed)
    first = sorted({s for s, _ in copies})                                 # the copied rows hold the highest levels: the tie blocks lead the order
    rank = np.empty((Q, K), np.int64)
    rest = [q for q in range(Q) if q not in first]
    rank[first] = rng.permutation(len(first) * K).reshape(len(first), K)
    rank[rest] = len(first) * K + rng.permutation(len(rest) * K).reshape(len(rest), K)
    z = -2e-3 * rank.astype(np.float64)
    total = np.exp(z).sum(1).max() * 1.25
    z = np.concatenate([z, np.log(total - np.exp(z).sum(1))[:, None]], 1).astype(np.float32)
    for src, dst in copies:
        z[dst] = z[src]
    return z


def dense_cls(Q, K, seed, topk=100):
    """Random class logits; the first seed from `seed` on whose float64 probabilities leave the selection to an fp32 softmax: at most 2 of
    the Q*K entries within (K + 8) 2^-23 (relative) of the k-th, and neighbours among the first topk + 10 more than twice that apart."""
    band = (K + 8) * 2.0 ** -23
    for s in range(seed, seed + 1000):
        z = (2.0 * np.random.default_rng(s).standard_normal((Q, K + 1))).astype(np.float32)
        p = np.sort(R.softmax(z)[:, :K].reshape(-1))[::-1]
        top = p[:topk + 10]
        if ((top[:-1] - top[1:]) / top[:-1]).min() > 2 * band and (np.abs(p - p[topk - 1]) <= band * p[topk - 1]).sum() <= 2:
            return z
    raise AssertionError("no dense case found")


@functools.lru_cache(maxsize=None)
def instances():
    """name -> case; the instance tests run each at several topk."""
    out = {}
    triples = [(s, s + 6) for s in range(6)] + [(s, s + 12) for s in range(6)]             # rows 0..5 three times: tie blocks of three
    for name, Q, K, geom, cls in [
            ("levels_q20_k133", 20, 133, "x4_w288", level_cls(20, 133, 3, triples)),
            ("levels_q7_k3", 7, 3, "x4_w256", level_cls(7, 3, 4, [(1, 5)])),
            ("levels_q128_k128", 128, 128, "x4_w256", level_cls(128, 128, 5, [(3, 77), (3, 120)])),    # Q*K = 16384: the last register-path size
            ("levels_q128_k129", 128, 129, "x4_w256", level_cls(128, 129, 6, [(3, 77), (3, 120)])),    # 16512: the global-memory path
            ("dense_q128_k128", 128, 128, "x4_w256", dense_cls(128, 128, 8000)),
            ("dense_q128_k129", 128, 129, "x4_w256", dense_cls(128, 129, 9000))]:
        c = make(name, Q, K, geom, 2000 + len(out), dup=False)
        c["mask_cls"] = cls
        out[name] = c
    return out


@functools.lru_cache(maxsize=None)
def entry_case():
    """The per-image entry points' case: logits in [-2, 2], where no sigmoid comes near an fp16 rounding boundary (inst_stats exact)."""
    c = make("entry_q20_k133", 20, 133, "x4_w288", 3000)
    rng = np.random.default_rng(3001)
    c["logits"] = exact_logits(rng, 20, 8, 72, -2.0, 2.0)
    c["logits"][18] = c["logits"][0]
    return c


@functools.lru_cache(maxsize=None)
def rotation():
    """Six distinct images of mixed sizes for one call (more than the four (S, ids) sets): same Q / K / logits resolution."""
    sizes = [((32, 288), (32, 288)), ((30, 285), (30, 285)), ((32, 276), (32, 276)), ((30, 285), (40, 300)), ((32, 288), (32, 288)),
             ((17, 100), (17, 100))]
    out = []
    for i, (img, o) in enumerate(sizes):
        c = make(f"rot{i}", 20, 133, "x4_w288", 4000 + i)
        c["img"], c["out"] = img, o
        out.append(c)
    return out


def all_cases():
    d = dict(sweep())
    d.update(decisions())
    d.update(instances())
    d[entry_case()["name"]] = entry_case()
    return d
