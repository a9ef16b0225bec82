"""Crafted inputs of the instance-evaluation tests (tests/test_instance_eval_cpu.py, tests/test_gpu_instance_eval.py): the mask set of the
RLE tests, run lengths with zero-length runs, and pictures that pin one rule of COCOeval.evaluateImg each.  IoUs are kept away from the
thresholds by construction (the fractions are written beside each case), except the one case that sits exactly on 0.5."""
import numpy as np

from odise_amd import coco_rle as R

H, W = 96, 80          # the pictures of the matching cases


def blobs(h, w, seed):
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y, x = np.ogrid[:h, :w]
    for _ in range(5):
        cy, cx = g.integers(0, h), g.integers(0, w)
        ry, rx = g.integers(1, max(2, h // 3)), g.integers(1, max(2, w // 3))
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


def mask_set(h, w):
    """zeros, ones, one pixel in each corner, checkerboard, random blobs, a coarse noise mask (the set of tests/test_gpu_instance_rle.py)."""
    ms = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        ms.append(m)
    yy, xx = np.mgrid[:h, :w]
    ms.append(((yy + xx) % 2).astype(np.uint8))
    ms.append(blobs(h, w, h * 7 + w))
    ms.append((np.random.default_rng(h + w).random((h, w)) < 0.5).astype(np.uint8))
    return np.stack(ms)


def with_zero_runs(counts, seed=0):
    """The same mask with zero-length runs put in: a run c becomes c1, 0, c2 (c1 + c2 = c), at a few places and once at the very end."""
    g = np.random.default_rng(seed)
    out = []
    for c in (int(v) for v in counts):
        if g.random() < 0.3:
            c1 = int(g.integers(0, c + 1))
            out += [c1, 0, c - c1]
        else:
            out.append(c)
    return np.asarray(out + [0, 0], np.int64)


def rect(y0, y1, x0, x1, h=H, w=W):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def ann(mask, category=0, iscrowd=0, area=None, compressed=True):
    """An annotation dict with RLE ground truth (compressed string or uncompressed list)."""
    cnts = R.mask_counts(mask)
    seg = {"size": list(mask.shape), "counts": R.counts_to_string(cnts) if compressed else [int(c) for c in cnts]}
    return {"category_id": category, "iscrowd": iscrowd, "area": float(mask.sum() if area is None else area), "segmentation": seg}


def case(masks, scores, classes, anns, K=1):
    return {"masks": np.stack(masks).astype(np.uint8), "scores": np.asarray(scores, np.float32), "classes": np.asarray(classes, np.int32),
            "annotations": anns, "K": K}


def matching_cases():
    c = {}
    # one ground truth of 21 x 20 = 420; A (score .9) 17 x 16 = 272 inside it: 272 / 420 = .6476; B (score .8) 20 x 19 = 380: .9048
    c["two_on_one"] = case([rect(10, 27, 10, 26), rect(10, 30, 10, 29)], [.9, .8], [0, 0], [ann(rect(10, 31, 10, 30))])
    # a 10 x 20 detection over two ground truths of 10 x 14 that each share 10 x 12 with it: 120 / 220 = .5454 twice -> the later one;
    # the second detection covers the later one with 130 / 140 = .9286 and finds it taken at t = .5 only
    c["equal_iou"] = case([rect(10, 20, 10, 30), rect(10, 20, 18, 31)], [.9, .8], [0, 0], [ann(rect(10, 20, 8, 22)), ann(rect(10, 20, 18, 32))])
    # two detections inside a crowd region and nothing else: inter / area_d = 1 for both, matched and ignored, the crowd stays available
    c["crowd"] = case([rect(5, 15, 5, 15), rect(20, 30, 20, 30)], [.9, .8], [0, 0], [ann(rect(0, 40, 0, 40), iscrowd=1)])
    # the detection 20 x 20 lies in a crowd (iou 1) and over a regular 20 x 26 ground truth: 400 / 520 = .7692: the regular match is kept up
    # to t = .75, beyond it the crowd takes the detection
    c["break"] = case([rect(10, 30, 10, 30)], [.9], [0], [ann(rect(0, 50, 0, 50), iscrowd=1), ann(rect(10, 30, 10, 36))])
    # a 30 x 30 ground truth (small) matched exactly, and an unmatched 40 x 40 detection (medium)
    c["areas"] = case([rect(0, 30, 0, 30), rect(50, 90, 40, 80)], [.9, .8], [0, 0], [ann(rect(0, 30, 0, 30))])
    # exactly on 0.5: one pixel against two
    c["on_half"] = case([rect(5, 6, 5, 6)], [.9], [0], [ann(rect(5, 7, 5, 6))])
    return c


def random_case(seed=5, n=100, n_gt=40, K=5):
    """100 detections and 40 ground truths over 5 categories: crowds, all four area classes on the ground-truth side (the annotation's
    area is a number of its own), detections that are jittered ground truths or noise, scores on a grid of 0.05 (ties)."""
    g = np.random.default_rng(seed)

    def box(scale):
        hh, ww = int(g.integers(2, scale)), int(g.integers(2, scale))
        y, x = int(g.integers(0, H - hh)), int(g.integers(0, W - ww))
        return y, y + hh, x, x + ww

    boxes = [box(70 if i % 3 == 0 else 28) for i in range(n_gt)]
    anns = []
    for i, b in enumerate(boxes):
        m = rect(*b)
        area = [None, 500.0, 4000.0, 12000.0][i % 4] if i % 5 else None     # mostly a class of its own choosing, sometimes the mask's
        anns.append(ann(m, category=int(g.integers(0, K)), iscrowd=int(i % 7 == 3), area=area, compressed=bool(i % 2)))
    masks, classes = [], []
    for i in range(n):
        if i % 4 != 3 and n_gt:
            j = int(g.integers(0, n_gt))
            y0, y1, x0, x1 = boxes[j]
            dy0, dy1, dx0, dx1 = (int(v) for v in g.integers(-3, 4, 4))
            y0, x0 = max(0, y0 + dy0), max(0, x0 + dx0)
            masks.append(rect(y0, max(y0 + 1, min(H, y1 + dy1)), x0, max(x0 + 1, min(W, x1 + dx1))))
            classes.append(anns[j]["category_id"] if g.random() < 0.8 else int(g.integers(0, K)))
        else:
            masks.append(rect(*box(50)) & (g.random((H, W)) < 0.9))
            classes.append(int(g.integers(0, K)))
    scores = np.round(g.random(n) * 20) / 20
    return case(masks, scores, classes, anns, K)


def bits(word, a):
    """The ten threshold bits of area range a of a matched / ignored word, as a list of 0 / 1."""
    return [int((int(word) >> (10 * a + t)) & 1) for t in range(10)]
