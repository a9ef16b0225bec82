"""Pictures for the PQ-for-semantic-segmentation tests (tests/test_semseg_pq_cpu.py, tests/test_gpu_semseg_pq.py; odise_amd/semseg_pq.py,
csrc/sem_pq.hip): crafted edges of the matching rule - an IoU of exactly one half and just above it, a predicted class with exactly
half and with more than half of its pixels on VOID, a class on one side only, an all-VOID ground truth, two ignore labels - seeded
smooth-and-noisy maps at the sizes and class counts where the device takes another path, and seeded random maps.  A case holds the
prediction and the RAW ground truth (classes and `ignore_label`); the expected statistics come from the literal host restatement and are
computed once per case."""
import numpy as np

from odise_amd import semseg_pq as SP
from semseg_cases import blobs


class Case:
    def __init__(self, name, K, pred, gt, ignore_label=255):
        self.name, self.K, self.ignore_label = name, int(K), int(ignore_label)
        self.pred, self.gt_raw = np.ascontiguousarray(pred, np.int32), np.ascontiguousarray(gt, np.int64)
        assert self.pred.ndim == 2 and self.pred.shape == self.gt_raw.shape
        self.hw = self.pred.shape
        self._literal = None

    def gt(self):
        """The ground truth as the device takes it: int32, the ignore label mapped to K."""
        return SP.map_ignore(self.gt_raw, self.K, self.ignore_label)

    def literal(self):
        """(PQStats, flags) of this picture alone, from the literal restatement."""
        if self._literal is None:
            self._literal = SP.image_stats_literal(self.pred, self.gt_raw, self.K, self.ignore_label)
        return self._literal


def _row(*runs):
    """A 1 x n map from (value, length) runs."""
    return np.concatenate([np.full(n, v, np.int64) for v, n in runs])[None, :]


def _edges():
    V = 255
    cases = [
        # class 1: pred = pixels 0-2, gt = pixels 1-3, inter 2, union 4: iou exactly 0.5 -> no tp, one fn, one fp.  class 0: 8 / 10: tp
        Case("iou_exactly_half", 2, _row((1, 3), (0, 9)), _row((0, 1), (1, 3), (0, 8))),
        # class 1: pred = pixels 0-75, gt = pixels 25-100, inter 51, union 101: iou 51 / 101 -> tp
        Case("iou_just_above_half", 2, _row((1, 76), (0, 44)), _row((0, 25), (1, 76), (0, 19))),
        # class 2 is predicted on two pixels, one on VOID, one on class 0: the VOID share is exactly 0.5 -> fp is counted
        Case("void_share_exactly_half", 3, _row((2, 2), (0, 6)), _row((V, 1), (0, 7))),
        # class 2 on three pixels, two on VOID -> skipped: neither fp nor anything else
        Case("void_share_above_half", 3, _row((2, 3), (0, 6)), _row((V, 2), (0, 7))),
        # class 1 in the ground truth only: fn.  class 2 in the prediction only: fp
        Case("class_only_in_gt", 3, _row((0, 8)), _row((0, 5), (1, 3))),
        Case("class_only_in_pred", 3, _row((0, 5), (2, 3)), _row((0, 8))),
        # VOID takes pixels out of the union: class 0 pred 6, gt 3, inter 3, VOID 2 -> union 4, iou 0.75
        Case("void_leaves_the_union", 2, _row((0, 6), (1, 2)), _row((0, 3), (1, 1), (V, 2), (1, 2))),
        Case("gt_all_void", 4, _row((0, 3), (3, 2)), _row((V, 5))),
        Case("one_pixel_right", 1, [[0]], [[0]]),
        Case("one_pixel_void", 1, [[0]], [[V]]),
        # 255 is the ignore label and 253 the last class; 65535 as the ignore label leaves 255 a class
        Case("ignore255_K254", 254, _row((253, 4), (0, 4), (7, 2)), _row((253, 3), (V, 2), (0, 3), (V, 2))),
        Case("ignore65535_K300", 300, _row((255, 4), (299, 4), (7, 2)), _row((255, 3), (65535, 2), (299, 3), (65535, 2)), ignore_label=65535),
    ]
    return cases


def picture(name, h, w, K, seed, void_share=0.1, ignore_label=255, noise=0.15, agree=0.7):
    """Seeded map: smooth blobs with `noise` of the pixels redrawn over all of [0, K); the ground truth agrees with it on `agree` of
    the pixels, is redrawn elsewhere, and is VOID on `void_share`.  With more than two pixels the last two are (K - 1, K - 1) and
    (K - 1, VOID): the last cell of the inter and of the void_pred vector."""
    rng = np.random.default_rng(seed)
    pred = blobs(h, w, K, seed).astype(np.int64)
    redraw = rng.random((h, w)) < noise
    pred[redraw] = rng.integers(0, K, int(redraw.sum()))
    gt = np.where(rng.random((h, w)) < agree, pred, rng.integers(0, K, (h, w)))
    gt[rng.random((h, w)) < void_share] = ignore_label
    if h * w > 2:
        pred.reshape(-1)[-2:] = K - 1
        gt.reshape(-1)[-2:] = (K - 1, ignore_label)
    if ignore_label < K:                                   # never the case for the datasets; keep the precondition
        pred[pred == ignore_label] = 0
    return Case(name, K, pred, gt, ignore_label)


# the sizes and class counts of the device tests: one pixel, odd sizes, exactly 16 rows of 256 pixels, more than one block; K = 3072 is
# the last count whose 4 K cells fit the LDS histogram, 3073 the first that is counted in global memory, 12288 the cap
SIZES = ((1, 1), (37, 53), (64, 64), (130, 257))


def _shapes():
    cases, seed = [], 300
    for h, w in SIZES:
        for K in (1, 2, 150):
            cases.append(picture(f"blobs_{h}x{w}_K{K}", h, w, K, seed, ignore_label=255))
            seed += 1
    for K in (3072, 3073, 12288):
        cases.append(picture(f"blobs_64x64_K{K}", 64, 64, K, seed, ignore_label=65535, noise=0.5))
        seed += 1
    return cases


EDGES = {c.name: c for c in _edges()}
SHAPES = {c.name: c for c in _shapes()}
CASES = {**EDGES, **SHAPES}


def random_case(seed):
    """1x1 to 40x60, K from 1 to 300, a VOID share from 0 to 1 (every fifth case: exactly 0 or exactly 1)."""
    rng = np.random.default_rng(1000 + seed)
    h, w, K = int(rng.integers(1, 41)), int(rng.integers(1, 61)), int(rng.integers(1, 301))
    K = {1: 1, 2: 300}.get(seed % 50, K)                                              # the ends of every range are met on purpose
    h, w = {3: (1, 1), 4: (40, 60)}.get(seed % 50, (h, w))
    share = (0.0, 1.0)[seed // 5 % 2] if seed % 5 == 0 else float(rng.random())
    ignore = 65535 if K > 255 else 255
    return picture(f"random{seed}", h, w, K, 2000 + seed, void_share=share, ignore_label=ignore, noise=float(rng.random()) * 0.5,
                   agree=float(rng.random()))


def stream_cases():
    """Six pictures of different sizes with the classes of one vocabulary (K = 150): most classes match in several pictures, so the iou
    sums depend on the order of the pictures."""
    sizes = ((37, 53), (64, 64), (1, 200), (130, 257), (90, 31), (8, 8))
    out = []
    for i, (h, w) in enumerate(sizes):
        rng = np.random.default_rng(500 + i)
        pred = (blobs(h, w, 6, 500 + i) * 3 + 2).astype(np.int64)                    # classes 2, 5, .., 17 in every picture
        gt = np.where(rng.random((h, w)) < 0.9, pred, rng.integers(0, 150, (h, w)))
        gt[rng.random((h, w)) < 0.05] = 255
        out.append(Case(f"stream{i}", 150, pred, gt))
    return out


def score_cases():
    """sem_seg float32 [K, 37, 53] with planted ties (three levels: most pixels tie between their best planes), K = 3 and 21."""
    rng = np.random.default_rng(77)
    return {K: rng.integers(0, 3, (K, 37, 53)).astype(np.float32) for K in (3, 21)}


def write_pictures(tmp_path, cases, names):
    """sem_seg_predictions.json rows (np.unique order per picture) and the ground truth as 8-bit PNGs (ignore label 255) under
    tmp_path; -> (json path, gt dir, the rows)."""
    import json

    from PIL import Image
    from odise_amd.semseg_eval import encode_json_sem_seg
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    rows = []
    for case, name in zip(cases, names):
        rows += encode_json_sem_seg(case.pred, f"some/dir/{name}.jpg")
        Image.fromarray(case.gt_raw.astype(np.uint8)).save(str(gt_dir / f"{name}.png"))
    path = tmp_path / "sem_seg_predictions.json"
    path.write_text(json.dumps(rows))
    return str(path), str(gt_dir), rows
