"""The label maps shared by tests/test_semseg_eval_cpu.py and tests/test_gpu_semseg_eval.py (odise_hip_semantic_eval / odise_amd/semseg_eval.py):
sizes around the 64-row word and the column (H in 1, 63, 64, 65, 129; W in 1, 3, 67), K in 1, 3, 150, 847, and the maps that stress the
per-class RLE - one class, stripes (horizontal ones change label at every row of every column), checkerboards (every pixel is a
transition), a class of a single pixel at the ends of the column-major order and on both sides of a word boundary, smooth blobs, more
classes than max_classes, labels outside [0, K), a label pointer that is only 4-byte aligned.  The expected values come from the literal
host restatement and are computed once per case."""
import numpy as np

from odise_amd import coco_rle
from odise_amd import semseg_eval as SE

HS, WS, KS = (1, 63, 64, 65, 129), (1, 3, 67), (1, 3, 150, 847)


def blobs(h, w, K, seed):
    """Seeded smooth map: the arg-max of min(K, 6) box-filtered noise planes, spread over [0, K)."""
    rng = np.random.default_rng(seed)
    n = min(K, 6)
    x = rng.standard_normal((n, h + 8, w + 8))
    c = np.cumsum(np.cumsum(np.pad(x, ((0, 0), (1, 0), (1, 0))), axis=1), axis=2)
    box = c[:, 9:, 9:] - c[:, :-9, 9:] - c[:, 9:, :-9] + c[:, :-9, :-9]
    ids = np.sort(rng.choice(K, n, replace=False))
    return ids[box.argmax(0)].astype(np.int32)


class Case:
    def __init__(self, name, K, labels, max_classes=None, flag=0, offset=False):
        self.name, self.K, self.labels, self.max_classes, self.flag, self.offset = name, int(K), np.ascontiguousarray(labels, np.int32), max_classes, flag, offset
        self.hw = self.labels.shape
        self._cache = {}

    def valid(self):
        return (self.labels >= 0) & (self.labels < self.K)

    def expected(self):
        """(classes int32 [n] ascending, strings [n], area int64 [n]) of the labels in [0, K): np.unique, a mask per class, coco_rle.encode."""
        if "exp" not in self._cache:
            classes = np.unique(self.labels[self.valid()]).astype(np.int32)
            masks = [(self.labels == c) for c in classes]
            self._cache["exp"] = (classes, [coco_rle.encode(m.astype(np.uint8))["counts"] for m in masks], np.asarray([m.sum() for m in masks], np.int64))
        return self._cache["exp"]

    def gt(self):
        """Seeded ground truth in [0, K] with a few values outside (they count as K)."""
        if "gt" not in self._cache:
            rng = np.random.default_rng(len(self.name) + 7 * self.K)
            g = np.where(rng.random(self.hw) < 0.6, np.clip(self.labels, 0, self.K - 1), rng.integers(0, self.K + 1, self.hw)).astype(np.int32)
            g[rng.random(self.hw) < 0.05] = -1
            g[rng.random(self.hw) < 0.05] = self.K + 5
            self._cache["gt"] = g
        return self._cache["gt"]

    def conf(self):
        if "conf" not in self._cache:
            n, v = self.K + 1, self.valid()
            g = np.where((self.gt() < 0) | (self.gt() > self.K), self.K, self.gt()).astype(np.int64)
            self._cache["conf"] = np.bincount(n * self.labels[v].astype(np.int64) + g[v], minlength=n * n).reshape(n, n).astype(np.int64)
        return self._cache["conf"]


def _k(i, least=1):
    return [k for k in KS if k >= least][i % len([k for k in KS if k >= least])]


def _build():
    cases, i = [], 0
    for h in HS:
        for w in WS:
            yy, xx = np.mgrid[0:h, 0:w]
            m = i + i // 3                                                            # so that a width does not always meet the same K
            K = _k(m)
            cases.append(Case(f"one0_{h}x{w}_K{K}", K, np.zeros((h, w))))
            K = _k(m + 1)
            cases.append(Case(f"onelast_{h}x{w}_K{K}", K, np.full((h, w), K - 1)))
            K = _k(m + 2, 3)
            cases.append(Case(f"vstripes_{h}x{w}_K{K}", K, xx % 3 * (K // 3)))
            K = _k(m + 3, 3)
            cases.append(Case(f"hstripes_{h}x{w}_K{K}", K, (yy % 3) * (K - 1) // 2))
            K = _k(m, 3)
            cases.append(Case(f"checker2_{h}x{w}_K{K}", K, (yy + xx) % 2 * (K - 1)))
            K = _k(m + 1, 3)
            cases.append(Case(f"checker3_{h}x{w}_K{K}", K, (yy + 2 * xx) % 3 * ((K - 1) // 2)))
            K = _k(m + 2)
            cases.append(Case(f"blobs_{h}x{w}_K{K}", K, blobs(h, w, K, seed=i)))
            i += 1
    h, w = 129, 67
    for name, (y, x) in {"first": (0, 0), "last": (h - 1, w - 1), "row63": (63, 5), "row64": (64, 66)}.items():
        for K in (3, 847):
            m = np.zeros((h, w), np.int32)
            m[y, x] = K - 1
            cases.append(Case(f"single_{name}_K{K}", K, m))
    yy, xx = np.mgrid[0:65, 0:67]
    five = (xx // 14) * 30 + 7                                                       # classes 7, 37, 67, 97, 127
    cases.append(Case("five_of_max2_K150", 150, five, max_classes=2))
    for name, bad in (("minus1", -1), ("labelK", 150)):
        m = blobs(65, 67, 150, seed=90).copy()
        m[3:9, 60:67] = bad
        m[64, 0] = bad
        cases.append(Case(f"bad_{name}_K150", 150, m, flag=1))
    cases.append(Case("offset_pointer_65x67_K847", 847, blobs(65, 67, 847, seed=91), offset=True))
    return {c.name: c for c in cases}


CASES = _build()


def score_cases():
    """(name, sem_seg float32 [K,h,w]): K = 3 with exact ties between planes (first maximum wins), K = 150 random."""
    rng = np.random.default_rng(5)
    ties = rng.integers(0, 3, (3, 65, 67)).astype(np.float32)                         # three levels: most pixels tie between planes
    return {"ties_K3": ties, "random_K150": rng.standard_normal((150, 65, 67)).astype(np.float32)}


def argmax_first(sem):
    return np.asarray(sem).argmax(0).astype(np.int32)                                # numpy's argmax returns the first maximum


def host_rows(case, file_name="f", mapping=None):
    return SE.encode_json_sem_seg(case.labels, file_name, mapping)
