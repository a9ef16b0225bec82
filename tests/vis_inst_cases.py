"""Overlapping instance masks and semantic label maps for the drawing tests (tests/test_visualize_inst_cpu.py,
tests/test_gpu_visualize_inst.py): the smallest shapes at which the packed-word histograms (64 rows per word), the overlay's tiles
(64 x 64, 4 x 4 pixels per thread, 50 masks staged at a time) and the semantic record (per-block histogram, rank by counting, at most
MAX_SEGMENTS rows) can go wrong.  The references (odise_amd.visualize, the restatement) are computed once per case and shared."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS


@dataclass
class InstCase:
    name: str
    masks: np.ndarray                     # bool [topk,H,W]
    scores: Optional[np.ndarray] = None   # float32 [topk]
    min_score: float = 0.0
    n: Optional[int] = None               # the table's count (None: no table, every mask counts)
    note: str = ""
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def topk(self):
        return len(self.masks)

    @property
    def hw(self):
        return self.masks.shape[1:]

    def live(self) -> np.ndarray:
        return self.masks[:self.topk if self.n is None else self.n]

    def live_scores(self):
        return None if self.scores is None else self.scores[:len(self.live())]

    def table(self) -> Optional[np.ndarray]:
        if self.n is None:
            return None
        t = np.zeros(1 + 2 * self.topk, np.int32)
        t[0] = self.n
        t[1:1 + self.topk] = np.arange(self.topk)
        return t

    def image(self) -> np.ndarray:
        h, w = self.hw
        return np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)

    def colors(self) -> np.ndarray:
        return np.random.default_rng(self.topk).integers(0, 256, (self.topk, 3), dtype=np.uint8)

    def edge_colors(self) -> np.ndarray:
        return np.random.default_rng(self.topk + 1000).integers(0, 256, (self.topk, 3), dtype=np.uint8)

    # the restatement's answers, computed once
    def anchors(self) -> np.ndarray:
        if "anchors" not in self._cache:
            self._cache["anchors"] = V.instance_anchors(self.live(), self.live_scores(), self.min_score, self.topk)
        return self._cache["anchors"]

    def order(self) -> np.ndarray:
        if "order" not in self._cache:
            self._cache["order"] = V.instance_order(self.live(), self.live_scores(), self.min_score, self.topk)
        return self._cache["order"]

    def overlay(self, alpha256=128) -> np.ndarray:
        key = ("overlay", alpha256)
        if key not in self._cache:
            self._cache[key] = V.instance_overlay(self.image(), self.live(), self.colors(), self.edge_colors(), alpha256, self.live_scores(),
                                                  self.min_score)
        return self._cache[key]


def _blob_masks(seed, n, h, w, cell=5, p=0.45):
    """n random masks on a coarse grid, blown up and cropped, with single-pixel noise: ragged, overlapping, touching the borders."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, h, w), bool)
    for i in range(n):
        coarse = rng.random((h // cell + 2, w // cell + 2)) < p
        m = np.kron(coarse, np.ones((cell, cell), bool))[2:2 + h, 1:1 + w]
        out[i] = m ^ (rng.random((h, w)) < 0.02)
    return out


def _scores(seed, n):
    return np.random.default_rng(seed).random(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = []
    for h in (1, 63, 64, 65, 130):        # around the word (64 rows) and the tile
        for w in (1, 3, 64, 65, 67):
            out.append(InstCase(f"size_{h}x{w}", _blob_masks(h * 100 + w, 5, h, w), _scores(h + w, 5), 0.2))
    out.append(InstCase("n0", _blob_masks(1, 3, 20, 30), _scores(1, 3), 0.0, n=0, note="an empty table: the picture is copied, every row is -1"))
    out.append(InstCase("n1", _blob_masks(2, 3, 33, 70), _scores(2, 3), 0.0, n=1, note="masks past the count are not drawn"))
    many = np.zeros((100, 70, 90), bool)
    y, x = np.mgrid[0:70, 0:90]
    rng = np.random.default_rng(7)
    for i in range(100):                  # discs of a few radii around the middle: heavy overlap, many equal areas
        cy, cx, r = 35 + rng.integers(-12, 13), 45 + rng.integers(-20, 21), (6, 9, 9, 14, 20)[i % 5]
        many[i] = (y - cy) ** 2 + (x - cx) ** 2 <= r * r
    many[41] = many[17]                   # two identical masks
    many[63] = np.roll(many[17], 3, axis=1)   # and the same area at another place
    out.append(InstCase("n100_overlap", many, _scores(3, 100), 0.1, n=100, note="two chunks of staged masks; ties in area"))
    sp = np.zeros((7, 66, 70), bool)
    sp[0, 10:30, 5:40] = True
    # 1: an empty mask inside the table
    sp[2, :, :] = True                    # a full mask: no edge pixel anywhere
    sp[3, 0, :] = True; sp[3, :, 0] = True; sp[3, -1, :] = True; sp[3, :, -1] = True   # the frame: touches every border
    sp[4, 64, 69] = True                  # one pixel: all edge
    sp[5, 20:23, 50:53] = True            # 9 pixels: odd count, x2 / y2 even
    sp[6, 40:44, 10:15] = True            # 20 pixels: even count; rows 40..43 -> y2 = 83, odd
    out.append(InstCase("special", sp, None, 0.0, note="no scores: every non-empty mask is kept"))
    ring = np.zeros((2, 40, 41), bool)
    yy, xx = np.mgrid[0:40, 0:41]
    d = (yy - 20) ** 2 + (xx - 20) ** 2
    ring[0] = (d <= 18 * 18) & (d >= 12 * 12)      # the median (20, 20) lies in the hole
    ring[1, 3:9, 2:6] = True; ring[1, 30:36, 37:41] = True   # two pieces of 24 pixels: the median lies between them
    out.append(InstCase("median_in_a_hole", ring, np.array([0.9, 0.8], np.float32), 0.5))
    sc = _blob_masks(11, 6, 50, 66)
    s = np.array([0.9, 0.25, 0.5, 0.1, 0.7, 0.5], np.float32)
    out.append(InstCase("min_score_equal", sc, s, 0.5, n=6, note="score == min_score is kept"))
    out.append(InstCase("min_score_above_all", sc, s, 0.95, n=6, note="nothing is kept"))
    return {c.name: c for c in out}


# (case, anchors as tuples, order, picture) of two hand-worked pictures
def hand_cases():
    a = np.zeros((2, 3, 4), bool)
    a[0, :, 0:3] = True                                   # 3 x 3 at the left of a 3 x 4 picture
    a[1, 0, 2] = a[1, 0, 3] = a[1, 1, 3] = True
    # mask 0: columns 0 1 2 three times each -> median 1, rows alike; its column 2 has the picture's column 3 outside the mask -> edge.
    # mask 1: columns 2 3 3 -> 3, rows 0 0 1 -> 0.  (0,2): (0,1) is outside -> edge; (0,3): left and below inside, the rest outside the
    # picture -> blended over the bare image; (1,3): (1,2) outside -> edge.  blend of 100 with 200 at 128: (12800 + 25600 + 128) >> 8 = 150,
    # with 0: (12800 + 128) >> 8 = 50.
    ha = dict(masks=a, scores=None, min_score=0.0, image=np.full((3, 4, 3), 100, np.uint8), colors=[(200, 0, 0), (0, 0, 200)],
              edge_colors=[(1, 2, 3), (4, 5, 6)], alpha256=128,
              anchors=[(0, 9, 2, 2, 0, 0, 2, 2), (1, 3, 6, 0, 2, 0, 3, 1)], order=[0, 1],
              picture=[[(150, 50, 50), (150, 50, 50), (4, 5, 6), (50, 50, 150)],
                       [(150, 50, 50), (150, 50, 50), (1, 2, 3), (4, 5, 6)],
                       [(150, 50, 50), (150, 50, 50), (1, 2, 3), (100, 100, 100)]])
    b = np.zeros((3, 2, 5), bool)
    b[0, 0, 0:2] = True
    b[1, 1, 3:5] = True                                   # the same area: the smaller index is drawn first
    b[2] = True                                           # the full mask scores below min_score: not kept
    # every pixel of masks 0 and 1 has a neighbour in the other row that is outside its mask: all edge.  x2 of columns 0 1 = 1, of 3 4 = 7.
    hb = dict(masks=b, scores=np.array([0.5, 0.5, 0.2], np.float32), min_score=0.5, image=np.zeros((2, 5, 3), np.uint8),
              colors=[(10, 20, 30), (40, 50, 60), (70, 80, 90)], edge_colors=[(7, 7, 7), (8, 8, 8), (9, 9, 9)], alpha256=256,
              anchors=[(0, 2, 1, 0, 0, 0, 1, 0), (1, 2, 7, 2, 3, 1, 4, 1), (-1, 0, 0, 0, 0, 0, 0, 0)], order=[0, 1, -1],
              picture=[[(7, 7, 7), (7, 7, 7), (0, 0, 0), (0, 0, 0), (0, 0, 0)],
                       [(0, 0, 0), (0, 0, 0), (0, 0, 0), (8, 8, 8), (8, 8, 8)]])
    return [ha, hb]


@dataclass
class SemCase:
    name: str
    labels: np.ndarray                    # int32 [H,W]
    K: int
    small_area: int = 4
    large_area: int = 50
    note: str = ""
    _cache: dict = field(default_factory=dict, repr=False)

    @property
    def hw(self):
        return self.labels.shape

    def record(self) -> np.ndarray:
        if "record" not in self._cache:
            self._cache["record"] = V.semantic_record(self.labels, self.K)
        return self._cache["record"]

    def sem_seg(self) -> np.ndarray:
        """float32 [K,H,W] whose first-maximum arg-max is `labels` clipped into [0, K): every second pixel has a second plane with the
        same maximum further up (the tie goes to the lower class)."""
        h, w = self.hw
        lab = np.clip(self.labels, 0, self.K - 1)
        rng = np.random.default_rng(self.K)
        sem = rng.random((self.K, h, w), dtype=np.float32)
        yy, xx = np.mgrid[0:h, 0:w]
        sem[lab, yy, xx] = 2.0
        tie = ((yy + xx) % 2 == 0) & (lab < self.K - 1)
        sem[np.minimum(lab + 1 + (yy + 2 * xx) % 3, self.K - 1)[tie], yy[tie], xx[tie]] = 2.0
        assert np.array_equal(sem.argmax(0), lab)
        return sem


@functools.lru_cache(maxsize=None)
def sem_cases() -> dict:
    out = []
    rng = np.random.default_rng(0)
    a = np.kron(rng.integers(-1, 5, (6, 9)), np.ones((6, 5), np.int64)).astype(np.int32)      # labels -1 .. 4 with K = 3: -1, 3, 4 are outside
    out.append(SemCase("K3", a, 3, 4, 50, "negative labels and labels >= K get id 0"))
    b = np.kron(rng.integers(0, 847, (10, 13)), np.ones((4, 5), np.int64)).astype(np.int32)
    b[0:4, 0:5] = 846; b[4:8, 0:5] = 0; b[8:12, 0:5] = 847; b[12:16, 0:5] = -5
    out.append(SemCase("K847", b, 847, 4, 50, "40 x 65: the ADE-847 vocabulary; more present classes than rows"))
    runs = np.repeat(np.arange(150), 2)[:256].reshape(16, 16).astype(np.int32)                # 128 classes in runs of two
    out.append(SemCase("more_than_MAX_SEGMENTS", runs, 200, 1, 50, "128 present classes of equal count: the 100 smallest indices keep a row"))
    assert len(np.unique(runs)) > MAX_SEGMENTS
    eq = np.zeros((12, 20), np.int32)
    eq[:, 0:5] = 7; eq[:, 5:10] = 2; eq[:, 10:14] = 9; eq[:, 14:18] = 4; eq[:, 18:20] = 5    # counts 60 60 48 48 24
    out.append(SemCase("equal_counts", eq, 10, 4, 50, "ties go to the smaller category: 2 7 4 9 5"))
    sm = np.zeros((30, 70), np.int32)
    sm[2:4, 3:5] = 1; sm[10:11, 20:23] = 1         # class 1: components of 4 and 3 pixels, small_area 5: no label
    sm[15:25, 30:60] = 2                           # class 2: 300 pixels
    sm[0:2, 60:70] = 2                             # and 20 more, not above large_area
    out.append(SemCase("small_component", sm, 3, 5, 250, "a class whose largest component is below small_area"))
    big = np.kron(rng.integers(0, 12288, (8, 8)), np.ones((3, 3), np.int64)).astype(np.int32)
    big[0, 0] = 12287
    out.append(SemCase("K12288", big, 12288, 1, 50, "the largest vocabulary the call takes"))
    return {c.name: c for c in out}
