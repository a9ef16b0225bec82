"""Crafted inputs of the test-time-augmentation tests: the smallest that can still go wrong.  The views of a case come from ONE smooth
low-resolution field per query, resampled to each view's logit grid (mirrored for a mirrored view) plus small noise, and from one set of
class rows plus small noise: the views agree, so the class gaps are wide (tests/test_tta_cpu.py asserts the decided share)."""
import numpy as np

# name: (Q, K, out (h, w), [(h4, w4, img (h, w), hflip)], twin)
SPECS = {
    "q7_k3_a1": (7, 3, (32, 48), [(8, 12, (32, 48), False)], None),
    "q7_k3_a2": (7, 3, (32, 48), [(8, 12, (32, 48), False), (8, 12, (32, 48), True)], None),
    # odd width (the out_w-1-x mirror), 37 * 53 = 1961 pixels: a multiple of neither 32 nor 128
    "q20_k133_a4": (20, 133, (37, 53), [(12, 16, (37, 53), False), (12, 16, (37, 53), True), (16, 24, (56, 80), False), (16, 24, (56, 80), True)], None),
    # depth 6 * 104 = 624; the first view in the exact x4 geometry, the others img < pad and out != img (the generic sampler)
    "q100_k150_a6": (100, 150, (64, 96), [(16, 24, (64, 96), False), (16, 24, (64, 96), True), (24, 32, (86, 128), False), (24, 32, (86, 128), True),
                                         (32, 48, (120, 180), False), (32, 48, (120, 180), True)], None),
    # class-loop tail: 847 = 4 * 192 + 79 = 26 * 32 + 15
    "q100_k847_a2": (100, 847, (33, 47), [(12, 16, (40, 57), False), (12, 16, (40, 57), True)], None),
    # class 250 repeats class 5: another class tile AND another pass over S (192 classes a pass above 160): the first maximum wins
    "q20_k300_twin": (20, 300, (32, 48), [(8, 12, (32, 48), False), (12, 16, (40, 60), True)], (5, 250)),
}


def _sample(field, ys, xs):
    """field [Q, gh, gw] bilinearly at fractional positions ys [n], xs [m] in 0..1 -> [Q, n, m]."""
    Q, gh, gw = field.shape
    fy, fx = np.clip(ys, 0, 1) * (gh - 1), np.clip(xs, 0, 1) * (gw - 1)
    y0, x0 = np.minimum(fy.astype(int), gh - 2), np.minimum(fx.astype(int), gw - 2)
    ty, tx = (fy - y0)[None, :, None], (fx - x0)[None, None, :]
    rows = field[:, y0, :] * (1 - ty) + field[:, y0 + 1, :] * ty
    return rows[:, :, x0] * (1 - tx) + rows[:, :, x0 + 1] * tx


def _class_rows(rng, Q, K, twin=None):
    """[Q, K+1] logits: query q has probability level_q on its class, the levels a geometric ladder from 0.3 to 0.95 (neighbours 1.2 % apart
    at Q = 100, six times the device bound) in random order, the classes distinct where K >= Q, one query in ten on the null class.  Where
    several saturated masks overlap, the winner is then decided by the ladder and not by a near-tie of two probabilities."""
    z = rng.uniform(-1.0, 1.0, (Q, K + 1))
    lab = rng.permutation(K)[:Q] if K >= Q else np.arange(Q) % K
    lab = np.where((rng.random(Q) < 0.1) & (np.arange(Q) > 0), K, lab)
    if twin is not None:                                                   # query 0 (on everywhere) carries the repeated class; nobody else its copy
        lab = np.where((lab == twin[0]) | (lab == twin[1]), K, lab)
        lab[0] = twin[0]
    level = rng.permutation(0.3 * (0.95 / 0.3) ** (np.arange(Q) / max(Q - 1, 1)))
    low = int(level.argmin())
    level[0], level[low] = level[low], level[0]
    z[np.arange(Q), lab] = -np.inf
    z[np.arange(Q), lab] = np.log(level / (1.0 - level)) + np.log(np.exp(z).sum(-1))
    return z


def make(name):
    Q, K, out, views, twin = SPECS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    # steep and sparse: a query is on (+24) at one grid node in twelve (at most three queries a node on average) and off (-24) elsewhere, so its mask saturates, a transition is a pixel
    # wide and few masks overlap; query 0 is on everywhere (no pixel without a mask) and holds the lowest step of the ladder
    field = np.where(rng.random((Q, 5, 7)) < min(1.0 / 12, 3.0 / Q), 24.0, -24.0)
    field[0] = 24.0
    cls = _class_rows(rng, Q, K, twin)
    if twin is not None:
        cls[:, twin[1]] = cls[:, twin[0]]
    vs = []
    for h4, w4, img, hflip in views:
        pad = (4 * h4, 4 * w4)
        ys, xs = (np.arange(h4) + 0.5) * 4 / img[0], (np.arange(w4) + 0.5) * 4 / img[1]
        lg = _sample(field, ys, 1.0 - xs if hflip else xs) + rng.normal(0, 0.05, (Q, h4, w4))
        mc = cls + rng.normal(0, 0.002, cls.shape)
        if twin is not None:
            mc[:, twin[1]] = mc[:, twin[0]]
        mc = mc - np.log(np.exp(mc).sum(-1, keepdims=True))                 # log-probabilities, as the classification stage hands them over
        mc = mc.astype(np.float32)
        if twin is not None:
            mc[:, twin[1]] = mc[:, twin[0]]
        vs.append({"h4": h4, "w4": w4, "pad": pad, "img": tuple(img), "hflip": hflip, "mask_cls": mc,
                   "logits": lg.astype(np.float16).astype(np.float32)})
    return {"name": name, "Q": Q, "K": K, "out": tuple(out), "views": vs, "twin": twin}


_CACHE = {}


def case(name):
    """(case, float64 reference): computed once, shared, never modified."""
    if name not in _CACHE:
        import tta_reference as TR
        c = make(name)
        ref = TR.tta(c)
        ref.setflags(write=False)
        _CACHE[name] = (c, ref)
    return _CACHE[name]


NAMES = list(SPECS)
