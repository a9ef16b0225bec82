"""Pictures for the Boundary PQ tests (tests/test_panoptic_boundary_cpu.py, tests/test_gpu_panoptic_boundary.py, tools/pq_boundary_bench.py).

A blocky picture of tests/pq_cases.py alone is a weak Boundary PQ case: at a large radius its small blocks have no interior, B(s) = s, and
the boundary statistics equal the PQ statistics.  `boundary_case` therefore paints two staged pairs of rectangles, sized by the radius,
over such a picture, with the ids of rows the tables already hold (full tables stay full):

    lowered   a wide rectangle and its copy one column to the right: both IoUs stay above one half, the boundary IoU below the mask IoU
    demoted   a rectangle and its copy a sixth of its height down and as far to the right as leaves the mask IoU above one half: the
              rings meet less than the masks do, at any radius that leaves the rectangle an interior

and asserts in the reference that both happen (`assert_boundary_rules_fire`).  The rectangles need (2r + 1) + 8 rows each; a picture
below 64 pixels a side (5x7 in the GPU file) is instead split into two columns on either side, one column apart (`_split`), which
lowers one pair and demotes the other.  Only where the rule itself forbids such pairs is a case compared without the assertion
(`must_fire`): at 1x1 and 1x67 every pixel is a boundary pixel, and an empty table has no candidates."""
import numpy as np

from odise_amd import panoptic_quality as PQ
from odise_amd.sem_boundary import boundary_radius
from pq_cases import Case, blocky_case


class BoundaryCase(Case):
    radius = None   # None: the formula

    def boundary_stats(self, trace=None, into=None):
        return PQ.image_boundary_stats(self.pan_gt, self.gt_rows, self.pan_pred, self.pred_rows, self.C, self.radius, into, trace)

    def assert_boundary_rules_fire(self):
        """A case whose boundary statistics equal its PQ statistics shows nothing: a pair loses its match to the boundary IoU, and a pair
        is matched at a boundary IoU below its mask IoU."""
        tr = {}
        stats, flags = self.boundary_stats(tr)
        assert flags == 0 and tr["demoted"] >= 1 and tr["lowered"] >= 1, (flags, tr)
        assert stats != self.stats()[0]
        return tr


def dense_boundary_pairs(case) -> list:
    """The matched pairs of Boundary PQ as (gt id, pred id, category, iou_b), ascending, by a second formulation: slot maps, "off its
    boundary" = the window's sliding minimum AND maximum equal the pixel (sem_boundary.erode of the slot map and of its complement),
    dense count matrices.  Valid for pictures without a flag."""
    from odise_amd.sem_boundary import erode
    from pq_cases import slot_map
    h, w = case.pan_gt.shape
    r = boundary_radius(h, w) if case.radius is None else case.radius
    g_id, g_cat, g_crowd, g_area = (case.gt_rows[:, k].astype(np.int64) for k in range(4))
    p_id, p_cat = case.pred_rows[:, 0].astype(np.int64), case.pred_rows[:, 2].astype(np.int64)
    ng, n = len(g_id), len(p_id)
    gs, ps = slot_map(case.pan_gt, g_id).reshape(h, w), slot_map(case.pan_pred, p_id).reshape(h, w)

    def on_boundary(m):
        if 2 * r + 1 > min(h, w):
            return np.ones((h, w), bool)
        return (erode(m, r) != m) | (erode(255 - m, r) != 255 - m)
    bg, bp = on_boundary(gs), on_boundary(ps)
    M, MB = np.zeros((ng + 2, n + 2), np.int64), np.zeros((ng + 2, n + 2), np.int64)
    np.add.at(M, (gs.reshape(-1), ps.reshape(-1)), 1)
    np.add.at(MB, (gs[bg & bp], ps[bg & bp]), 1)
    b_area_g, b_area_p = np.bincount(gs[bg], minlength=ng + 2), np.bincount(ps[bp], minlength=n + 2)
    b_void_p = np.bincount(ps[bp & (gs == 0)], minlength=n + 2)
    pairs = []
    for g in range(ng):
        for p in range(n):
            inter = int(M[g + 1, p + 1])
            union = int(M[:, p + 1].sum() + g_area[g] - inter - M[0, p + 1])
            if inter == 0 or g_crowd[g] or g_cat[g] != p_cat[p] or union <= 0:
                continue
            ib = int(MB[g + 1, p + 1])
            ub = int(b_area_p[p + 1] + b_area_g[g + 1] - ib - b_void_p[p + 1])
            v = min(inter / union, ib / ub if ub > 0 else 0.0)
            if v > 0.5:
                pairs.append((int(g_id[g]), int(p_id[p]), int(g_cat[g]), v))
    return sorted(pairs)


def _paint(case, gi, pj, y0, x0, b, a, dy, dx):
    """Ground-truth row gi over rows y0 .. y0 + b, columns x0 .. x0 + a and nowhere else (VOID where it was); predicted row pj over the
    same rectangle moved by (dy, dx) and nowhere else."""
    case.pan_gt[case.pan_gt == case.gt_rows[gi, 0]] = 0
    case.pan_pred[case.pan_pred == case.pred_rows[pj, 0]] = 0
    case.pan_gt[y0:y0 + b, x0:x0 + a] = case.gt_rows[gi, 0]
    case.pan_pred[y0 + dy:y0 + dy + b, x0 + dx:x0 + dx + a] = case.pred_rows[pj, 0]
    case.pred_rows[pj, 2] = case.gt_rows[gi, 1]


def _split(case, g1, g2):
    """A picture too small for the rectangles: ground-truth rows g1 | g2 split it at column c = w // 2 + 1, the first two predicted rows at
    column c + 1, ids and tables as they were.  5 x 7 at r = 1: the left pair has iou 20 / 25 and b_iou 11 / 19 (lowered), the right pair
    10 / 15 and 7 / 15 (demoted); a ground-truth row that owned pixels before owns none now."""
    h, w = case.pan_gt.shape
    c = w // 2 + 1
    case.pan_gt[:, :c], case.pan_gt[:, c:] = case.gt_rows[g1, 0], case.gt_rows[g2, 0]
    case.pan_pred[:, :c + 1], case.pan_pred[:, c + 1:] = case.pred_rows[0, 0], case.pred_rows[1, 0]
    case.pred_rows[0, 2], case.pred_rows[1, 2] = case.gt_rows[g1, 1], case.gt_rows[g2, 1]
    case.gt_rows[g1, 3], case.gt_rows[g2, 3] = h * c, h * (w - c)
    case.pred_rows = case.pred_rows[:2]


def must_fire(case) -> bool:
    """Whether the rule allows a demoted and a lowered pair at all, i.e. whether the staged pairs are painted and
    `assert_boundary_rules_fire` applies: some pixel is off its boundary (2r + 1 <= min(h, w)) and both tables can hold two candidates."""
    h, w = case.pan_gt.shape
    r = boundary_radius(h, w) if case.radius is None else case.radius
    plain = int((case.gt_rows[:, 2] == 0).sum()) if len(case.gt_rows) else 0
    return 2 * r + 1 <= min(h, w) and plain >= 2 and len(case.pred_rows) >= 2


def boundary_case(seed, h, w, n_gt, n, radius=None, C=6, cell=(11, 13)) -> BoundaryCase:
    """blocky_case(seed, h, w, n_gt, n) with the two staged pairs painted in wherever `must_fire`: the rectangles from 64 pixels a side,
    the two-column split of `_split` below that.  Rows that the rectangles covered get a pixel back; the JSON area of a painted ground-truth
    row is its pixel count, every other row keeps the area it had (and may now disagree with the map)."""
    base = blocky_case(seed, h, w, n_gt, n, C, cell)
    case = BoundaryCase(base.pan_gt.copy(), base.gt_rows.copy(), base.pan_pred.copy(), base.pred_rows.copy(), C)
    case.radius = radius
    r = boundary_radius(h, w) if radius is None else radius
    plain = [i for i in range(len(case.gt_rows)) if case.gt_rows[i, 2] == 0 and (case.pan_gt == case.gt_rows[i, 0]).any()]
    if not must_fire(case):
        return case
    rng = np.random.default_rng(seed + 7)
    if min(h, w) < 64:   # the whole picture is repainted: rows without pixels serve as well
        _split(case, *(int(v) for v in rng.choice(np.flatnonzero(case.gt_rows[:, 2] == 0), 2, replace=False)))
        return case
    assert len(plain) >= 2
    g1, g2 = (int(v) for v in rng.choice(plain, 2, replace=False))
    p1, p2 = (int(v) for v in rng.choice(len(case.pred_rows), 2, replace=False))
    b = min(2 * r + 9, (h - 6) // 2 - max(1, (2 * r + 9) // 6))       # rows of a rectangle: an interior of 8 rows where the picture has room
    a1 = min(4 * b, w - 3)
    _paint(case, g1, p1, 1, 1, b, a1, 0, 1)
    a2 = min(2 * b, (w - 3) * 3 // 4)
    dy = max(1, b // 6)
    _paint(case, g2, p2, b + 3, 1, b, a2, dy, 1)

    def iou_above_half(d):   # of the pair with the prediction d columns to the right; VOID below the prediction leaves the union
        void = int((case.pan_gt[b + 3 + dy:b + 3 + dy + b, 1 + d:1 + d + a2] == 0).sum())
        inter = (b - dy) * (a2 - d)
        return 2 * inter > 2 * a2 * b - inter - void
    dx = max(d for d in range(1, a2 // 3) if iou_above_half(d))
    _paint(case, g2, p2, b + 3, 1, b, a2, dy, dx)
    painted = np.zeros((h, w), bool)
    painted[:2 * b + 4 + dy, :] = True
    # a pixel back for every row that lost all of its own, taken from an id of the unpainted part that has pixels to spare
    free = np.flatnonzero(~painted.reshape(-1))
    for pan, ids in ((case.pan_gt, [case.gt_rows[i, 0] for i in range(len(case.gt_rows)) if (base.pan_gt == case.gt_rows[i, 0]).any()]),
                     (case.pan_pred, case.pred_rows[:, 0])):
        flat = pan.reshape(-1)
        for i in ids:
            if not (flat == i).any():
                for pos in rng.permutation(free):
                    if (flat == flat[pos]).sum() > 1:
                        flat[pos] = i
                        break
    for gi in (g1, g2):
        case.gt_rows[gi, 3] = int((case.pan_gt == case.gt_rows[gi, 0]).sum())
    return case


# (seed, h, w, n_gt, n) at the formula's radius: 1 pixel; W % 4 = 3 at r = 1; one row (2r + 1 > H: the degenerate case); r = 3; r = 8;
# r = 14 and several blocks
SIZES = [(8, 1, 1, 1, 1), (7, 5, 7, 3, 2), (1, 1, 67, 5, 4), (1, 67, 131, 37, 20), (12, 200, 333, 37, 20), (11, 512, 512, 37, 20)]
# explicit radii on 200 x 333: one, two, three and four growing-window passes per direction (2r + 1 = 3, 5, 7, 17, 43, 81)
RADII = [1, 2, 3, 8, 21, 40]
# (n_gt, n): (254, 100) counts both matrices in global memory, and its "absent" ground-truth slot is 255
TABLES = [(0, 20), (37, 0), (37, 100), (254, 100)]


def size_case(seed, h, w, n_gt, n):
    return boundary_case(seed, h, w, n_gt, n)


def radius_case(radius):
    return boundary_case(40 + radius, 200, 333, 37, 20, radius)


def table_case(n_gt, n):
    return boundary_case(100 + 3 * n_gt + n, 200, 333, n_gt, n)


def stream_cases():
    return [boundary_case(1, 67, 131, 37, 20), boundary_case(108, 200, 333, 37, 100), boundary_case(12, 200, 333, 37, 20)]


def gpu_cases() -> dict:
    """Every generated case of the GPU file, by name."""
    out = {f"size_{h}x{w}": size_case(s, h, w, n_gt, n) for s, h, w, n_gt, n in SIZES}
    out.update({f"radius_{r}": radius_case(r) for r in RADII})
    out.update({f"tables_{n_gt}_{n}": table_case(n_gt, n) for n_gt, n in TABLES})
    out.update({f"stream_{i}": c for i, c in enumerate(stream_cases())})
    out["unaligned"] = boundary_case(1, 67, 131, 37, 20)
    return out
