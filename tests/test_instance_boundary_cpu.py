"""The host restatement of Boundary AP's IoU (odise_amd/instance_eval.py mask_boundary / boundary_iou / image_rows(iou_type="boundary")),
the reference of the device form (tests/test_gpu_instance_boundary.py): against the literal repeated 3x3 erosion, against
sem_boundary.mask_to_boundary, on hand-worked pictures, and against a second dense formulation of the matching written here.  The published
boundary-iou package is no dependency of this project: parity with it is unpinned."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

import inst_cases as IC
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE
from odise_amd import sem_boundary as SB

SIZES = [(1, 1), (1, 130), (130, 1), (63, 5), (64, 5), (65, 5), (200, 300)]


def radii(h, w):
    """1, the formula, 32, 64, 70, the last radius whose window fits (2 r + 1 == min(h, w) on an odd side, one less on an even one) and
    the first at which everything erodes."""
    side = min(h, w)
    rs = {1, SB.boundary_radius(h, w), 32, 64, 70, (side - 1) // 2, (side - 1) // 2 + 1}
    return sorted(r for r in rs if r >= 1)


def literal_boundary(m, r):
    """_mask_to_boundary as it is written: r 3x3 erosions that see zeros outside the picture, subtracted from the mask."""
    m = np.asarray(m) != 0
    return (m & ~ndimage.binary_erosion(m, np.ones((3, 3), bool), iterations=r, border_value=0)).astype(np.uint8)


def edge_masks(h, w):
    """The mask set of the RLE tests and two masks that touch all four picture edges: the full picture with a few holes, and a frame."""
    ms = list(IC.mask_set(h, w))
    holes = np.ones((h, w), np.uint8)
    holes[h // 2, w // 2] = holes[h // 3, (2 * w) // 3] = 0
    frame = np.ones((h, w), np.uint8)
    frame[h // 4:h - h // 4, w // 4:w - w // 4] = 0
    return np.stack(ms + [holes, frame])


@pytest.mark.parametrize("h,w", SIZES)
def test_mask_boundary_is_the_literal_erosion_and_the_semantic_rule(h, w):
    ms = edge_masks(h, w)
    assert np.array_equal(IE.mask_boundary(ms), IE.mask_boundary(ms, 0)) and np.array_equal(IE.mask_boundary(ms), IE.mask_boundary(ms, SB.boundary_radius(h, w)))
    for r in radii(h, w):
        got = IE.mask_boundary(ms.astype(np.float32) * 0.75 if r == 1 else ms, r)
        assert got.dtype == np.uint8 and got.shape == ms.shape
        for k, m in enumerate(ms):
            np.testing.assert_array_equal(got[k], literal_boundary(m, r), err_msg=f"mask {k} r {r}")
            np.testing.assert_array_equal(got[k], SB.mask_to_boundary(m, r), err_msg=f"mask {k} r {r}")
        if 2 * r + 1 > min(h, w):
            np.testing.assert_array_equal(got, ms)                          # everything erodes: the boundary is the mask
    assert IE.mask_boundary(np.zeros((0, h, w), np.uint8)).shape == (0, h, w)


def test_a_square_of_ten_has_a_boundary_of_64():
    m = np.zeros((1, 30, 30), np.uint8)
    m[0, 8:18, 11:21] = 1
    b = IE.mask_boundary(m, 2)
    assert int(b.sum()) == 64 and not b[0, 10:16, 13:19].any() and b[0, 8:18, 11:21].sum() == 64


def _shifted_case(shift):
    gt = IC.rect(10, 50, 10, 50, 64, 64)
    det = IC.rect(10, 50, 10 + shift, 50 + shift, 64, 64)
    return IC.case([det], [.9], [0], [IC.ann(gt)])


def _rows(c, iou_type, radius=None, image=0):
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    return IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"], iou_type=iou_type, radius=radius)


def test_the_shifted_square_matches_in_segm_and_not_in_boundary():
    assert SB.boundary_radius(64, 64) == 2
    c = _shifted_case(4)
    counts = [R.mask_counts(IC.rect(10, 50, 10, 50, 64, 64))]
    iou, m_iou, b_iou = IE.boundary_iou(c["masks"], counts)
    bd, bg = IE.mask_boundary(c["masks"]), IE.mask_boundary(IC.rect(10, 50, 10, 50, 64, 64)[None])
    assert int(bd.sum()) == 304 == int(bg.sum()) and int((bd & bg).sum()) == 144
    assert m_iou[0, 0] == 1440 / 1760 and b_iou[0, 0] == 144 / 464 and iou[0, 0] == 144 / 464
    segm, f0 = _rows(c, "segm")
    bnd, f1 = _rows(c, "boundary")
    assert f0 == 0 == f1
    assert IC.bits(segm["matched"][0], 0) == [1, 1, 1, 1, 1, 1, 1, 0, 0, 0]          # .5 to .8
    assert int(bnd["matched"][0]) == 0
    assert bnd["area"][0] == segm["area"][0] == 1600 and bnd["score"][0] == segm["score"][0]
    # unshifted: every threshold in both tasks
    c = _shifted_case(0)
    for t in ("segm", "boundary"):
        rows, _ = _rows(c, t)
        assert all(IC.bits(rows["matched"][0], a) == [1] * 10 for a in range(4)), t


def test_crowd_and_empty_masks():
    h, w = 64, 64
    det = IC.rect(20, 30, 20, 30, h, w)                                     # 10 x 10 inside the crowd region: r = 2, boundary 64
    crowd = IC.rect(10, 50, 10, 50, h, w)
    empty = np.zeros((h, w), np.uint8)
    counts = [R.mask_counts(crowd), R.mask_counts(empty)]
    iou, m_iou, b_iou = IE.boundary_iou(np.stack([det, empty]), counts, [1, 0])
    bd, bg = IE.mask_boundary(det[None])[0], IE.mask_boundary(crowd[None])[0]
    inter = int((bd & bg).sum())
    assert int(bd.sum()) == 64 and inter == 0 and b_iou[0, 0] == 0 and m_iou[0, 0] == 1.0 and iou[0, 0] == 0
    # a detection on the crowd's edge shares boundary pixels with it: inter / area_b(d), not the union
    det2 = IC.rect(10, 20, 10, 20, h, w)
    iou, m_iou, b_iou = IE.boundary_iou(det2[None], counts[:1], [1])
    b2 = IE.mask_boundary(det2[None])[0]
    inter = int((b2 & bg).sum())
    assert inter == 36 and int(b2.sum()) == 64 and b_iou[0, 0] == 36 / 64 and m_iou[0, 0] == 1.0 and iou[0, 0] == 36 / 64
    assert IE.boundary_iou(det2[None], counts[:1], [0])[2][0, 0] == 36 / (64 + int(bg.sum()) - 36)
    # empty masks on either side give 0 everywhere
    iou, m_iou, b_iou = IE.boundary_iou(np.stack([det, empty]), counts, [1, 0])
    assert not iou[1].any() and not iou[:, 1].any() and not b_iou[1].any() and not b_iou[:, 1].any()
    assert IE.boundary_iou(np.zeros((0, h, w), np.uint8), counts)[0].shape == (0, 2)
    assert IE.boundary_iou(det[None], [])[0].shape == (1, 0)


def dense_boundary_rows(c, image, radius=None):
    """A second formulation of image_rows(iou_type="boundary"): the IoU from the literal erosion and numpy sums, the matching per
    (category, range, threshold) over arrays of ground truths sorted by ignore - the best IoU among the available ones, later on ties."""
    masks = c["masks"] != 0
    n, h, w = masks.shape
    r = SB.boundary_radius(h, w) if radius is None else radius
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    gts = np.stack([IE.decode_runs(runs[offs[i]:offs[i + 1]], h, w) for i in range(len(table))]).astype(bool) if len(table) else np.zeros((0, h, w), bool)
    bd = np.stack([literal_boundary(m, r) for m in masks]).astype(bool) if n else masks
    bg = np.stack([literal_boundary(g, r) for g in gts]).astype(bool) if len(gts) else gts

    def iou_of(a, b):
        inter = (a.reshape(len(a), 1, h * w) & b.reshape(1, len(b), h * w)).sum(2).astype(np.float64)
        aa, ab = a.reshape(len(a), h * w).sum(1).astype(np.float64)[:, None], b.reshape(len(b), h * w).sum(1).astype(np.float64)[None]
        union = np.where(table[:, 1][None] != 0, aa + 0 * ab, aa + ab - inter)
        return np.where(inter > 0, inter / np.where(union > 0, union, 1), 0.0)
    ious = np.minimum(iou_of(masks, gts), iou_of(bd, bg))
    area = masks.reshape(n, -1).sum(1)
    order = np.argsort(-c["scores"][:n], kind="stable")
    rows = np.zeros(n, IE.ROW_DTYPE)
    rows["score"], rows["category"], rows["area"], rows["image"] = c["scores"][order], c["classes"][order], area[order], image
    for a in range(4):
        for t, thr in enumerate(IE.IOU_THRS):
            taken = np.zeros(len(table), bool)
            for k, d in enumerate(order):
                same = table[:, 0] == c["classes"][d]
                ign = (table[:, 1] != 0) | (((table[:, 2] >> a) & 1) != 0)
                ok = same & (ious[d] >= min(thr, 1 - 1e-10)) & (~taken | (table[:, 1] != 0))
                m = -1
                for group in (ok & ~ign, ok & ign):                        # a regular ground truth wins over any ignored one
                    idx = np.flatnonzero(group)
                    if len(idx):
                        best = ious[d][idx].max()
                        m = int(idx[ious[d][idx] == best][-1])
                        break
                bit = np.uint64(1 << (10 * a + t))
                if m >= 0:
                    taken[m] = True
                    rows["matched"][k] |= bit
                    if ign[m]:
                        rows["ignored"][k] |= bit
                elif IE.area_outside(int(area[d]), a):
                    rows["ignored"][k] |= bit
    return rows


@pytest.mark.parametrize("name", sorted(IC.matching_cases()) + ["random", "no_gt", "shifted"])
def test_image_rows_boundary_equal_the_dense_formulation(name):
    c = {"random": lambda: IC.random_case(n=60, n_gt=30, K=3), "no_gt": lambda: IC.random_case(seed=9, n=25, n_gt=0),
         "shifted": lambda: _shifted_case(4)}.get(name, lambda: IC.matching_cases()[name])()
    for radius in (None, 1, 5):
        rows, flags = _rows(c, "boundary", radius, image=3)
        assert flags == 0
        want = dense_boundary_rows(c, 3, radius)
        for field in IE.ROW_DTYPE.names:
            np.testing.assert_array_equal(rows[field], want[field], err_msg=f"{field} r {radius}")
    if name == "random":                                                    # the two tasks part ways somewhere, and the areas stay the masks'
        segm = _rows(c, "segm", image=3)[0]
        rows = _rows(c, "boundary", image=3)[0]
        assert (segm["matched"] != rows["matched"]).any() and np.array_equal(segm["area"], rows["area"])


def test_flags_are_the_segm_task_s():
    c = IC.matching_cases()["two_on_one"]
    table, runs, offs = IE.gt_rows(c["annotations"], {0: 0})
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], [np.r_[runs, 5]], table, num_categories=1, iou_type="boundary")
    assert flags == IE.FLAG_BAD_RUNS and len(rows) == 0
    rows, flags = IE.image_rows(c["masks"], c["scores"], [0, 3], [runs], table, num_categories=1, iou_type="boundary")
    assert flags == IE.FLAG_BAD_CLASS and len(rows) == 0


def test_the_binding_mirrors_the_header():
    import __graft_entry__ as entry
    from odise_amd import _lib
    entry.build()
    lib = _lib.load()
    assert lib.odise_hip_sizeof_inst_boundary_task() == C.sizeof(_lib.InstBoundaryTask) == 24
    protos = _lib.header_prototypes()
    assert len(protos["odise_hip_mask_boundary"]) == 9 and len(protos["odise_hip_mask_boundary_iou"]) == 18
    assert len(protos["odise_hip_instance_eval_boundary"]) == 5
