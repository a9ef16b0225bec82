"""CPU: the numpy restatement of the drawing rules (odise_amd/visualize.py) - the reference tests/test_gpu_visualize.py holds the device
to - against independent formulations: scipy.ndimage.label with a full 3x3 structure, np.median on np.nonzero, a literal per-pixel loop,
and two hand-worked pictures."""
import numpy as np
import pytest
from scipy import ndimage

from odise_amd import visualize as V
from vis_cases import cases, hand_cases

CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_roots_are_scipy_components_with_minimum_index(name):
    case = CASES[name]
    ids, roots = case.ids, case.roots()
    H, W = ids.shape
    index = np.arange(H * W).reshape(H, W)
    ref = np.full((H, W), -1, np.int64)
    for l in np.unique(ids):
        if l <= 0:
            continue
        lab, n = ndimage.label(ids == l, structure=np.ones((3, 3), int))
        mins = ndimage.minimum(index, lab, np.arange(1, n + 1))
        ref[lab > 0] = np.asarray(mins, np.int64)[lab[lab > 0] - 1]
    assert roots.dtype == np.int32 and np.array_equal(roots, ref)
    assert np.array_equal(roots < 0, ids <= 0)


def test_the_shapes_are_what_they_claim():
    assert np.unique(CASES["serpentine"].roots()).tolist() == [-1, 0]
    cb = CASES["checkerboard"].roots()
    assert np.unique(cb).tolist() == [0, 1]                              # two components under 8-connectivity
    four, n4 = ndimage.label(CASES["checkerboard"].ids == 1)            # the default structure is 4-connectivity
    assert n4 == (CASES["checkerboard"].ids == 1).sum()
    assert len(np.unique(CASES["rings"].roots())) == len(range(0, 34, 4))


def independent_anchors(case):
    """scipy's components per table row, np.argmax over its label order, np.median on np.nonzero."""
    out = []
    seen = set()
    for r, (i, isthing, _) in enumerate(case.segments):
        if i <= 0 or i in seen:
            continue
        seen.add(i)
        mask = case.ids == i
        if not mask.any():
            continue
        if isthing:
            picks = [mask]
        else:
            lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
            areas = np.bincount(lab.ravel())[1:]
            k = int(np.argmax(areas))
            if areas[k] < case.small_area:
                continue
            picks = [lab == c + 1 for c in range(n) if c == k or areas[c] > case.large_area]     # scipy labels in row-major order of first pixels
        for m in picks:
            ys, xs = np.nonzero(m)
            my, mx = np.median(np.nonzero(m), axis=1)
            out.append((r, int(m.sum()), int(2 * mx), int(2 * my), xs.min(), ys.min(), xs.max(), ys.max()))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_anchors_against_scipy_and_np_median(name):
    case = CASES[name]
    got = [tuple(int(v) for v in a) for a in case.anchors()]
    assert got == [tuple(int(v) for v in a) for a in independent_anchors(case)]


def test_every_branch_of_the_anchor_rules_occurs():
    rows = [int(a["segment_row"]) for a in CASES["thresholds"].anchors()]
    assert rows == [1, 2, 2, 3, 4, 5]            # too small: none; largest only; largest plus large; a thing in two pieces: one; == small_area
    thing = CASES["thresholds"].anchors()[3]
    assert thing["area"] == 12 + 27 and (thing["y0"], thing["y1"]) == (1, 38)
    rows = [int(a["segment_row"]) for a in CASES["mismatch"].anchors()]
    assert rows == [2, 3, 3, 5]                  # rows 1, 4 without pixels, row 6 a repeated id
    assert [int(a["segment_row"]) for a in CASES["defaults"].anchors()] == [0, 2, 3, 4]
    assert CASES["defaults"].anchors()[0]["area"] > V.LARGE_AREA
    assert len(CASES["equal_areas"].anchors()) == 2 and len(CASES["equal_areas_largest_only"].anchors()) == 1
    assert CASES["equal_areas"].anchors()[0]["y0"] == 2          # the earlier of the two 36-pixel components
    assert len(CASES["many_anchors"].anchors()) == 32


def test_hand_worked_pictures():
    for case, want in hand_cases():
        assert [tuple(int(v) for v in a) for a in case.anchors()] == want, case.name


def test_overlay_against_a_per_pixel_loop():
    case = CASES["mismatch"]
    ids = case.ids[:14, 36:90].copy()            # pieces of ids 3, 4, 99 and VOID
    ids[0, 0] = 3
    H, W = ids.shape
    rng = np.random.default_rng(1)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    colors = case.colors()
    rows = {}
    for r, (i, _, _) in enumerate(case.segments):
        rows.setdefault(i, r)
    for alpha in (0, 77, 256):
        edge = (9, 200, 31)
        want = image.copy()
        for y in range(H):
            for x in range(W):
                i = int(ids[y, x])
                if i <= 0 or i not in rows:
                    continue
                nb = [(y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)]
                if any(0 <= b < H and 0 <= a < W and ids[b, a] != i for b, a in nb):
                    want[y, x] = edge
                    continue
                for c in range(3):
                    want[y, x, c] = (int(image[y, x, c]) * (256 - alpha) + int(colors[rows[i], c]) * alpha + 128) >> 8
        got = V.panoptic_overlay(image, ids, case.segments, colors, alpha, edge)
        assert got.dtype == np.uint8 and np.array_equal(got, want), alpha
        assert (got != image).any() and (got[ids == 99] == image[ids == 99]).all()


def test_segment_colors_and_demo_arguments():
    md = {"stuff_colors": [(10, 20, 30), (40, 50, 60)], "thing_colors": [(200, 100, 0)], "stuff_classes": ["sky", "road"], "thing_classes": ["cat"]}
    segs = [(1, 0, 1), (2, 1, 0), (3, 1, 0), (4, 0, 7)]
    col = V.segment_colors(segs, md)
    assert col.dtype == np.uint8 and col.shape == (4, 3) and tuple(col[0]) == (40, 50, 60)
    assert np.abs(col[1].astype(int) - (200, 100, 0)).max() <= 24 and tuple(col[1]) != tuple(col[2])    # jitter by segment id
    assert np.array_equal(col, V.segment_colors(segs, md))                                             # and deterministic
    assert V.segment_names(segs, md) == ["road", "cat", "cat", "class 7"]
    pic = V.draw_panoptic_seg(np.zeros((40, 90, 3), np.uint8), cases()["thresholds"].ids, cases()["thresholds"].segments)
    assert pic.shape == (40, 90, 3) and pic.dtype == np.uint8 and pic.any()

    from odise_amd import demo
    args = demo.parse_args(["--input", "a.jpg", "b.png", "--output", "out", "--vocab", "black pickup truck, pickup truck; blue sky, sky", "--synthetic"])
    assert args.input == ["a.jpg", "b.png"] and args.output == "out" and args.synthetic
    assert demo.extra_classes(args.vocab) == [["black pickup truck", "pickup truck"], ["blue sky", "sky"]]
    assert demo.output_path("out", "dir/a.jpg") == "out/a.png"
    with pytest.raises(SystemExit):
        demo.parse_args(["--output", "out"])
