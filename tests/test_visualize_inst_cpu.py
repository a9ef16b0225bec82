"""CPU: the numpy restatement of instance and semantic drawing (odise_amd.visualize: instance_anchors / instance_order /
instance_overlay / semantic_record) against independent formulations - np.median on np.nonzero, a stable sort, a per-pixel loop,
np.unique, scipy.ndimage.label - and against hand-worked pictures; the demo's --task arguments."""
import numpy as np
import pytest
from scipy import ndimage

from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS
from vis_inst_cases import cases, hand_cases, sem_cases

CASES = cases()
SEM = sem_cases()


def _kept(case):
    m, s = case.live(), case.live_scores()
    return [bool(m[i].any()) and (s is None or bool(np.float32(s[i]) >= np.float32(case.min_score))) for i in range(len(m))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_anchors_against_median_and_nonzero(name):
    case = CASES[name]
    got = case.anchors()
    assert got.dtype == V.ANCHOR_DTYPE and got.shape == (case.topk,)
    kept = _kept(case)
    for i in range(case.topk):
        if i >= len(kept) or not kept[i]:
            assert tuple(got[i]) == (-1, 0, 0, 0, 0, 0, 0, 0), (name, i)
            continue
        ys, xs = np.nonzero(case.masks[i])
        want = (i, len(ys), int(2 * np.median(xs)), int(2 * np.median(ys)), xs.min(), ys.min(), xs.max(), ys.max())
        assert tuple(int(v) for v in got[i]) == tuple(int(v) for v in want), (name, i)


@pytest.mark.parametrize("name", sorted(CASES))
def test_order_against_a_stable_sort(name):
    case = CASES[name]
    kept = _kept(case)
    area = [int(m.sum()) for m in case.live()]
    drawn = sorted([i for i in range(len(kept)) if kept[i]], key=lambda i: -area[i])      # sorted is stable: equal areas stay in index order
    want = np.full(case.topk, -1, np.int32)
    want[drawn] = np.arange(len(drawn))
    assert np.array_equal(case.order(), want)


def _overlay_loop(image, masks, order, colors, edge_colors, alpha):
    H, W = image.shape[:2]
    out = image.copy()
    drawn = sorted([i for i in range(len(masks)) if order[i] >= 0], key=lambda i: order[i])
    for y in range(H):
        for x in range(W):
            c = [int(v) for v in image[y, x]]
            for i in drawn:
                m = masks[i]
                if not m[y, x]:
                    continue
                if any(0 <= b < H and 0 <= a < W and not m[b, a] for b, a in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x))):
                    c = [int(v) for v in edge_colors[i]]
                else:
                    c = [(c[k] * (256 - alpha) + int(colors[i][k]) * alpha + 128) >> 8 for k in range(3)]
            out[y, x] = c
    return out


@pytest.mark.parametrize("name,alpha", [("size_65x67", 128), ("size_1x3", 77), ("size_63x1", 128), ("special", 0), ("special", 128), ("special", 256),
                                        ("median_in_a_hole", 200), ("min_score_equal", 128), ("min_score_above_all", 128), ("n0", 128), ("n1", 128)])
def test_overlay_against_a_per_pixel_loop(name, alpha):
    case = CASES[name]
    got = case.overlay(alpha)
    want = _overlay_loop(case.image(), case.live(), case.order(), case.colors(), case.edge_colors(), alpha)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if name in ("n0", "min_score_above_all"):
        assert np.array_equal(got, case.image())
    elif alpha:
        assert (got != case.image()).any()


def test_what_the_special_masks_are_there_for():
    case = CASES["special"]
    a, o = case.anchors(), case.order()
    assert a[1]["segment_row"] == -1 and o[1] == -1                                   # the empty mask
    pic = case.overlay(256)
    e = case.edge_colors()
    full_only = case.masks[2] & ~(case.masks[0] | case.masks[3] | case.masks[4] | case.masks[5] | case.masks[6])
    assert o[2] == 0 and (pic[full_only] == case.colors()[2]).all()                   # the full mask is drawn first and has no edge pixel
    assert tuple(pic[64, 69]) == tuple(e[4])                                          # the one-pixel mask is all edge (drawn last)
    assert a[5]["area"] % 2 == 1 and a[5]["x2"] % 2 == 0 and a[6]["area"] % 2 == 0 and a[6]["y2"] % 2 == 1
    ring = CASES["median_in_a_hole"]
    r = ring.anchors()
    assert not ring.masks[0, r[0]["y2"] // 2, r[0]["x2"] // 2] and not ring.masks[1, r[1]["y2"] // 2, r[1]["x2"] // 2]
    many = CASES["n100_overlap"]
    assert many.masks[17].sum() == many.masks[41].sum() == many.masks[63].sum()
    assert 0 <= many.order()[17] < many.order()[41] < many.order()[63] and (many.order() >= 0).sum() > 50   # equal areas: by index
    eq = CASES["min_score_equal"]
    assert list(eq.order() >= 0) == [True, False, True, False, True, True]
    assert (CASES["min_score_above_all"].order() == -1).all()


def test_hand_worked_pictures():
    for hc in hand_cases():
        anchors = V.instance_anchors(hc["masks"], hc["scores"], hc["min_score"])
        assert [tuple(int(v) for v in a) for a in anchors] == hc["anchors"]
        assert list(V.instance_order(hc["masks"], hc["scores"], hc["min_score"])) == hc["order"]
        pic = V.instance_overlay(hc["image"], hc["masks"], hc["colors"], hc["edge_colors"], hc["alpha256"], hc["scores"], hc["min_score"])
        assert pic.tolist() == [[list(p) for p in row] for row in hc["picture"]]


@pytest.mark.parametrize("name", sorted(SEM))
def test_semantic_record_against_unique(name):
    case = SEM[name]
    rec = case.record()
    h, w = case.hw
    ids, n, rows = rec[:h * w].reshape(h, w), int(rec[h * w]), rec[h * w + 1:].reshape(MAX_SEGMENTS, 3)
    assert rec.dtype == np.int32 and rec.shape == (h * w + 1 + 3 * MAX_SEGMENTS,)
    cats, counts = np.unique(case.labels[(case.labels >= 0) & (case.labels < case.K)], return_counts=True)
    want = sorted(zip(cats.tolist(), counts.tolist()), key=lambda t: (-t[1], t[0]))[:MAX_SEGMENTS]
    assert n == len(want) and rows[:n].tolist() == [[c + 1, 0, c] for c, _ in want] and not rows[n:].any()
    kept = np.isin(case.labels, [c for c, _ in want])
    assert np.array_equal(ids, np.where(kept, case.labels + 1, 0))
    if name == "more_than_MAX_SEGMENTS":
        assert n == MAX_SEGMENTS < len(cats) and (ids == 0).any()
    if name == "equal_counts":
        assert rows[:n, 2].tolist() == [2, 7, 4, 9, 5]
    sem = case.sem_seg()
    assert np.array_equal(V.semantic_record(V.sem_labels(sem), case.K), V.semantic_record(np.clip(case.labels, 0, case.K - 1), case.K))


def test_semantic_record_is_drawn_by_the_panoptic_restatements_as_draw_sem_seg_draws():
    """The record through segment_anchors, against scipy.ndimage.label per class: a label at the largest 8-connected component and at
    every other one above large_area, none when the largest is below small_area."""
    case = SEM["small_component"]
    h, w = case.hw
    rec = case.record()
    n = int(rec[h * w])
    ids, rows = rec[:h * w].reshape(h, w), rec[h * w + 1:h * w + 1 + 3 * n].reshape(n, 3)
    got = V.segment_anchors(ids, rows, case.small_area, case.large_area)
    want = []
    for r, (_, isthing, cat) in enumerate(rows):
        assert isthing == 0
        lab, k = ndimage.label(case.labels == cat, structure=np.ones((3, 3), int))
        areas = np.bincount(lab.ravel())[1:]
        best = int(np.argmax(areas))
        if areas[best] < case.small_area:
            continue
        for c in range(k):
            if c == best or areas[c] > case.large_area:
                ys, xs = np.nonzero(lab == c + 1)
                want.append((r, len(ys), int(2 * np.median(xs)), int(2 * np.median(ys)), xs.min(), ys.min(), xs.max(), ys.max()))
    assert [tuple(int(v) for v in a) for a in got] == [tuple(int(v) for v in a) for a in want]
    assert sorted(set(rows[[a[0] for a in want], 2].tolist())) == [0, 2]             # class 1 (components of 4 and 3 < 5) has no label
    colors = V.segment_colors(rows)
    pic = V.panoptic_overlay(np.zeros((h, w, 3), np.uint8), ids, rows, colors, 256, (255, 255, 255))
    inner = np.zeros((h, w), bool)
    inner[16:24, 31:59] = True                                                       # inside class 2's block
    assert (pic[inner] == colors[list(rows[:, 2]).index(2)]).all()
    twin = V.draw_sem_seg(np.zeros((h, w, 3), np.uint8), case.labels, case.K, None, 128, (0, 0, 0), case.small_area, case.large_area)
    assert twin.shape == (h, w, 3) and twin.dtype == np.uint8 and twin.any()


def test_instance_colors_texts_and_the_host_twin():
    md = {"thing_colors": [(200, 100, 0), (10, 20, 30)], "thing_classes": ["cat", "dog"]}
    col = V.instance_colors([0, 0, 1, 5], md)
    assert col.dtype == np.uint8 and col.shape == (4, 3)
    assert np.abs(col[0].astype(int) - (200, 100, 0)).max() <= 24 and tuple(col[0]) != tuple(col[1])   # jitter by table index
    assert np.array_equal(col, V.instance_colors([0, 0, 1, 5], md))
    edge = V.instance_edge_colors([(200, 200, 200), (10, 20, 30), (128, 128, 128)])
    assert edge.tolist() == [[60, 60, 60], [182, 185, 188], [38, 38, 38]]             # light -> 3/10, dark -> 7/10 of the way to white
    assert V.instance_texts([0, 1, 5], [0.987, 0.5, 0.004], md) == ["cat 99%", "dog 50%", "class 5 0%"]
    case = CASES["median_in_a_hole"]
    pic = V.draw_instance_predictions(case.image(), case.masks, [0, 1], case.scores, md, 128, case.min_score)
    assert pic.shape == case.image().shape and pic.dtype == np.uint8 and (pic != case.image()).any()


def test_demo_task_arguments_and_the_unchanged_default_route():
    from odise_amd import demo
    base = ["--input", "a.jpg", "--output", "out"]
    args = demo.parse_args(base)
    assert args.task == "panoptic" and args.confidence_threshold == 0.5
    args = demo.parse_args(base + ["--task", "instance", "--confidence-threshold", "0.3"])
    assert args.task == "instance" and args.confidence_threshold == 0.3
    assert demo.parse_args(base + ["--task", "semantic"]).task == "semantic"
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--task", "depth"])

    # the default route: panoptic head on, the record drawn by draw_panoptic_seg, nothing else touched
    class Inner:
        keep_instance_selection, instance_rle, semantic_argmax, num_classes = False, False, False, 3

        def open_state_dict(self):
            return {"saved": 1}

        def load_open_state_dict(self, d):
            self.loaded = d

        def infer_device(self, images, layout, img_hw, out_sizes, pan_out=None):
            self.call = dict(pan_out=pan_out, flags=(self.keep_instance_selection, self.instance_rle, self.semantic_argmax))
            return [{}]

    class Wrapper:
        model, open_state_dict = Inner(), {"open": 1}

    class Vis:
        def draw_panoptic_seg(self, image, record, hw):
            return ("panoptic", record, hw)

    class Arr:
        shape = (6, 8, 3)

    class Ctx:
        def empty(self, shape, dtype):
            return ("record", shape)

    import odise_amd.ingest as ingest
    saved = ingest.HipDatasetMapper
    ingest.HipDatasetMapper = lambda ctx, a, b: type("M", (), {"_finish": staticmethod(lambda d, im: {"image": im})})()
    try:
        got = demo.run_on_image(Ctx(), Wrapper, Vis(), Arr())
    finally:
        ingest.HipDatasetMapper = saved
    assert got == ("panoptic", ("record", (6 * 8 + 1 + 3 * MAX_SEGMENTS,)), (6, 8))
    assert Wrapper.model.call == dict(pan_out=[("record", (6 * 8 + 1 + 3 * MAX_SEGMENTS,))], flags=(False, False, False))
    assert Wrapper.model.loaded == {"saved": 1}
