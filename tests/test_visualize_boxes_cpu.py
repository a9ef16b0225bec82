"""CPU: the host twins of odise_hip_instance_draw_boxes (odise_amd.visualize instance_order_boxes / instance_anchors_boxes /
instance_overlay_boxes, draw_instance_predictions(boxes=)) against a per-pixel Python loop written from the rule in include/odise_hip.h,
and on two hand-worked pictures.  Integers and bytes: everything is exact."""
import math
import struct

import numpy as np
import pytest

import vis_box_cases as BX
from odise_amd import visualize as V

CASES = BX.cases()
RECTS = sorted(n for n in CASES if n.startswith("rects_"))


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def trunc(v):
    return int(max(-2.0 ** 29, min(2.0 ** 29, float(v))))


def loop_reference(case):
    """-> (order list, anchors tuples, picture) by plain loops over instances and pixels"""
    h, w = case.hw
    n = case.count()
    masks, boxes, scores = case.masks[:n], [[float(v) for v in b] for b in case.boxes[:n]], case.live_scores()
    kept, key = [], {}
    for i in range(n):
        x0, y0, x1, y1 = boxes[i]
        ok = masks[i].any() and (scores is None or f32(scores[i]) >= f32(case.min_score))
        ok = ok and all(math.isfinite(v) for v in boxes[i]) and x1 > x0 and y1 > y0
        if ok:
            kept.append(i)
            key[i] = f32(f32(x1 - x0) * f32(y1 - y0))
    kept.sort(key=lambda i: (-key[i], i))
    order = [-1] * case.topk
    anchors = [(-1, 0, 0, 0, 0, 0, 0, 0)] * case.topk
    pic = case.image().astype(int).tolist()
    colors, edges = case.colors().tolist(), case.edge_colors().tolist()
    for rank, i in enumerate(kept):
        order[i] = rank
        x0, y0, x1, y1 = boxes[i]
        ix0, iy0, ix1, iy1 = trunc(x0), trunc(y0), trunc(x1), trunc(y1)
        tx, ty = ix0, iy0
        if key[i] < case.small_area or f32(y1 - y0) < 40:
            if y1 >= h - 5:
                tx = ix1
            else:
                ty = iy1
        anchors[i] = (i, int(masks[i].sum()), 2 * tx, 2 * ty, ix0, iy0, ix1, iy1)
        bx0, by0, bx1, by1 = max(ix0, 0), max(iy0, 0), min(ix1, w), min(iy1, h)
        bw, ba = case.box_width, case.box_alpha256
        for y in range(by0, by1):
            for x in range(bx0, bx1):
                if x < bx0 + bw or x >= bx1 - bw or y < by0 + bw or y >= by1 - bw:
                    pic[y][x] = [(c * (256 - ba) + colors[i][k] * ba + 128) >> 8 for k, c in enumerate(pic[y][x])]
        m = masks[i]
        for y in range(h):
            for x in range(w):
                if not m[y, x]:
                    continue
                edge = any(0 <= yy < h and 0 <= xx < w and not m[yy, xx] for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)))
                pic[y][x] = list(edges[i]) if edge else [(c * 128 + colors[i][k] * 128 + 128) >> 8 for k, c in enumerate(pic[y][x])]
    return order, anchors, np.array(pic, np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_twins_equal_a_per_pixel_loop(name):
    case = CASES[name]
    order, anchors, pic = loop_reference(case)
    assert case.order().tolist() == order
    assert [tuple(int(v) for v in r) for r in case.anchors()] == anchors
    assert case.overlay().tobytes() == pic.tobytes()


def test_equal_boxes_are_drawn_in_index_order_and_rectangles_in_mask_order():
    case = CASES["n100"]
    assert 0 <= case.order()[17] < case.order()[41]
    for name in RECTS:
        c = CASES[name]
        assert np.array_equal(V.instance_order(c.masks, None, 0.0), c.order()) and c.order()[1] + 1 == c.order()[4] and c.order()[5] == -1


def test_the_cases_hold_what_they_are_meant_to():
    assert {c.hw for c in CASES.values()} >= {(1, 1), (64, 64), (70, 45), (130, 33), (200, 37)}
    assert {c.count() for c in CASES.values()} >= {0, 1, 100} and {c.box_width for c in CASES.values()} >= {1, 3, 1 << 30}
    assert {c.box_alpha256 for c in CASES.values()} == {0, 128, 256}
    lab = CASES["labels"].anchors()
    pos = [(int(r["x2"]) // 2, int(r["y2"]) // 2) for r in lab]
    #       the corner   39 high     area < 1000  reaches the end  (86..125: 39 high, y1 = 125)  y1 = 124.5    10 x 25: small, 125   124.75
    assert pos == [(10, 10), (10, 49), (10, 50), (10, 90), (140, 86), (10, 124), (20, 100), (10, 124)]
    fr = CASES["frames"]
    assert fr.order().tolist()[5] == -1 and fr.order()[6] + 1 == fr.order()[7]                 # no width: not kept; equal areas: by index
    out, img = fr.overlay(), fr.image()
    assert (out[70:120, 100:148] != img[70:120, 100:148]).any() and not fr.masks[:, 64:, 64:].any()   # a frame in tiles no mask touches
    assert (out[10:60, 70:74] != img[10:60, 70:74]).all(axis=2).mean() > 0.9                    # 4 wide, frame 3: all frame
    nf = CASES["non_finite"]
    assert nf.order()[:3].tolist() == [-1, -1, -1] and (nf.order()[3:5] >= 0).all()


def test_hand_worked_pictures():
    for hc in BX.hand_cases():
        a = V.instance_anchors_boxes(hc["masks"], hc["boxes"], hc["scores"], hc["min_score"], None, hc["small_area"])
        assert [tuple(int(v) for v in r) for r in a] == hc["anchors"]
        assert V.instance_order_boxes(hc["masks"], hc["boxes"], hc["scores"], hc["min_score"]).tolist() == hc["order"]
        pic = V.instance_overlay_boxes(hc["image"], hc["masks"], hc["boxes"], hc["colors"], hc["edge_colors"], hc["alpha256"], hc["scores"], hc["min_score"],
                                       hc["box_width"], hc["box_alpha256"])
        assert pic.tolist() == [[list(p) for p in row] for row in hc["picture"]]


def test_default_box_width_and_the_picture_call():
    assert [V.default_box_width(h, w) for h, w in ((1, 1), (480, 640), (1024, 1024), (1280, 1280), (2560, 2560))] == [2, 2, 3, 4, 7]
    case = CASES["loose_70x45"]
    n = case.count()
    classes = np.arange(n) % 3
    md = {"thing_classes": ["a", "b", "c"], "thing_colors": [(250, 10, 10), (10, 250, 10), (10, 10, 250)]}
    got = V.draw_instance_predictions(case.image(), case.masks[:n], classes, case.live_scores(), md, 128, case.min_score, boxes=case.boxes[:n])
    plain = V.draw_instance_predictions(case.image(), case.masks[:n], classes, case.live_scores(), md, 128, case.min_score)
    assert got.shape == plain.shape == case.hw + (3,) and got.dtype == np.uint8 and (got != plain).any()
    colors = V.instance_colors(classes, md)
    bare = V.instance_overlay_boxes(case.image(), case.masks[:n], case.boxes[:n], colors, V.instance_edge_colors(colors), 128, case.live_scores(), case.min_score,
                                    V.default_box_width(*case.hw), 128)
    anchors = V.instance_anchors_boxes(case.masks[:n], case.boxes[:n], case.live_scores(), case.min_score)
    order = V.instance_order_boxes(case.masks[:n], case.boxes[:n], case.live_scores(), case.min_score)
    kept = sorted((i for i in range(n) if order[i] >= 0), key=lambda i: order[i])
    assert got.tobytes() == V.draw_texts(bare, anchors[kept], V.instance_texts(classes, case.live_scores(), md)).tobytes()
