"""GPU: odise_hip_instance_draw_boxes (csrc/vis_inst.hip, the box variant of the instance overlay) against the numpy restatement
odise_amd.visualize.instance_overlay_boxes / instance_anchors_boxes / instance_order_boxes on tests/vis_box_cases.py: integers and bytes,
every comparison exact; every call runs twice.  With box_alpha256 = 0 and a box order equal to the mask order the picture is
odise_hip_instance_draw's.  (HipVideoVisualizer.draw_instance_predictions(boxes=True) is held to its host twin on the three-frame sequence
of tests/test_gpu_box_track.py, which shares that sequence's forward passes.)"""
import ctypes as C

import numpy as np
import pytest

import vis_box_cases as BX
from odise_amd import visualize as V
from odise_amd._lib import U8, InstBoxDraw, InstDrawDesc

pytestmark = pytest.mark.gpu

CASES = BX.cases()
GUARD = 3


def device_draw(ctx, case, want=("out", "anchors", "order"), in_place=False, misalign=0, dtype=np.uint8, boxes=True, box_alpha256=None):
    """Twice -> {"out": [h,w,3], "anchors": [topk], "order": [topk]} of the outputs asked for (boxes=False: odise_hip_instance_draw)."""
    h, w = case.hw
    topk = case.topk
    image = case.image()
    masks = ctx.to_device(case.masks.astype(dtype) * (3 if dtype == np.float32 else 1))
    table = None if case.table() is None else ctx.to_device(case.table())
    scores = None if case.scores is None else ctx.to_device(case.scores)
    colors, edges, bx = ctx.to_device(case.colors()), ctx.to_device(case.edge_colors()), ctx.to_device(np.ascontiguousarray(case.boxes, np.float32))
    runs = []
    for _ in range(2):
        src = ctx.to_device(np.concatenate([np.full(misalign, 9, np.uint8), image.reshape(-1)]))
        dst = src if in_place else ctx.to_device(np.full(misalign + image.size + 5, 77, np.uint8))
        rows = np.zeros(topk + GUARD, V.ANCHOR_DTYPE)
        rows["segment_row"], rows["area"] = -5, -6
        anchors, order = ctx.to_device(rows), ctx.to_device(np.full(topk + GUARD, -9, np.int32))
        kw = dict(table_row=table, scores_row=scores, masks=masks, min_score=case.min_score, image=src.view((h, w, 3), np.uint8, misalign), colors=colors,
                  edge_colors=edges, alpha256=128, want=want, out=dst.view((h, w, 3), np.uint8, misalign), anchors=anchors, order=order)
        if boxes:
            ctx.instance_draw_boxes((h, w), topk, bx, case.box_width, case.box_alpha256 if box_alpha256 is None else box_alpha256, case.small_area, **kw)
        else:
            ctx.instance_draw((h, w), topk, **kw)
        got = {"out": dst.numpy(), "anchors": anchors.numpy(), "order": order.numpy()}
        if "out" in want:
            assert (got["out"][:misalign] == (9 if in_place else 77)).all()
            if not in_place:
                assert (got["out"][misalign + image.size:] == 77).all(), "bytes behind the picture were written"
        if "anchors" in want:
            assert got["anchors"][topk:].tobytes() == rows[topk:].tobytes(), "rows behind topk were written"
        if "order" in want:
            assert (got["order"][topk:] == -9).all(), "entries behind topk were written"
        runs.append(got)
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), f"{k}: the second run differs from the first"
    g = runs[0]
    return {"out": g["out"][misalign:misalign + image.size].reshape(h, w, 3), "anchors": g["anchors"][:topk], "order": g["order"][:topk]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_box_variant_equals_the_restatement(ctx, name):
    case = CASES[name]
    got = device_draw(ctx, case, dtype=np.float32 if len(name) % 2 else np.uint8)
    print(name, case.hw, "kept", int((case.order() >= 0).sum()), "differing pixels", int((got["out"] != case.overlay()).any(axis=2).sum()),
          "anchor rows differing", int((got["anchors"] != case.anchors()).sum()))
    assert got["order"].tobytes() == case.order().tobytes()
    assert got["anchors"].tobytes() == case.anchors().tobytes()
    assert got["out"].tobytes() == case.overlay().tobytes()


@pytest.mark.parametrize("in_place,misalign", [(True, 0), (False, 1), (True, 2), (False, 3), (True, 3)])
def test_misaligned_and_in_place_pictures(ctx, in_place, misalign):
    for name in ("loose_70x45", "frames", "n100"):
        case = CASES[name]
        got = device_draw(ctx, case, ("out",), in_place, misalign)
        assert got["out"].tobytes() == case.overlay().tobytes(), name


@pytest.mark.parametrize("name", ["rects_64x64", "rects_70x45", "rects_130x33", "rects_200x37", "one_pixel", "n0"])
def test_without_a_frame_and_in_mask_order_it_is_the_plain_instance_draw(ctx, name):
    """Filled rectangles with their tight boxes order as their masks do, so with box_alpha256 = 0 only the mask step is left."""
    case = CASES[name]
    n = case.count()
    assert np.array_equal(V.instance_order(case.masks[:n], case.live_scores(), case.min_score, case.topk), case.order())
    with_boxes = device_draw(ctx, case, ("out", "order"), box_alpha256=0)
    plain = device_draw(ctx, case, ("out", "order"), boxes=False)
    assert with_boxes["out"].tobytes() == plain["out"].tobytes() and with_boxes["order"].tobytes() == plain["order"].tobytes()


def test_hand_worked_pictures_on_the_device(ctx):
    for hc in BX.hand_cases():
        m = hc["masks"]
        case = BX.BoxCase("hand", m, hc["boxes"], hc["scores"], hc["min_score"], None, hc["box_width"], hc["box_alpha256"], hc["small_area"])
        case.image = lambda hc=hc: hc["image"]
        case.colors = lambda hc=hc: np.array(hc["colors"], np.uint8)
        case.edge_colors = lambda hc=hc: np.array(hc["edge_colors"], np.uint8)
        h, w = case.hw
        topk = case.topk
        masks, bx = ctx.to_device(m.astype(np.uint8)), ctx.to_device(hc["boxes"])
        scores = None if hc["scores"] is None else ctx.to_device(hc["scores"])
        res = ctx.instance_draw_boxes((h, w), topk, bx, hc["box_width"], hc["box_alpha256"], hc["small_area"], scores_row=scores, masks=masks,
                                      min_score=hc["min_score"], image=ctx.to_device(hc["image"]), colors=ctx.to_device(case.colors()),
                                      edge_colors=ctx.to_device(case.edge_colors()), alpha256=hc["alpha256"])
        assert [tuple(int(v) for v in r) for r in res["anchors"].numpy()] == hc["anchors"]
        assert res["order"].numpy().tolist() == hc["order"]
        assert res["out"].numpy().tolist() == [[list(p) for p in row] for row in hc["picture"]]


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    lib, case = ctx.lib, CASES["loose_70x45"]
    (h, w), topk = case.hw, case.topk
    masks, table, scores = ctx.to_device(case.masks.astype(np.uint8)), ctx.to_device(case.table()), ctx.to_device(case.scores)
    image, colors, edges, bxs = ctx.to_device(case.image()), ctx.to_device(case.colors()), ctx.to_device(case.edge_colors()), ctx.to_device(case.boxes)
    out = ctx.to_device(np.full((h, w, 3), 55, np.uint8))
    d = InstDrawDesc()
    d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk, d.min_score = h, w, masks.ptr, U8, table.ptr, scores.ptr, topk, case.min_score
    d.image, d.colors, d.edge_colors, d.alpha256, d.out = image.ptr, colors.ptr, edges.ptr, 128, out.ptr

    def bx(**kw):
        b = InstBoxDraw()
        b.boxes, b.box_width, b.box_alpha256, b.small_area = bxs.ptr, 1, 128, 1000
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    for b in (bx(boxes=None), bx(boxes=bxs.ptr + 2), bx(box_width=0), bx(box_width=-3), bx(box_alpha256=-1), bx(box_alpha256=257)):
        assert lib.odise_hip_instance_draw_boxes(ctx.h, C.byref(d), C.byref(b)) == -1
        assert lib.odise_hip_last_error()
    assert lib.odise_hip_instance_draw_boxes(ctx.h, C.byref(d), None) == -1 and lib.odise_hip_instance_draw_boxes(ctx.h, None, C.byref(bx())) == -1
    d.alpha256 = 300                                              # and what odise_hip_instance_draw refuses
    assert lib.odise_hip_instance_draw_boxes(ctx.h, C.byref(d), C.byref(bx())) == -1
    ctx.sync()
    assert (out.numpy() == 55).all()
    d.alpha256 = 128
    assert lib.odise_hip_instance_draw_boxes(ctx.h, C.byref(d), C.byref(bx(box_width=case.box_width, box_alpha256=case.box_alpha256, small_area=case.small_area))) == 0
    assert out.numpy().tobytes() == case.overlay().tobytes()
