"""GPU: odise_hip_instance_draw / odise_hip_semantic_record (csrc/vis_inst.hip) against the numpy restatement odise_amd.visualize on
the case set of tests/vis_inst_cases.py.  Everything is integers and bytes: all comparisons are exact, and every call is made twice and
must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

from odise_amd import coco_rle
from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS, U8, InstDrawDesc
from record_helpers import upload_record
from vis_inst_cases import cases, hand_cases, sem_cases

pytestmark = pytest.mark.gpu

CASES = cases()
SEM = sem_cases()
GUARD = 2          # anchor rows / order entries behind topk that must stay as they were


def device_draw(ctx, case, alpha256=128, want=("out", "anchors", "order"), in_place=False, misalign=0, dtype=np.uint8):
    """Route B, twice -> {"out": [h,w,3], "anchors": [topk], "order": [topk]} of the outputs asked for."""
    h, w = case.hw
    topk = case.topk
    masks = ctx.to_device(case.masks.astype(dtype))
    table = ctx.to_device(case.table()) if case.n is not None else None
    scores = ctx.to_device(case.scores) if case.scores is not None else None
    image, colors, edges = case.image(), ctx.to_device(case.colors()), ctx.to_device(case.edge_colors())
    runs = []
    for _ in range(2):
        src = ctx.to_device(np.concatenate([np.full(misalign, 9, np.uint8), image.reshape(-1)]))
        dst = src if in_place else ctx.to_device(np.full(misalign + image.size + 5, 77, np.uint8))
        rows = np.zeros(topk + GUARD, V.ANCHOR_DTYPE)
        rows["segment_row"], rows["area"] = -5, -6
        anchors, order = ctx.to_device(rows), ctx.to_device(np.full(topk + GUARD, -9, np.int32))
        ctx.instance_draw((h, w), topk, table, scores, masks=masks, min_score=case.min_score, image=src.view((h, w, 3), np.uint8, misalign),
                          colors=colors, edge_colors=edges, alpha256=alpha256, want=want, out=dst.view((h, w, 3), np.uint8, misalign),
                          anchors=anchors, order=order)
        got = {"out": dst.numpy(), "anchors": anchors.numpy(), "order": order.numpy()}
        if "out" in want:
            assert (got["out"][:misalign] == (9 if in_place else 77)).all()
            if not in_place:
                assert (got["out"][misalign + image.size:] == 77).all(), "bytes behind the picture were written"
        elif not in_place:
            assert (got["out"] == 77).all(), "a picture that was not asked for was written"
        if "anchors" in want:
            assert got["anchors"][topk:].tobytes() == rows[topk:].tobytes(), "rows behind topk were written"
        else:
            assert got["anchors"].tobytes() == rows.tobytes()
        assert (got["order"][topk:] == -9).all() and ("order" in want or (got["order"] == -9).all())
        runs.append(got)
    for k in want:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), f"{k}: not the same from run to run"
    g = runs[0]
    return {"out": g["out"][misalign:misalign + image.size].reshape(h, w, 3), "anchors": g["anchors"][:topk], "order": g["order"][:topk]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_route_b_equals_the_restatement(ctx, name):
    case = CASES[name]
    got = device_draw(ctx, case, dtype=np.float32 if len(name) % 2 else np.uint8)
    print(name, case.hw, "kept", int((case.order() >= 0).sum()), "differing pixels", int((got["out"] != case.overlay()).any(axis=2).sum()))
    assert got["anchors"].tobytes() == case.anchors().tobytes()
    assert got["order"].tobytes() == case.order().tobytes()
    assert got["out"].tobytes() == case.overlay().tobytes()


@pytest.mark.parametrize("name", ["size_65x67", "n100_overlap", "special", "n0"])
def test_outputs_asked_for_singly_equal_those_asked_for_together(ctx, name):
    case = CASES[name]
    for k, ref in (("out", case.overlay()), ("anchors", case.anchors()), ("order", case.order())):
        assert device_draw(ctx, case, want=(k,))[k].tobytes() == ref.tobytes(), k


@pytest.mark.parametrize("alpha256", [0, 256])
@pytest.mark.parametrize("in_place,misalign", [(True, 0), (False, 1), (True, 2), (False, 3), (True, 3)])
def test_overlay_options(ctx, alpha256, in_place, misalign):
    for name in ("size_65x67", "special", "size_130x3"):
        case = CASES[name]
        got = device_draw(ctx, case, alpha256, ("out",), in_place, misalign)
        assert got["out"].tobytes() == case.overlay(alpha256).tobytes(), name


def test_hand_worked_pictures_on_the_device(ctx):
    for hc in hand_cases():
        m = hc["masks"]
        topk, (h, w) = len(m), m.shape[1:]
        scores = ctx.to_device(hc["scores"]) if hc["scores"] is not None else None
        res = ctx.instance_draw((h, w), topk, None, scores, masks=ctx.to_device(m.astype(np.uint8)), min_score=hc["min_score"],
                                image=ctx.to_device(hc["image"]), colors=ctx.to_device(np.asarray(hc["colors"], np.uint8)),
                                edge_colors=ctx.to_device(np.asarray(hc["edge_colors"], np.uint8)), alpha256=hc["alpha256"])
        assert [tuple(int(v) for v in a) for a in res["anchors"].numpy()] == hc["anchors"]
        assert list(res["order"].numpy()) == hc["order"]
        assert res["out"].numpy().tolist() == [[list(p) for p in row] for row in hc["picture"]]


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    case = CASES["min_score_equal"]
    (h, w), topk = case.hw, case.topk
    masks, table, scores = ctx.to_device(case.masks.astype(np.uint8)), ctx.to_device(case.table()), ctx.to_device(case.scores)
    image = ctx.to_device(np.concatenate([case.image().reshape(-1), np.zeros(8, np.uint8)]))
    colors, edges = ctx.to_device(case.colors()), ctx.to_device(case.edge_colors())
    out = ctx.to_device(np.full((h, w, 3), 55, np.uint8))
    rows, order = ctx.to_device(np.full(8 * topk, -1, np.int32)), ctx.to_device(np.full(topk, -4, np.int32))
    lib = ctx.lib

    def desc(**kw):
        d = InstDrawDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk, d.min_score = h, w, masks.ptr, U8, table.ptr, scores.ptr, topk, 0.5
        d.image, d.colors, d.edge_colors, d.alpha256, d.out, d.anchors, d.order = image.ptr, colors.ptr, edges.ptr, 128, out.ptr, rows.ptr, order.ptr
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = [{"image": None}, {"colors": None}, {"edge_colors": None}, {"out": None, "anchors": None, "order": None}, {"h": 0}, {"w": -3},
           {"h": 1 << 15, "w": 1 << 14}, {"topk": 0}, {"topk": 101}, {"alpha256": -1}, {"alpha256": 257}, {"dtype": 7},
           {"out": image.ptr + 3}, {"out": image.ptr + 3 * h * w - 1},               # overlaps the image without being equal to it
           {"masks": None, "inst_table": None}, {"masks": None, "inst_scores": None}]    # the logits route needs both
    for kw in bad:
        assert lib.odise_hip_instance_draw(ctx.h, C.byref(desc(**kw))) == -1, kw
    assert lib.odise_hip_instance_draw(ctx.h, None) == -1
    record = ctx.to_device(np.full(h * w + 1 + 3 * MAX_SEGMENTS, -8, np.int32))
    labels, sem = ctx.to_device(np.zeros((h, w), np.int32)), ctx.to_device(np.zeros((2, h, w), np.float32))
    for args in ((None, None, 2, h, w, record.ptr), (labels.ptr, sem.ptr, 2, h, w, record.ptr), (labels.ptr, None, 2, h, w, None),
                 (labels.ptr, None, 0, h, w, record.ptr), (labels.ptr, None, 12289, h, w, record.ptr), (labels.ptr, None, 2, 0, w, record.ptr),
                 (labels.ptr, None, 2, 1 << 15, 1 << 14, record.ptr)):
        assert lib.odise_hip_semantic_record(ctx.h, *args) == -1, args
    ctx.sync()
    assert (out.numpy() == 55).all() and (rows.numpy() == -1).all() and (order.numpy() == -4).all() and (record.numpy() == -8).all()
    assert np.array_equal(image.numpy()[:h * w * 3], case.image().reshape(-1))
    assert lib.odise_hip_instance_draw(ctx.h, C.byref(desc())) == 0
    ctx.sync()
    assert order.numpy().tobytes() == case.order().tobytes() and out.numpy().tobytes() == case.overlay().tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_masks_of_an_unsupported_dtype_raise_and_write_nothing(ctx, dtype):
    """The smallest legal call but for the dtype of its masks: refused by the binding, before the library is called."""
    image, colors = ctx.to_device(np.full((1, 1, 3), 9, np.uint8)), ctx.to_device(np.full((1, 3), 200, np.uint8))
    out = ctx.to_device(np.full((1, 1, 3), 55, np.uint8))
    rows, order = ctx.to_device(np.full(8, -1, np.int32)), ctx.to_device(np.full(1, -4, np.int32))
    with pytest.raises(ValueError, match="dtype"):
        ctx.instance_draw((1, 1), 1, masks=ctx.to_device(np.ones((1, 1, 1), dtype)), image=image, colors=colors, edge_colors=colors, out=out,
                          anchors=rows, order=order)
    ctx.sync()
    assert (out.numpy() == 55).all() and (rows.numpy() == -1).all() and (order.numpy() == -4).all() and (image.numpy() == 9).all()


@pytest.mark.parametrize("name", sorted(SEM))
def test_semantic_record_from_labels_and_from_scores(ctx, name):
    case = SEM[name]
    labels = ctx.to_device(case.labels)
    first, second = ctx.semantic_record(labels, case.K).numpy(), ctx.semantic_record(labels, case.K).numpy()
    assert first.tobytes() == case.record().tobytes() and second.tobytes() == first.tobytes()
    sem = ctx.to_device(case.sem_seg())
    want = V.semantic_record(np.clip(case.labels, 0, case.K - 1), case.K)
    got = [ctx.semantic_record(sem).numpy() for _ in range(2)]
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == got[0].tobytes()
    # the record draws through the two existing calls as the restatement draws it
    h, w = case.hw
    _, ids, table = upload_record(ctx, case.record(), case.hw)
    n = int(case.record()[h * w])
    rows = case.record()[h * w + 1:h * w + 1 + 3 * n].reshape(n, 3)
    anchors, count = ctx.segment_anchors(ids, table, case.small_area, case.large_area, 256)
    ref = V.segment_anchors(case.record()[:h * w].reshape(h, w), rows, case.small_area, case.large_area)
    assert int(count.numpy()[0]) == len(ref) and anchors.numpy()[:min(len(ref), 256)].tobytes() == ref[:256].tobytes()


@pytest.fixture(scope="module")
def drawn(ctx):
    """One forward of the small model with the semantic and the instance head on: the selection stays on the device (route A), its masks
    come back as the RLE strings the segm evaluator scores, the semantic scores stay on the device."""
    from small_model import GROUPS, build_small, image_u8
    hip = build_small(ctx, panoptic_on=False)
    h, w = 250, 251                                                  # the generic sampler: ragged, resized from 512 x 512
    big = image_u8(512, 512, seed=5)
    hip.keep_instance_selection, hip.instance_rle = True, True
    try:
        res = hip.forward([{"image": big, "height": h, "width": w}], to_host=False)[0]
    finally:
        hip.keep_instance_selection, hip.instance_rle = False, False
    sel = hip.last_selection
    topk = sel["topk"]
    inst = res["instances"]
    masks = np.stack([coco_rle.decode(r) for r in inst["pred_masks_rle"]]).astype(bool)
    image = np.ascontiguousarray(np.ascontiguousarray(big.numpy())[:, :2 * h:2, :2 * w:2].transpose(1, 2, 0))
    names = [f"class {c}" for c in range(len(GROUPS))]
    md = {"stuff_classes": names, "thing_classes": names, "stuff_colors": [(10 * c, 255 - 20 * c, 40 + c) for c in range(len(GROUPS))],
          "thing_colors": [(255 - 9 * c, 30 + c, 11 * c) for c in range(len(GROUPS))]}
    return dict(hw=(h, w), topk=topk, sel=sel, table=sel["inst_table"].view((1 + 2 * topk,), np.int32), scores=sel["inst_scores"].view((topk,), np.float32),
                masks=masks, host_scores=inst["scores"], classes=inst["pred_classes"], image=image, sem=res["sem_seg"], K=len(GROUPS), md=md)


def test_route_a_draws_exactly_the_evaluated_pixels(ctx, drawn):
    d = drawn
    (h, w), topk, n = d["hw"], d["topk"], len(d["masks"])
    assert 6 < n <= topk and d["masks"].shape[1:] == (h, w) and d["masks"].any()
    min_score = float(np.sort(d["host_scores"])[n // 3])             # equal to one instance's score: a third is left out
    colors = np.random.default_rng(4).integers(0, 256, (topk, 3), dtype=np.uint8)
    edges = V.instance_edge_colors(colors)
    res = [ctx.instance_draw((h, w), topk, d["table"], d["scores"], b=0, pad_hw=d["sel"]["pad_hw"], img_hw=d["sel"]["img_hw"][0], min_score=min_score,
                             image=ctx.to_device(d["image"]), colors=ctx.to_device(colors), edge_colors=ctx.to_device(edges), alpha256=100)
           for _ in range(2)]
    got = [{k: v.numpy() for k, v in r.items()} for r in res]
    want_order = V.instance_order(d["masks"], d["host_scores"], min_score, topk)
    assert 0 < (want_order >= 0).sum() < n
    assert got[0]["anchors"].tobytes() == V.instance_anchors(d["masks"], d["host_scores"], min_score, topk).tobytes()
    assert got[0]["order"].tobytes() == want_order.tobytes()
    assert got[0]["out"].tobytes() == V.instance_overlay(d["image"], d["masks"], colors, edges, 100, d["host_scores"], min_score).tobytes()
    assert all(got[0][k].tobytes() == got[1][k].tobytes() for k in got[0])


def test_the_visualizer_equals_its_host_twins_on_the_small_model(ctx, drawn):
    d = drawn
    h, w = d["hw"]
    vis = V.HipVisualizer(ctx, d["md"], alpha=0.5, small_area=50, large_area=2000)
    image_dev = ctx.to_device(d["image"])
    sem_host = d["sem"].numpy()
    got = vis.draw_sem_seg(image_dev, d["sem"])
    want = V.draw_sem_seg(d["image"], sem_host, d["K"], d["md"], 128, (0, 0, 0), 50, 2000)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) and got.tobytes() == want.tobytes() and (got != d["image"]).any()
    amax = ctx.to_device(sem_host.argmax(0).astype(np.int32))
    assert vis.draw_sem_seg(image_dev, amax, d["K"]).tobytes() == want.tobytes()                    # the fused arg-max map draws the same
    min_score = float(np.median(d["host_scores"]))
    got = vis.draw_instance_predictions(image_dev, 0, d["table"], d["scores"], d["topk"], d["sel"]["pad_hw"], d["sel"]["img_hw"][0], (h, w), min_score)
    want = V.draw_instance_predictions(d["image"], d["masks"], d["classes"], d["host_scores"], d["md"], 128, min_score)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) and got.tobytes() == want.tobytes() and (got != d["image"]).any()
