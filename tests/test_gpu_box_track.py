"""GPU: odise_hip_box_track_create / _frame / _reset / _destroy (csrc/box_track.hip) against the numpy restatement
odise_amd.video.BoxColorTracker on the sequences of tests/box_track_cases.py, frame by frame: colours, edge colours, the live dump, n_live,
the float64 IoU matrix and the guard rows behind every buffer.  The IoU is a handful of double operations rounded one by one on both
sides: all comparisons are exact.  Every sequence runs twice (the second time after a reset) and must give the same bytes."""
import ctypes as C

import numpy as np
import pytest

import box_track_cases as BC
from odise_amd import instance_eval as IE
from odise_amd import video as VD
from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS, BoxTrackDesc

pytestmark = pytest.mark.gpu

CASES = BC.cases()
GUARD = 3                  # rows behind live_cap / iou_cap / topk that must stay as they were


def live_guard(cap):
    g = np.zeros(cap + GUARD, VD.TRACK_ROW_DTYPE)
    g["frame"], g["rgb"], g["pad1"] = -5, -6, -8
    return g


def edge_prefill(topk):
    return (BC.prefill(topk + GUARD) ^ 0x55).astype(np.uint8)


def run_sequence(ctx, case, tracker, live_cap=None):
    """Every frame checked against the restatement -> the bytes the device wrote, per frame."""
    got, topk = [], case.topk
    for t, want in enumerate(BC.expected(case)):
        boxes, table, scores = BC.device_frame(case, t)
        colors, edges = ctx.to_device(BC.prefill(topk + GUARD)), ctx.to_device(edge_prefill(topk))
        cap = len(want["live"]) if live_cap is None else live_cap
        live, n_live = ctx.to_device(live_guard(cap)), ctx.to_device(np.full(1, -9, np.int32))
        iou_cap = want["n_before"]
        iou_fill = np.full((iou_cap + GUARD, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)
        ctx.box_track_frame(tracker, ctx.to_device(boxes), ctx.to_device(table), ctx.to_device(scores), min_score=case.min_score, colors=colors,
                            edge_colors=edges, live=live, n_live=n_live, iou=iou, live_cap=cap, iou_cap=iou_cap)
        c, e, l, n, u = colors.numpy(), edges.numpy(), live.numpy(), int(n_live.numpy()[0]), iou.numpy()
        want_c = BC.prefill(topk + GUARD)
        want_c[:topk] = want["colors"]
        written = np.isin(np.arange(topk + GUARD), want["live"]["id"][want["live"]["frame"] == t])
        want_e = np.where(written[:, None], V.instance_edge_colors(want_c), edge_prefill(topk))
        want_iou = iou_fill.copy()
        want_iou[:iou_cap, :want["iou"].shape[1]] = want["iou"]
        want_live = live_guard(cap)
        want_live[:min(cap, len(want["live"]))] = want["live"][:cap]
        print(case.name, "frame", t, "n_live", n, "/", len(want["live"]), "colour bytes differing", int((c != want_c).sum()), "edge bytes differing",
              int((e != want_e).sum()), "live rows differing", int((l != want_live).sum()), "iou cells differing", int((u != want_iou).sum()))
        assert c.tobytes() == want_c.tobytes(), (case.name, t, "colors")                   # other rows keep the caller's bytes
        assert e.tobytes() == want_e.tobytes(), (case.name, t, "edge colours")
        assert n == len(want["live"]), (case.name, t)
        assert l.tobytes() == want_live.tobytes(), (case.name, t, "live list / guard rows")
        assert u.tobytes() == want_iou.tobytes(), (case.name, t, "iou / guard rows")
        got.append((c.tobytes(), e.tobytes(), l.tobytes(), n, u.tobytes()))
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_sequence_matches_the_restatement_twice(ctx, name):
    case = CASES[name]
    trk = ctx.box_track_create(case.topk, case.ttl, case.pool)
    try:
        first = run_sequence(ctx, case, trk)
        trk.reset()
        assert run_sequence(ctx, case, trk) == first, "not the first run again after a reset"
    finally:
        trk.close()


def test_two_trackers_do_not_share_state(ctx):
    case = CASES["random_fractional"]
    a, b = ctx.box_track_create(case.topk, case.ttl, case.pool), ctx.box_track_create(case.topk, case.ttl, case.pool)
    try:
        assert run_sequence(ctx, case, a) == run_sequence(ctx, case, b)
    finally:
        a.close()
        b.close()


def test_a_short_live_cap_clips_the_dump_not_the_count(ctx):
    case = CASES["two_claim"]
    trk = ctx.box_track_create(case.topk, case.ttl, case.pool)
    try:
        run_sequence(ctx, case, trk, live_cap=1)
        trk.reset()
        run_sequence(ctx, case, trk, live_cap=0)
    finally:
        trk.close()


def test_frames_without_the_optional_arguments(ctx):
    """No table (n = topk, every class 0), no scores, no dumps, colours allocated by the binding."""
    case = CASES["moving"]
    trk, host = ctx.box_track_create(case.topk, case.ttl, case.pool), VD.BoxColorTracker(case.ttl, case.pool)
    try:
        for t in range(4):
            boxes, _, _ = BC.device_frame(case, t)
            colors = ctx.box_track_frame(trk, ctx.to_device(boxes))
            want = host.assign(np.zeros(case.topk, np.int32), None, boxes, 0.0)
            assert colors.numpy().tobytes() == want.tobytes()
    finally:
        trk.close()


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    lib, case = ctx.lib, CASES["two_claim"]
    topk = case.topk
    pool = np.ascontiguousarray(case.pool)
    pp = pool.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    ref = C.byref(out)
    for k, ttl, p, n_pool, o in ((0, 8, pp, 3, ref), (101, 8, pp, 3, ref), (7, 0, pp, 3, ref), (7, 9, pp, 3, ref), (7, 8, pp, 0, ref),
                                 (7, 8, pp, (1 << 20) + 1, ref), (7, 8, None, 3, ref), (7, 8, pp, 3, None)):
        assert lib.odise_hip_box_track_create(ctx.h, k, ttl, p, n_pool, o) == -1, (k, ttl, n_pool)
        assert out.value is None
    assert lib.odise_hip_box_track_create(None, 7, 8, pp, 3, ref) == -1
    assert lib.odise_hip_box_track_reset(ctx.h, None) == -1 and lib.odise_hip_box_track_destroy(ctx.h, None) == -1
    assert lib.odise_hip_box_track_frame(ctx.h, None) == -1

    trk = ctx.box_track_create(topk, case.ttl, case.pool)
    try:
        b, table, scores = BC.device_frame(case, 0)
        boxes, table, scores = ctx.to_device(b), ctx.to_device(table), ctx.to_device(scores)
        colors, edges = ctx.to_device(BC.prefill(topk)), ctx.to_device(edge_prefill(topk))
        live, n_live = ctx.to_device(live_guard(4)), ctx.to_device(np.full(1, -9, np.int32))
        iou_fill = np.full((4, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)

        def desc(**kw):
            d = BoxTrackDesc()
            d.track, d.boxes, d.inst_table, d.inst_scores, d.topk, d.min_score = trk.handle, boxes.ptr, table.ptr, scores.ptr, topk, 0.5
            d.colors, d.edge_colors, d.live, d.live_cap, d.n_live, d.iou, d.iou_cap = colors.ptr, edges.ptr, live.ptr, 4, n_live.ptr, iou.ptr, 4
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        bad = [desc(track=None), desc(boxes=None), desc(colors=None), desc(topk=topk - 1), desc(topk=topk + 1), desc(topk=0), desc(topk=101),
               desc(live_cap=-1), desc(iou_cap=-1), desc(n_live=None), desc(boxes=boxes.ptr + 2), desc(iou=iou.ptr + 4)]
        for d in bad:
            assert lib.odise_hip_box_track_frame(ctx.h, C.byref(d)) == -1
            assert lib.odise_hip_last_error()
        ctx.sync()
        assert colors.numpy().tobytes() == BC.prefill(topk).tobytes() and edges.numpy().tobytes() == edge_prefill(topk).tobytes()
        assert live.numpy().tobytes() == live_guard(4).tobytes() and int(n_live.numpy()[0]) == -9 and iou.numpy().tobytes() == iou_fill.tobytes()
        run_sequence(ctx, case, trk)                                                    # and the tracker is where it was: empty, at frame 0
    finally:
        trk.close()
    with pytest.raises(RuntimeError):
        ctx.box_track_create(7, ttl=9)


def test_the_dump_refusals_carry_the_entry_points_name(ctx):
    """live_cap -1, iou_cap -1 and live without n_live: the checks the three trackers share (track_match.h) answer as
    odise_hip_box_track_frame.  Nothing is launched and nothing is written."""
    topk = 7
    pool = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    trk = ctx.box_track_create(topk, 8, pool)
    try:
        boxes, colors = ctx.zeros((topk, 4), np.float32), ctx.to_device(BC.prefill(topk))
        live, n_live = ctx.to_device(live_guard(4)), ctx.to_device(np.full(1, -9, np.int32))
        iou_fill = np.full((4, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)
        for kw in (dict(live_cap=-1), dict(iou_cap=-1), dict(n_live=None)):
            d = BoxTrackDesc()
            d.track, d.boxes, d.topk, d.colors = trk.handle, boxes.ptr, topk, colors.ptr
            d.live, d.live_cap, d.n_live, d.iou, d.iou_cap = live.ptr, 4, n_live.ptr, iou.ptr, 4
            for k, v in kw.items():
                setattr(d, k, v)
            assert ctx.lib.odise_hip_box_track_frame(ctx.h, C.byref(d)) == -1, kw
            assert ctx.lib.odise_hip_last_error().decode().startswith("box_track_frame:"), (kw, ctx.lib.odise_hip_last_error())
        ctx.sync()
        assert colors.numpy().tobytes() == BC.prefill(topk).tobytes() and live.numpy().tobytes() == live_guard(4).tobytes()
        assert int(n_live.numpy()[0]) == -9 and iou.numpy().tobytes() == iou_fill.tobytes()
    finally:
        trk.close()


# ---- boxes straight from odise_hip_instance_boxes of the narrow model's mask logits ---------------------------------------------------------
@pytest.fixture(scope="module")
def clip(ctx):
    """Three frames through the narrow model (frames 0 and 1 are the same picture).  Per frame, while its selection is the one of the last
    head forward: odise_hip_instance_boxes from the logits -> the box tracker, nothing read back in between; and
    HipVideoVisualizer.draw_instance_predictions(boxes=True); with what the host twins need (the masks of odise_hip_instance_masks)."""
    from small_model import GROUPS, build_small, image_u8
    hip = build_small(ctx, panoptic_on=False)
    h, w = 250, 251
    names = [f"class {c}" for c in range(len(GROUPS))]
    md = {"stuff_classes": names, "thing_classes": names, "stuff_colors": [(10 * c, 255 - 20 * c, 40 + c) for c in range(len(GROUPS))],
          "thing_colors": [(255 - 9 * c, 30 + c, 11 * c) for c in range(len(GROUPS))]}
    vis = V.HipVideoVisualizer(ctx, md, ttl=3, alpha=0.5)
    frames, trk = [], None
    hip.keep_instance_selection, hip.instance_rle = True, True
    try:
        for seed in (5, 5, 6):
            big = image_u8(512, 512, seed=seed)
            res = hip.forward([{"image": big, "height": h, "width": w}], to_host=False)[0]
            sel = hip.last_selection
            topk = sel["topk"]
            table, scores = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)
            inst = res["instances"]
            n = len(inst["pred_masks_rle"])
            min_score = float(np.sort(inst["scores"])[n // 3])        # equal to one instance's score: a third is left out
            if trk is None:
                trk = ctx.box_track_create(topk, 3)
            colors, edges = ctx.to_device(BC.prefill(topk)), ctx.to_device(edge_prefill(topk)[:topk])
            live, n_live = ctx.to_device(live_guard(8 * MAX_SEGMENTS)), ctx.to_device(np.full(1, -9, np.int32))
            iou = ctx.to_device(np.full((8 * MAX_SEGMENTS, MAX_SEGMENTS), -7.0, np.float64))
            boxes = ctx.instance_boxes((h, w), topk, table, b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0])
            ctx.box_track_frame(trk, boxes, table, scores, min_score, colors, edges, live, n_live, iou)
            dump = (colors.numpy(), edges.numpy(), live.numpy(), int(n_live.numpy()[0]), iou.numpy(), boxes.numpy())
            masks = ctx.zeros((topk, h, w), np.float32)
            rc = ctx.lib.odise_hip_instance_masks(ctx.h, 0, C.c_void_p(table.ptr + 4), n, sel["pad_hw"][0], sel["pad_hw"][1], sel["img_hw"][0][0],
                                                  sel["img_hw"][0][1], h, w, C.c_void_p(masks.ptr))
            assert rc == 0
            image = np.ascontiguousarray(np.ascontiguousarray(big.numpy())[:, :2 * h:2, :2 * w:2].transpose(1, 2, 0))
            picture = vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk, sel["pad_hw"], sel["img_hw"][0], (h, w), min_score, boxes=True)
            frames.append(dict(dump=dump, picture=picture, image=image, min_score=min_score, topk=topk, classes=np.asarray(inst["pred_classes"]),
                               scores=np.asarray(inst["scores"], np.float32), masks=masks.numpy()[:n] != 0))
        vis.reset()
        again = vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk, sel["pad_hw"], sel["img_hw"][0], (h, w), min_score, labels=False,
                                              boxes=True, box_width=2, box_alpha256=256)
    finally:
        hip.keep_instance_selection, hip.instance_rle = False, False
        vis.close()
        if trk is not None:
            trk.close()
    return dict(frames=frames, md=md, hw=(h, w), after_reset=again)


def test_boxes_from_the_mask_logits_track_as_the_restatement_does(clip):
    host = VD.BoxColorTracker(3)
    for t, f in enumerate(clip["frames"]):
        c, e, l, n, u, boxes = f["dump"]
        topk, n_before, m = f["topk"], len(host.live), len(f["masks"])
        want_boxes = IE.mask_boxes(f["masks"])
        assert boxes[:m].tobytes() == want_boxes.tobytes() and not boxes[m:].any()
        want = host.assign(f["classes"], f["scores"], want_boxes, f["min_score"], BC.prefill(topk))
        rows = host.live_rows()
        print("frame", t, "instances", host.last_iou.shape[1], "of", m, "live", n, "matched", int((host.last_iou > 0.6).any(axis=0).sum()))
        assert 0 < host.last_iou.shape[1] < m
        assert c.tobytes() == want.tobytes() and n == len(rows) and l[:n].tobytes() == rows.tobytes()
        assert l[n:].tobytes() == live_guard(8 * MAX_SEGMENTS)[n:].tobytes()
        assert u[:n_before, :host.last_iou.shape[1]].tobytes() == host.last_iou.tobytes()
    # the same picture again: something is matched.  Not everything: the narrow model's masks share boxes, and of the live rows whose
    # first maximum is one and the same box only the earliest takes it (the rule, and what the restatement above gave as well)
    assert clip["frames"][1]["dump"][3] < 2 * clip["frames"][0]["dump"][3]


def test_the_video_visualizer_draws_boxes_as_its_host_twin_does(clip):
    twin = VD.BoxColorTracker(3)
    for t, f in enumerate(clip["frames"]):
        want = VD.draw_instance_predictions(f["image"], f["masks"], f["classes"], f["scores"], twin, clip["md"], 128, f["min_score"],
                                            boxes=IE.mask_boxes(f["masks"]))
        got = f["picture"]
        print("frame", t, "bytes differing", int((got != want).sum()))
        assert got.dtype == np.uint8 and got.shape == clip["hw"] + (3,) and got.tobytes() == want.tobytes() and (got != f["image"]).any()
    f = clip["frames"][-1]
    want = VD.draw_instance_predictions(f["image"], f["masks"], f["classes"], f["scores"], VD.BoxColorTracker(3), clip["md"], 128, f["min_score"], labels=False,
                                        boxes=IE.mask_boxes(f["masks"]), box_width=2, box_alpha256=256)
    assert clip["after_reset"].tobytes() == want.tobytes()
