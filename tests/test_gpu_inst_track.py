"""GPU: odise_hip_inst_track_create / _frame / _reset / _destroy (csrc/inst_track.hip) against the numpy restatement
odise_amd.video.InstanceColorTracker on the sequences of tests/inst_track_cases.py, frame by frame.  Everything is integers, bytes and one
double division of two exact integers: all comparisons are exact.  Every sequence runs twice (the second time after a reset) and must give
the same bytes."""
import ctypes as C

import numpy as np
import pytest

import inst_track_cases as IC
from odise_amd import coco_rle
from odise_amd import video as VD
from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS, U8, InstTrackDesc

pytestmark = pytest.mark.gpu

CASES = IC.cases()
GUARD = 3                  # rows behind live_cap / iou_cap / topk that must stay as they were


def live_guard(cap):
    g = np.zeros(cap + GUARD, VD.TRACK_ROW_DTYPE)
    g["frame"], g["rgb"], g["pad1"] = -5, -6, -8
    return g


def edge_prefill(topk):
    return (IC.prefill(topk + GUARD) ^ 0x55).astype(np.uint8)


def run_sequence(ctx, case, tracker, dtype=np.uint8, live_cap=None):
    """Every frame checked against the restatement -> the bytes the device wrote, per frame."""
    got, topk = [], case.topk
    for t, want in enumerate(IC.expected(case)):
        dense, table, scores = IC.device_frame(case, t, dtype)
        colors, edges = ctx.to_device(IC.prefill(topk + GUARD)), ctx.to_device(edge_prefill(topk))
        cap = len(want["live"]) if live_cap is None else live_cap
        live, n_live = ctx.to_device(live_guard(cap)), ctx.to_device(np.full(1, -9, np.int32))
        iou_cap = want["n_before"]
        iou_fill = np.full((iou_cap + GUARD, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)
        ctx.inst_track_frame(tracker, ctx.to_device(table), ctx.to_device(scores), masks=ctx.to_device(dense), min_score=case.min_score, colors=colors,
                             edge_colors=edges, live=live, n_live=n_live, iou=iou, live_cap=cap, iou_cap=iou_cap)
        c, e, l, n, u = colors.numpy(), edges.numpy(), live.numpy(), int(n_live.numpy()[0]), iou.numpy()
        want_c = IC.prefill(topk + GUARD)
        want_c[:topk] = want["colors"]
        written = (want_c != IC.prefill(topk + GUARD)).any(axis=1) | np.isin(np.arange(topk + GUARD), want["live"]["id"][want["live"]["frame"] == t])
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
    assert 8 <= len(case.frames) <= 12
    trk = ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool)
    try:
        first = run_sequence(ctx, case, trk, np.float32 if len(name) % 2 else np.uint8)
        trk.reset()
        assert run_sequence(ctx, case, trk, np.uint8 if len(name) % 2 else np.float32) == first, "not the first run again after a reset"
    finally:
        trk.close()


def test_the_cases_cover_the_sizes_and_limits_they_are_meant_to():
    sizes = {(c.hw, c.topk, c.ttl) for c in CASES.values()}
    assert {hw for hw, _, _ in sizes} == {(1, 1), (64, 64), (70, 45), (130, 33), (200, 37)}
    assert {k for _, k, _ in sizes} == {1, 7, 100} and {t for _, _, t in sizes} == {1, 3, 8}
    assert ((200, 37), 100, 8) in sizes
    assert max(len(e["live"]) for e in IC.expected(CASES["cap"])) == 8 * MAX_SEGMENTS
    assert any(e["n_before"] > 64 and e["iou"].shape[1] > 32 and e["iou"].any() for e in IC.expected(CASES["random_hundred"]))   # several tiles, matched


def test_two_trackers_do_not_share_state(ctx):
    case = CASES["random_ragged"]
    a, b = ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool), ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool)
    try:
        assert run_sequence(ctx, case, a) == run_sequence(ctx, case, b)
    finally:
        a.close()
        b.close()


def test_a_short_live_cap_clips_the_dump_not_the_count(ctx):
    case = CASES["two_claim"]
    trk = ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool)
    try:
        run_sequence(ctx, case, trk, live_cap=1)
        trk.reset()
        run_sequence(ctx, case, trk, live_cap=0)
    finally:
        trk.close()


def test_frames_without_the_optional_arguments(ctx):
    """No table (n = topk, every class 0), no scores, no dumps, colours allocated by the binding."""
    case = CASES["overlap_one_class"]
    trk, host = ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool), VD.InstanceColorTracker(case.ttl, case.pool)
    try:
        for classes, scores, masks in case.frames[:4]:
            colors = ctx.inst_track_frame(trk, masks=ctx.to_device(masks.astype(np.uint8)))
            want = host.assign(np.zeros(len(masks), np.int32), None, masks, 0.0)
            assert colors.numpy().tobytes() == want.tobytes()
    finally:
        trk.close()


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    lib, case = ctx.lib, CASES["two_claim"]
    (h, w), topk = case.hw, case.topk
    pool = np.ascontiguousarray(case.pool)
    pp = pool.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    ref = C.byref(out)
    for H, W, k, ttl, p, n_pool, o in ((0, 8, 7, 8, pp, 3, ref), (8, 0, 7, 8, pp, 3, ref), (-1, 8, 7, 8, pp, 3, ref), (1 << 15, 1 << 14, 7, 8, pp, 3, ref),
                                       (8, 8, 0, 8, pp, 3, ref), (8, 8, 101, 8, pp, 3, ref), (8, 8, 7, 0, pp, 3, ref), (8, 8, 7, 9, pp, 3, ref),
                                       (8, 8, 7, 8, pp, 0, ref), (8, 8, 7, 8, pp, (1 << 20) + 1, ref), (8, 8, 7, 8, None, 3, ref), (8, 8, 7, 8, pp, 3, None)):
        assert lib.odise_hip_inst_track_create(ctx.h, H, W, k, ttl, p, n_pool, o) == -1, (H, W, k, ttl, n_pool)
        assert out.value is None
    assert lib.odise_hip_inst_track_create(None, 8, 8, 7, 8, pp, 3, ref) == -1
    assert lib.odise_hip_inst_track_reset(ctx.h, None) == -1 and lib.odise_hip_inst_track_destroy(ctx.h, None) == -1
    assert lib.odise_hip_inst_track_frame(ctx.h, None) == -1

    trk = ctx.inst_track_create(case.hw, topk, case.ttl, case.pool)
    try:
        dense, table, scores = IC.device_frame(case, 0)
        masks, table, scores = ctx.to_device(dense), ctx.to_device(table), ctx.to_device(scores)
        colors, edges = ctx.to_device(IC.prefill(topk)), ctx.to_device(edge_prefill(topk))
        live, n_live = ctx.to_device(live_guard(4)), ctx.to_device(np.full(1, -9, np.int32))
        iou_fill = np.full((4, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)

        def desc(**kw):
            d = InstTrackDesc()
            d.track, d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk, d.min_score = trk.handle, h, w, masks.ptr, U8, table.ptr, scores.ptr, topk, 0.5
            d.colors, d.edge_colors, d.live, d.live_cap, d.n_live, d.iou, d.iou_cap = colors.ptr, edges.ptr, live.ptr, 4, n_live.ptr, iou.ptr, 4
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        bad = [desc(track=None), desc(colors=None), desc(h=0), desc(w=-2), desc(h=h + 1), desc(w=w - 1), desc(h=h // 2, w=w * 2), desc(h=1 << 15, w=1 << 14),
               desc(topk=topk - 1), desc(topk=topk + 1), desc(topk=0), desc(topk=101), desc(dtype=7), desc(live_cap=-1), desc(iou_cap=-1),
               desc(n_live=None),                                                       # live without n_live
               desc(masks=None, inst_table=None), desc(masks=None, inst_scores=None)]   # the logits route needs both
        for d in bad:
            assert lib.odise_hip_inst_track_frame(ctx.h, C.byref(d)) == -1
            assert lib.odise_hip_last_error()
        # the geometry errors of odise_hip_instance_rle are pinned where there are mask logits (the `clip` fixture); refused here either way
        assert lib.odise_hip_inst_track_frame(ctx.h, C.byref(desc(masks=None, pad_h=-4, pad_w=-4, img_h=h, img_w=w))) != 0
        ctx.sync()
        assert colors.numpy().tobytes() == IC.prefill(topk).tobytes() and edges.numpy().tobytes() == edge_prefill(topk).tobytes()
        assert live.numpy().tobytes() == live_guard(4).tobytes() and int(n_live.numpy()[0]) == -9 and iou.numpy().tobytes() == iou_fill.tobytes()
        run_sequence(ctx, case, trk)                                                    # and the tracker is where it was: empty, at frame 0
    finally:
        trk.close()
    with pytest.raises(RuntimeError):
        ctx.inst_track_create((8, 8), 7, ttl=9)


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_masks_of_an_unsupported_dtype_raise_and_write_nothing(ctx, dtype):
    """The smallest legal call but for the dtype of its masks: refused by the binding, before the library is called; the tracker stays at
    frame 0 (the sequence of the 1 x 1 case runs as on a fresh one)."""
    case = CASES["one_pixel"]
    assert case.hw == (1, 1) and case.topk == 1
    trk = ctx.inst_track_create(case.hw, case.topk, case.ttl, case.pool)
    try:
        colors, edges = ctx.to_device(IC.prefill(1)), ctx.to_device(edge_prefill(1))
        live, n_live = ctx.to_device(live_guard(1)), ctx.to_device(np.full(1, -9, np.int32))
        with pytest.raises(ValueError, match="dtype"):
            ctx.inst_track_frame(trk, masks=ctx.to_device(np.ones((1, 1, 1), dtype)), colors=colors, edge_colors=edges, live=live, n_live=n_live)
        ctx.sync()
        assert colors.numpy().tobytes() == IC.prefill(1).tobytes() and edges.numpy().tobytes() == edge_prefill(1).tobytes()
        assert live.numpy().tobytes() == live_guard(1).tobytes() and int(n_live.numpy()[0]) == -9
        run_sequence(ctx, case, trk)
    finally:
        trk.close()


# ---- the selection of the last head forward (masks sampled from the mask logits) ------------------------------------------------------------
@pytest.fixture(scope="module")
def clip(ctx):
    """Three frames through the narrow model (frames 0 and 1 are the same picture, frame 2 another one).  Per frame, while its selection
    is the one of the last head forward: the tracker fed from the mask logits, a second tracker fed with the dense masks of
    odise_hip_instance_masks, and HipVideoVisualizer.draw_instance_predictions; with what the host twins need."""
    from small_model import GROUPS, build_small, image_u8
    hip = build_small(ctx, panoptic_on=False)
    h, w = 250, 251                                                  # the generic sampler: ragged, resized from 512 x 512
    names = [f"class {c}" for c in range(len(GROUPS))]
    md = {"stuff_classes": names, "thing_classes": names, "stuff_colors": [(10 * c, 255 - 20 * c, 40 + c) for c in range(len(GROUPS))],
          "thing_colors": [(255 - 9 * c, 30 + c, 11 * c) for c in range(len(GROUPS))]}
    vis = V.HipVideoVisualizer(ctx, md, ttl=3, alpha=0.5)
    frames, a, b = [], None, None
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
            if a is None:
                a, b = ctx.inst_track_create((h, w), topk, 3), ctx.inst_track_create((h, w), topk, 3)
            dumps = []
            for trk, dense in ((a, False), (b, True)):
                colors, edges = ctx.to_device(IC.prefill(topk)), ctx.to_device(edge_prefill(topk)[:topk])
                live, n_live = ctx.to_device(live_guard(8 * MAX_SEGMENTS)), ctx.to_device(np.full(1, -9, np.int32))
                iou = ctx.to_device(np.full((8 * MAX_SEGMENTS, MAX_SEGMENTS), -7.0, np.float64))
                masks = None
                if dense:
                    masks = ctx.zeros((topk, h, w), np.float32)
                    rc = ctx.lib.odise_hip_instance_masks(ctx.h, 0, C.c_void_p(table.ptr + 4), n, sel["pad_hw"][0], sel["pad_hw"][1], sel["img_hw"][0][0],
                                                          sel["img_hw"][0][1], h, w, C.c_void_p(masks.ptr))
                    assert rc == 0
                ctx.inst_track_frame(trk, table, scores, masks=masks, b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0], min_score=min_score, colors=colors,
                                     edge_colors=edges, live=live, n_live=n_live, iou=iou)
                dumps.append((colors.numpy(), edges.numpy(), live.numpy(), int(n_live.numpy()[0]), iou.numpy()))
            image = np.ascontiguousarray(np.ascontiguousarray(big.numpy())[:, :2 * h:2, :2 * w:2].transpose(1, 2, 0))
            picture = vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk, sel["pad_hw"], sel["img_hw"][0], (h, w), min_score)
            frames.append(dict(dumps=dumps, picture=picture, image=image, min_score=min_score, topk=topk, classes=np.asarray(inst["pred_classes"]),
                               scores=np.asarray(inst["scores"], np.float32), masks=np.stack([coco_rle.decode(r) for r in inst["pred_masks_rle"]]).astype(bool)))
        # the geometry errors of odise_hip_instance_rle, against the logits of the last forward: refused, nothing written, the tracker unchanged
        (ph, pw), (ih, iw) = sel["pad_hw"], sel["img_hw"][0]
        untouched = ctx.to_device(IC.prefill(topk))
        geometry = []
        for bb, p_h, p_w, i_h, i_w in ((-1, ph, pw, ih, iw), (1, ph, pw, ih, iw), (0, ph + 4, pw, ih, iw), (0, ph, pw - 4, ih, iw), (0, ph, pw, 0, iw),
                                       (0, ph, pw, ih, pw + 1)):
            d = InstTrackDesc()
            d.track, d.h, d.w, d.topk, d.min_score, d.inst_table, d.inst_scores, d.colors = a.handle, h, w, topk, min_score, table.ptr, scores.ptr, untouched.ptr
            d.b, d.pad_h, d.pad_w, d.img_h, d.img_w = bb, p_h, p_w, i_h, i_w
            geometry.append(ctx.lib.odise_hip_inst_track_frame(ctx.h, C.byref(d)))
        geometry.append(untouched.numpy().tobytes() == IC.prefill(topk).tobytes())
        with pytest.raises(ValueError):
            vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk, sel["pad_hw"], sel["img_hw"][0], (h - 1, w), min_score)
        with pytest.raises(ValueError):
            vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk - 1, sel["pad_hw"], sel["img_hw"][0], (h, w), min_score)
        vis.reset()
        again = vis.draw_instance_predictions(ctx.to_device(image), 0, table, scores, topk, sel["pad_hw"], sel["img_hw"][0], (h, w), min_score, labels=False)
    finally:
        hip.keep_instance_selection, hip.instance_rle = False, False
        vis.close()
        for t in (a, b):
            if t is not None:
                t.close()
    return dict(frames=frames, md=md, hw=(h, w), after_reset=again, geometry=geometry)


def test_the_logits_route_equals_the_dense_route_and_the_restatement(clip):
    host = VD.InstanceColorTracker(3)
    for t, f in enumerate(clip["frames"]):
        (c0, e0, l0, n0, u0), (c1, e1, l1, n1, u1) = f["dumps"]
        assert c0.tobytes() == c1.tobytes() and e0.tobytes() == e1.tobytes() and l0.tobytes() == l1.tobytes() and n0 == n1 and u0.tobytes() == u1.tobytes(), t
        topk, n_before = f["topk"], len(host.live)
        want = host.assign(f["classes"], f["scores"], f["masks"], f["min_score"], IC.prefill(topk))
        rows = host.live_rows()
        print("frame", t, "instances", host.last_iou.shape[1], "of", len(f["masks"]), "live", n0, "matched", int((host.last_iou > 0.5).any(axis=0).sum()))
        assert 0 < host.last_iou.shape[1] < len(f["masks"])
        assert c0.tobytes() == want.tobytes() and n0 == len(rows) and l0[:n0].tobytes() == rows.tobytes()
        assert l0[n0:].tobytes() == live_guard(8 * MAX_SEGMENTS)[n0:].tobytes()
        assert u0[:n_before, :host.last_iou.shape[1]].tobytes() == host.last_iou.tobytes()
    assert clip["frames"][1]["dumps"][0][0].tobytes() == clip["frames"][0]["dumps"][0][0].tobytes()      # the same picture again: every colour kept
    assert clip["geometry"] == [-1] * 6 + [True]                                                          # bad geometries: ODISE_ERR_ARG, nothing written


def test_the_video_visualizer_draws_what_its_host_twin_draws(clip):
    twin = VD.InstanceColorTracker(3)
    for t, f in enumerate(clip["frames"]):
        want = VD.draw_instance_predictions(f["image"], f["masks"], f["classes"], f["scores"], twin, clip["md"], 128, f["min_score"])
        got = f["picture"]
        print("frame", t, "bytes differing", int((got != want).sum()))
        assert got.dtype == np.uint8 and got.shape == clip["hw"] + (3,) and got.tobytes() == want.tobytes() and (got != f["image"]).any()
    f = clip["frames"][-1]
    want = VD.draw_instance_predictions(f["image"], f["masks"], f["classes"], f["scores"], VD.InstanceColorTracker(3), clip["md"], 128, f["min_score"], labels=False)
    assert clip["after_reset"].tobytes() == want.tobytes()
