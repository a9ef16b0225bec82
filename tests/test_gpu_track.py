"""GPU: odise_hip_track_create / _frame / _reset / _destroy (csrc/track.hip) against the numpy restatement odise_amd.video.ColorTracker on
the sequences of tests/track_cases.py, frame by frame.  Everything is integers, bytes and one double division of two exact integers: all
comparisons are exact.  Every sequence runs on two trackers and once more after a reset, and must give the same bytes each time."""
import ctypes as C

import numpy as np
import pytest

import track_cases as TC
from record_helpers import upload_record
from odise_amd import video as VD
from odise_amd import visualize as V
from odise_amd._lib import MAX_SEGMENTS, TrackDesc

pytestmark = pytest.mark.gpu

CASES = TC.cases()
GUARD = 3                  # rows behind live_cap / iou_cap that must stay as they were
LIVE_MAX = 8 * MAX_SEGMENTS
LDS_CELLS = 12288          # csrc/lds_hist.h kLdsHistCells


def record_of(ids, tab):
    rec = np.zeros(ids.size + 1 + 3 * MAX_SEGMENTS, np.int32)
    rec[:ids.size] = ids.reshape(-1)
    rec[ids.size] = len(tab)
    rec[ids.size + 1:ids.size + 1 + 3 * len(tab)] = tab.reshape(-1)
    return rec


def live_guard(cap):
    g = np.zeros(cap + GUARD, VD.TRACK_ROW_DTYPE)
    g["frame"], g["rgb"], g["pad1"] = -5, -6, -8
    return g


def histogram_cells(case):
    """per frame: the cells the pixel pass counts in - one (rows + 1) x (n + 1) matrix per retained frame that still has a live row (a
    single row of n + 1 when there is none), as csrc/track.hip lays them out"""
    out = []
    for t, (_, tab) in enumerate(case.frames):
        frames = sorted(set(TC.expected(case)[t - 1]["live"]["frame"].tolist())) if t else []
        assert all(t - 8 <= f < t for f in frames)
        out.append(sum((len(case.frames[f][1]) + 1) * (len(tab) + 1) for f in frames) if frames else len(tab) + 1)
    return out


def run_sequence(ctx, case, tracker, unaligned=False, clobber=False, live_cap=None):
    """Every frame checked against the restatement -> the bytes the device wrote, per frame."""
    got = []
    for t, ((ids, tab), want) in enumerate(zip(case.frames, TC.expected(case))):
        buf, ids_dev, table_dev = upload_record(ctx, record_of(ids, tab), ids.shape, unaligned)
        colors = ctx.to_device(TC.prefill())
        cap = len(want["live"]) if live_cap is None else live_cap
        live, n_live = ctx.to_device(live_guard(cap)), ctx.to_device(np.full(1, -9, np.int32))
        iou_cap = want["n_before"]
        iou_fill = np.full((iou_cap + GUARD, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)
        ctx.track_frame(tracker, ids_dev, table_dev, colors, live=live, n_live=n_live, iou=iou, live_cap=cap, iou_cap=iou_cap)
        if clobber:   # the record is the caller's again as soon as the call has returned: overwrite it on the stream, behind the frame
            ctx.lib.odise_hip_memset(ctx.h, C.c_void_p(buf.ptr), 0x5a, C.c_size_t(buf.nbytes))
        c, l, n, u = colors.numpy(), live.numpy(), int(n_live.numpy()[0]), iou.numpy()
        n_inst = want["iou"].shape[1]
        want_iou = iou_fill.copy()
        want_iou[:iou_cap, :n_inst] = want["iou"]
        want_live = live_guard(cap)
        want_live[:min(cap, len(want["live"]))] = want["live"][:cap]
        print(case.name, "frame", t, "n_live", n, "/", len(want["live"]), "colour bytes differing", int((c != want["colors"]).sum()),
              "live rows differing", int((l != want_live).sum()), "iou cells differing", int((u != want_iou).sum()))
        assert c.tobytes() == want["colors"].tobytes(), (case.name, t, "colors")          # non-instance rows keep the caller's bytes
        assert n == len(want["live"]), (case.name, t)
        assert l.tobytes() == want_live.tobytes(), (case.name, t, "live list / guard rows")
        assert u.tobytes() == want_iou.tobytes(), (case.name, t, "iou / guard rows")
        got.append((c.tobytes(), l.tobytes(), n, u.tobytes()))
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_sequence_matches_the_restatement_on_two_trackers_and_after_reset(ctx, name):
    case = CASES[name]
    a, b = ctx.track_create(case.hw, case.ttl, case.pool), ctx.track_create(case.hw, case.ttl, case.pool)
    try:
        first = run_sequence(ctx, case, a)
        assert run_sequence(ctx, case, b) == first, "two trackers differ"
        a.reset()
        assert run_sequence(ctx, case, a) == first, "not the first run again after a reset"
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.hw == TC.SMALL))
def test_unaligned_records_are_read_pixel_by_pixel(ctx, name):
    case = CASES[name]
    trk = ctx.track_create(case.hw, case.ttl, case.pool)
    try:
        run_sequence(ctx, case, trk, unaligned=True)
    finally:
        trk.close()


def test_both_sides_of_the_lds_limit_are_counted():
    """The kernel switches on the cells of the frame: the sequences above run on both sides of it (and close to it)."""
    cells = {name: histogram_cells(case) for name, case in CASES.items()}
    print({k: (min(v), max(v)) for k, v in cells.items()})
    assert max(cells["hundred"]) == 8 * 101 * 101 > LDS_CELLS
    assert cells["hundred"][1] == 101 * 101 <= LDS_CELLS < cells["hundred"][2] == 2 * 101 * 101       # the switch falls inside this sequence
    assert all(max(v) <= LDS_CELLS for k, v in cells.items() if k != "hundred")
    assert max(cells["long"]) > 100                                                                    # several retained maps in one pass


def test_a_short_live_cap_clips_the_dump_not_the_count(ctx):
    case = CASES["three_back"]
    trk = ctx.track_create(case.hw, case.ttl, case.pool)
    try:
        run_sequence(ctx, case, trk, live_cap=1)
        trk.reset()
        run_sequence(ctx, case, trk, live_cap=0)
    finally:
        trk.close()


def test_the_record_may_be_overwritten_as_soon_as_the_call_returns(ctx):
    for name in ("moving", "three_back", "gone7_ttl8"):
        case = CASES[name]
        trk = ctx.track_create(case.hw, case.ttl, case.pool)
        try:
            run_sequence(ctx, case, trk, clobber=True)
        finally:
            trk.close()


def test_frames_without_the_optional_outputs(ctx):
    case = CASES["two_claim"]
    trk = ctx.track_create(case.hw, case.ttl, case.pool)
    try:
        for (ids, tab), want in zip(case.frames, TC.expected(case)):
            _, ids_dev, table_dev = upload_record(ctx, record_of(ids, tab), ids.shape)
            colors = ctx.track_frame(trk, ids_dev, table_dev, ctx.to_device(TC.prefill()))
            assert colors.numpy().tobytes() == want["colors"].tobytes()
    finally:
        trk.close()


def test_bad_arguments_are_refused_and_nothing_is_written(ctx):
    lib, case = ctx.lib, CASES["two_claim"]
    pool = np.ascontiguousarray(case.pool)
    pp = pool.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()
    for H, W, ttl, p, n_pool, o in ((0, 8, 8, pp, 3, C.byref(out)), (8, 0, 8, pp, 3, C.byref(out)), (-1, 8, 8, pp, 3, C.byref(out)),
                                    (1 << 15, 1 << 14, 8, pp, 3, C.byref(out)), (8, 8, 0, pp, 3, C.byref(out)), (8, 8, 9, pp, 3, C.byref(out)),
                                    (8, 8, 8, pp, 0, C.byref(out)), (8, 8, 8, None, 3, C.byref(out)), (8, 8, 8, pp, 3, None)):
        assert lib.odise_hip_track_create(ctx.h, H, W, ttl, p, n_pool, o) == -1, (H, W, ttl, n_pool)
        assert out.value is None
    assert lib.odise_hip_track_create(None, 8, 8, 8, pp, 3, C.byref(out)) == -1
    assert lib.odise_hip_track_reset(ctx.h, None) == -1 and lib.odise_hip_track_destroy(ctx.h, None) == -1
    assert lib.odise_hip_track_frame(ctx.h, None) == -1

    trk = ctx.track_create(case.hw, case.ttl, case.pool)
    try:
        (ids, tab) = case.frames[0]
        _, ids_dev, table_dev = upload_record(ctx, record_of(ids, tab), ids.shape)
        colors = ctx.to_device(TC.prefill())
        live, n_live = ctx.to_device(live_guard(4)), ctx.to_device(np.full(1, -9, np.int32))
        iou_fill = np.full((4, MAX_SEGMENTS), -7.0, np.float64)
        iou = ctx.to_device(iou_fill)

        def desc(**kw):
            d = TrackDesc()
            d.track, d.H, d.W, d.pred_ids, d.pred_segments, d.colors = trk.handle, case.hw[0], case.hw[1], ids_dev.ptr, table_dev.ptr, colors.ptr
            d.live, d.live_cap, d.n_live, d.iou, d.iou_cap = live.ptr, 4, n_live.ptr, iou.ptr, 4
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        bad = [desc(track=None), desc(pred_ids=None), desc(pred_segments=None), desc(colors=None), desc(H=0), desc(W=-2),
               desc(H=case.hw[0] + 1), desc(W=case.hw[1] - 1), desc(H=case.hw[0] // 2, W=case.hw[1] * 2),   # a tracker made for another size
               desc(live_cap=-1), desc(iou_cap=-1), desc(n_live=None)]                                # .. live without n_live
        for d in bad:
            assert lib.odise_hip_track_frame(ctx.h, C.byref(d)) == -1
            assert lib.odise_hip_last_error()
        ctx.sync()
        assert colors.numpy().tobytes() == TC.prefill().tobytes() and live.numpy().tobytes() == live_guard(4).tobytes()
        assert int(n_live.numpy()[0]) == -9 and iou.numpy().tobytes() == iou_fill.tobytes()
        run_sequence(ctx, case, trk)                                                                  # and the tracker is where it was: empty
    finally:
        trk.close()
    with pytest.raises(RuntimeError):
        ctx.track_create((8, 8), ttl=9)


def test_video_visualizer_draws_the_restatements_pictures(ctx):
    """HipVideoVisualizer.draw_panoptic_seg_predictions over five frames against the numpy twin: picture bytes before the labels."""
    case = CASES["long"]
    metadata = {"thing_colors": [(10, 200, 30), (40, 50, 220)], "stuff_colors": [(k, 2 * k, 255 - k) for k in range(12)],
                "thing_classes": ["a", "b", "c", "d"], "stuff_classes": [f"s{k}" for k in range(12)]}
    vis, twin = V.HipVideoVisualizer(ctx, metadata, ttl=4), VD.ColorTracker(ttl=4)
    rng = np.random.default_rng(9)
    try:
        for t, (ids, tab) in enumerate(case.frames[4:9]):
            image = rng.integers(0, 256, case.hw + (3,)).astype(np.uint8)
            record = ctx.to_device(record_of(ids, tab))
            got = vis.draw_panoptic_seg_predictions(ctx.to_device(image), record, case.hw, labels=False)
            want = VD.draw_panoptic_seg_predictions(image, ids, tab, twin, metadata, labels=False)
            print("frame", t, "bytes differing", int((got != want).sum()))
            assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), t
        labelled = vis.draw_panoptic_seg_predictions(ctx.to_device(image), record, case.hw)
        assert labelled.shape == image.shape and labelled.dtype == np.uint8
        with pytest.raises(ValueError):
            vis.draw_panoptic_seg_predictions(ctx.to_device(image[:50]), record, (50, case.hw[1]))
    finally:
        vis.close()
