"""GPU: odise_hip_video_eval_reset / _frame / _finish (csrc/video_eval.hip) and HipVideoInstanceEvaluator against the numpy
specification (odise_amd/video_eval.py).  Everything is integers and single double divisions, so every comparison is ==."""
import ctypes as C

import numpy as np
import pytest
import torch

from odise_amd import coco_poly, coco_rle
from odise_amd import instance_eval as IE
from odise_amd import video_eval as VE
from odise_amd._lib import U8, InstPolyGt, VideoFinishDesc, VideoFrameDesc
from odise_amd.video_seg_eval import HipVideoInstanceEvaluator
from small_model import GROUPS, build_small, image_u8

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

CANARY, PAD = 0xA5, 256


class Guarded:
    """A device output with canary bytes around it."""

    def __init__(self, ctx, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.buf = ctx.to_device(np.full(self.nbytes + 2 * PAD, CANARY, np.uint8))
        self.arr = self.buf.view(shape, dtype, PAD)

    def read(self, intact=False):
        raw = self.buf.numpy()
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + self.nbytes:] == CANARY).all(), "canary overwritten"
        if intact:
            assert (raw == CANARY).all(), "output written"
        return self.arr.numpy()


H, W = 70, 37          # two words per column, the second ragged; an odd width
K = 2


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = 1
    return m


def rle_gt(mask, compressed=True):
    return coco_rle.encode(mask) if compressed else {"size": list(mask.shape), "counts": coco_rle.mask_counts(mask).tolist()}


def gt_mask(seg, h, w):
    cnts = IE.annotation_counts(seg) if isinstance(seg, dict) else coco_poly.annotation_to_counts(seg, h, w)
    return IE.decode_runs(cnts, h, w)


def small_video():
    """T = 3, topk 8 with a table count of 5, tracks 0..5, ground-truth tracks 0..4 -> frames [(masks [8,H,W], n, det_slot [8],
    [(gt slot, segmentation)])]: runs in frame 0, no ground truth in frame 1, polygons and runs in frame 2; a detection and an
    annotation with slots out of range; track 2 absent from the middle frame; masks and slots past the count that must not be read."""
    rng = np.random.default_rng(7)
    base = [(2, 3), (30, 5), (50, 20), (10, 18), (40, 2), (20, 10)]              # (y, x) of track s in frame 0; 18 x 12 boxes, moving
    where = lambda s, f: (base[s][0] + 3 * f, base[s][0] + 3 * f + 18, base[s][1] + 2 * f, base[s][1] + 2 * f + 12)
    slots = [[0, 1, 2, 7, 3], [0, 1, -1, 3, 5], [3, 2, 1, 0, 9]]
    frames = []
    for f in range(3):
        masks = (rng.random((8, H, W)) < .5).astype(np.uint8)                    # past the count: noise on a live slot
        for i, s in enumerate(slots[f]):
            masks[i] = rect(H, W, *where(s % 6, f)) if i != 2 or f != 1 else rect(H, W, 0, 9, 0, 9)
        masks[4] &= (rng.random((H, W)) < .8).astype(np.uint8)
        det_slot = np.asarray(slots[f] + [4, 4, 0], np.int32)
        y0, y1, x0, x1 = where(3, f)
        gts = [[(0, rle_gt(rect(H, W, 4, 24, 3, 14))), (1, rle_gt(rect(H, W, 28, 50, 6, 20), compressed=False)), (2, rle_gt(rect(H, W, 52, 70, 18, 37))),
                (4, rle_gt(rect(H, W, 0, 70, 0, 2)))],
               [],
               [(1, rle_gt(rect(H, W, 36, 54, 9, 21))), (6, rle_gt(rect(H, W, 0, 70, 0, 37))), (0, rle_gt(rect(H, W, 8, 26, 7, 19), compressed=False)),
                (3, [[x0 + .0, y0 + .0, x1 + .0, y0 + .0, x1 + .0, y1 + .0, x0 + .0, y1 + .0], [1.5, 60.25, 9.0, 61.0, 4.0, 69.5]])]][f]
        frames.append((masks, 5, det_slot, gts))
    return frames


GT_TRACKS = [{"category_id": 0, "iscrowd": 0, "avg_area": 220.0}, {"category_id": 1, "iscrowd": 0, "avg_area": 20000.0},
             {"category_id": 0, "iscrowd": 1, "avg_area": 300.0}, {"category_id": 1, "iscrowd": 0, "avg_area": 216.0},
             {"category_id": 0, "iscrowd": 0, "avg_area": 70000.0}]
SCORES = np.asarray([.9, .8, .8, .95, .3, .6], np.float32)
CATS = np.asarray([0, 1, 0, 1, 0, 1], np.int32)


def spec_counts(frames, max_tracks, max_gt, counts=None):
    c = counts or VE.Counts(max_tracks, max_gt)
    flags = 0
    for masks, n, det_slot, gts in frames:
        h, w = masks.shape[1:]
        g = np.stack([gt_mask(seg, h, w) for _, seg in gts]) if gts else np.zeros((0, h, w), np.uint8)
        flags |= c.add_frame(masks[:n], det_slot[:n], g, [s for s, _ in gts])
    return c, flags


def table_of(n, topk, classes=None):
    t = np.zeros(1 + 2 * topk, np.int32)
    t[0] = n
    t[1 + topk:] = -7 if classes is None else classes                            # the frame call reads no class
    return t


def run_frames(ctx, ev, frames, dtype=np.uint8):
    for f, (masks, n, det_slot, gts) in enumerate(frames):
        topk, h, w = masks.shape
        ev.process_frame(f, (h, w), det_slot, masks=ctx.to_device(masks.astype(dtype)), table_row=ctx.to_device(table_of(n, topk)), annotations=gts)


def state_bytes(ev):
    return b"".join(a.tobytes() for a in ev.state.numpy())


def check_state(ev, c):
    inter, area_d, area_g, frames_d = ev.state.numpy()
    assert (inter == c.inter).all() and (area_d == c.area_d).all() and (area_g == c.area_g).all() and (frames_d == c.frames_d).all()


def padded(rows, topk):
    out = np.zeros(topk, IE.ROW_DTYPE)
    out[:len(rows)] = rows
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_small_video_equals_the_specification(ctx, dtype):
    frames = small_video()
    ev = HipVideoInstanceEvaluator(ctx, {0: 0, 1: 1}, ["a", "b"], max_tracks=6, max_gt=5)
    want, wflags = spec_counts(frames, 6, 5)
    assert wflags == 0 and want.inter.any() and int(want.frames_d[2]) == 2 and int(want.frames_d[5]) == 1 and int(want.area_d[4]) == 0
    iou, area = ctx.empty((6, 5), np.float64), ctx.empty((6,), np.float64)
    outs = []
    for _ in range(2):                                                           # the second run starts from a reset and gives the same bytes
        ev.begin_video(3, GT_TRACKS)
        assert not any(a.any() for a in ev.state.numpy())                        # reset really zeroes
        run_frames(ctx, ev, frames, dtype)
        check_state(ev, want)
        ev.end_video(SCORES, CATS, iou=iou, avg_area=area)
        outs.append((state_bytes(ev), iou.numpy().tobytes(), area.numpy().tobytes(), ev.rows().tobytes()))
    assert int(ev.flags.numpy()[0]) == 0
    assert (iou.numpy() == want.iou()).all() and (area.numpy() == want.avg_area()).all()
    table = VE.gt_track_rows(GT_TRACKS, {0: 0, 1: 1})
    rows, flags = VE.rows_from_counts(want, SCORES, CATS, table, video=3, num_categories=K)
    assert flags == 0 and (rows["matched"] & ~rows["ignored"]).any() and rows["ignored"].any()
    got = ev.rows()
    assert len(got) == 12 and got[:6].tobytes() == rows.tobytes() and got[6:].tobytes() == rows.tobytes()
    blocks, counts = ev._chunks[0]
    assert counts.numpy()[:3].tolist() == [6, 6, 0]
    assert outs[0][0] == outs[1][0] and outs[0][1:3] == outs[1][1:3] and outs[1][3][:len(outs[0][3])] == outs[0][3]


def test_sums_near_2_40_stay_in_64_bits(ctx):
    frames = small_video()[:1]
    ev = HipVideoInstanceEvaluator(ctx, {0: 0, 1: 1}, ["a", "b"], max_tracks=6, max_gt=5)
    want = VE.Counts(6, 5)
    rng = np.random.default_rng(1)
    want.inter[:] = (1 << 40) + rng.integers(0, 1000, (6, 5))
    want.area_d[:] = (1 << 40) + (1 << 20) + rng.integers(0, 1000, 6)
    want.area_g[:] = (1 << 41) + rng.integers(0, 1000, 5)
    want.frames_d[:] = [3, 1, 2, 5, 0, 7]
    ev.begin_video(0, GT_TRACKS)
    ev.state.copy_from(want.inter, want.area_d, want.area_g, want.frames_d)
    want, _ = spec_counts(frames, 6, 5, want)
    run_frames(ctx, ev, frames)
    check_state(ev, want)
    iou, area = ctx.empty((6, 5), np.float64), ctx.empty((6,), np.float64)
    ev.end_video(SCORES, CATS, iou=iou, avg_area=area)
    assert (iou.numpy() == want.iou()).all() and (area.numpy() == want.avg_area()).all() and iou.numpy().min() > .3
    rows, _ = VE.rows_from_counts(want, SCORES, CATS, VE.gt_track_rows(GT_TRACKS, {0: 0, 1: 1}), video=0, num_categories=K)
    assert rows["area"].max() == 2147483647 and ev.rows().tobytes() == rows.tobytes()     # means beyond int32 are clamped, beyond 1e10 ignored


def test_past_the_tile_and_through_accumulate(ctx):
    """max_tracks 100 and max_gt 70: two row tiles and three column tiles of the intersection; on through odise_hip_instance_accumulate."""
    rng = np.random.default_rng(11)
    h = w = 64
    T, G, Kc = 100, 70, 3
    track = np.zeros((T, h, w), np.uint8)                                        # track s in frame 0; frame 1 is one pixel to the right
    for s in range(T):
        y, x = rng.integers(0, 48, 2)
        track[s] = rect(h, w, y, y + rng.integers(4, 17), x, x + rng.integers(4, 17))
    of = rng.permutation(T)[:G]                                                  # ground-truth track j follows track of[j], a pixel off
    gtm = np.stack([np.roll(track[of[j]], rng.integers(-1, 2), axis=int(rng.integers(0, 2))) for j in range(G)])
    dperm, gperm = rng.permutation(T), rng.permutation(G)                        # frame 1 lists both sides in another order
    frames = [(track, T, np.arange(T, dtype=np.int32), [(j, rle_gt(gtm[j], compressed=bool(j & 1))) for j in range(G)]),
              (np.stack([np.roll(track[s], 1, axis=1) for s in dperm]), T, dperm.astype(np.int32),
               [(int(j), rle_gt(np.roll(gtm[j], 1, axis=1))) for j in gperm])]
    gt_tracks = [{"category_id": int(j % Kc), "iscrowd": int(j % 11 == 0), "avg_area": float(40 + 3 * j)} for j in range(G)]
    to_c = {k: k for k in range(Kc)}
    ev = HipVideoInstanceEvaluator(ctx, to_c, ["a", "b", "c"], max_tracks=T, max_gt=G)
    ev.begin_video(5, gt_tracks)
    run_frames(ctx, ev, frames)
    want, wflags = spec_counts(frames, T, G)
    assert wflags == 0
    check_state(ev, want)
    scores = rng.random(T).astype(np.float32).round(1)                            # ties
    cats = np.zeros(T, np.int32)
    cats[of] = np.arange(G) % Kc                                                 # a followed track has its ground truth's category
    cats[np.setdiff1d(np.arange(T), of)] = 1
    ev.end_video(scores, cats)
    table = VE.gt_track_rows(gt_tracks, to_c)
    rows, flags = VE.rows_from_counts(want, scores, cats, table, video=5, num_categories=Kc)
    assert flags == 0 and int(ev.flags.numpy()[0]) == 0
    assert ev.rows().tobytes() == rows.tobytes() and (rows["matched"] & ~rows["ignored"]).any()
    ev.evaluate()
    p, r = IE.accumulate(rows, IE.npig(table, Kc), Kc)
    assert ev.precision.tobytes() == p.tobytes() and ev.recall.tobytes() == r.tobytes() and (p > 0).any()
    ev.evaluate(accumulate_on="host")
    assert ev.precision.tobytes() == p.tobytes()


def test_flags(ctx):
    frames = small_video()
    ev = HipVideoInstanceEvaluator(ctx, {0: 0, 1: 1}, ["a", "b"], max_tracks=6, max_gt=5)
    # 16: two detections on one track, two annotations on one ground-truth track; both are added
    masks, n, det_slot, gts = frames[0]
    shared = [(masks, n, np.asarray([0, 0, 2, 7, 3, 4, 4, 0], np.int32), [(1, gts[0][1]), (1, gts[1][1]), (2, gts[2][1])])]
    want, wflags = spec_counts(shared, 6, 5)
    assert wflags == 16
    ev.begin_video(0, GT_TRACKS)
    run_frames(ctx, ev, shared)
    check_state(ev, want)
    assert int(ev.flags.numpy()[0]) == 16
    with pytest.raises(RuntimeError, match="share"):
        ev.evaluate()
    # 1: runs that do not sum to h * w - the frame adds nothing
    ev.reset()
    ev.begin_video(0, GT_TRACKS)
    bad = {"size": [H, W], "counts": coco_rle.mask_counts(rect(H, W, 0, 9, 0, 9)).tolist()}
    bad["counts"][-1] += 5
    ev.process_frame(0, (H, W), det_slot, masks=ctx.to_device(masks), table_row=ctx.to_device(table_of(n, 8)), annotations=[(0, bad), gts[1]])
    assert int(ev.flags.numpy()[0]) == 1 and not any(a.any() for a in ev.state.numpy())
    # 2: a track category outside the range empties the rows of the video
    ev.reset()
    ev.begin_video(0, GT_TRACKS)
    run_frames(ctx, ev, frames[:1])
    rows, counts = Guarded(ctx, (6,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32)
    table = ctx.to_device(VE.gt_track_rows(GT_TRACKS, {0: 0, 1: 1}))
    cats = CATS.copy()
    cats[3] = 2
    ctx.video_eval_finish(ev.state, 6, ctx.to_device(SCORES), ctx.to_device(cats), table, 5, K, 0, rows.arr, counts.arr, ev.flags)
    assert int(ev.flags.numpy()[0]) == 2 and int(counts.read()[0]) == 0 and not rows.read().tobytes().strip(b"\0")


def test_bad_arguments_enqueue_nothing(ctx):
    frames = small_video()
    masks, n, det_slot, gts = frames[0]
    state = ctx.video_eval_state(6, 5)
    state.buf.copy_from(np.full(state.buf.shape, 0x5A, np.uint8))
    rows, n_rows, flags = Guarded(ctx, (6,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
    iou = Guarded(ctx, (6, 5), np.float64)
    anns = [{"category_id": 0, "area": 0.0, "segmentation": seg} for _, seg in gts]
    gt = ctx.instance_gt_to_device(*IE.gt_rows(anns, {0: 0}))
    dm, dt, dslot = ctx.to_device(masks), ctx.to_device(table_of(n, 8)), ctx.to_device(det_slot)
    gslot = ctx.to_device(np.asarray([s for s, _ in gts], np.int32))
    sc, ca, tb = ctx.to_device(SCORES), ctx.to_device(CATS), ctx.to_device(VE.gt_track_rows(GT_TRACKS, {0: 0, 1: 1}))
    thr = np.ascontiguousarray(IE.IOU_THRS)
    pxy, poff, ppol = ctx.to_device(np.zeros(6, np.float64)), ctx.to_device(np.asarray([0, 3], np.int64)), ctx.to_device(np.asarray([0, 1, 1, 1, 1], np.int32))

    def poly(**over):
        p = InstPolyGt()
        p.xy, p.poly_offsets, p.gt_polys, p.n_poly = pxy.ptr, poff.ptr, ppol.ptr, 1
        for k, v in over.items():
            setattr(p, k, v)
        return p

    def st(**over):
        s = type(state.struct).from_buffer_copy(state.struct)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def frame(**over):
        d = VideoFrameDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.topk, d.det_slot = H, W, dm.ptr, U8, dt.ptr, 8, dslot.ptr
        d.gt_runs, d.gt_offsets, d.n_gt, d.gt_slot, d.flags = gt["runs"].ptr, gt["offsets"].ptr, 4, gslot.ptr, flags.arr.ptr
        s, p = over.pop("state", state.struct), over.pop("poly", None)
        d.st = C.addressof(s) if s is not None else None
        d.polys = C.addressof(p) if p is not None else None
        for k, v in over.items():
            setattr(d, k, v)
        rc = ctx.lib.odise_hip_video_eval_frame(ctx.h, C.byref(d))
        return rc, ctx.lib.odise_hip_last_error().decode()

    def finish(**over):
        d = VideoFinishDesc()
        d.n_tracks, d.track_scores, d.track_category, d.gt_rows, d.n_gt, d.num_categories, d.video = 6, sc.ptr, ca.ptr, tb.ptr, 5, K, 0
        d.iou_thresholds, d.rows, d.n_rows, d.flags, d.iou = thr.ctypes.data, rows.arr.ptr, n_rows.arr.ptr, flags.arr.ptr, iou.arr.ptr
        s = over.pop("state", state.struct)
        d.st = C.addressof(s) if s is not None else None
        for k, v in over.items():
            setattr(d, k, v)
        rc = ctx.lib.odise_hip_video_eval_finish(ctx.h, C.byref(d))
        return rc, ctx.lib.odise_hip_last_error().decode()

    for over, word in (({"topk": 0}, "topk"), ({"topk": 101}, "topk"), ({"n_gt": 1025}, "ground-truth"), ({"n_gt": -1}, "ground-truth"),
                       ({"h": 0}, "size"), ({"h": 40000, "w": 40000}, "size"), ({"dtype": 0}, "dtype"), ({"flags": None}, "null"),
                       ({"det_slot": None}, "null"), ({"gt_slot": None}, "null"), ({"gt_runs": None}, "null"), ({"state": None}, "null"),
                       ({"state": st(max_tracks=101)}, "max_tracks"), ({"state": st(max_tracks=0)}, "max_tracks"),
                       ({"state": st(max_gt=1025)}, "max_gt"), ({"state": st(inter=None)}, "null"), ({"state": st(frames_d=None)}, "null"),
                       ({"masks": None}, "null"),                                # no dense masks and no scores: no source
                       ({"poly": poly(n_poly=-1)}, "polygons"), ({"poly": poly(xy=None)}, "null polygon"), ({"poly": poly(poly_offsets=None)}, "null polygon"),
                       ({"poly": poly(gt_polys=None)}, "null polygon"),          # the polygon errors of odise_hip_instance_eval_poly
                       ({"det_slot": dslot.ptr + 2}, "aligned"), ({"gt_slot": gslot.ptr + 2}, "aligned"), ({"flags": flags.arr.ptr + 2}, "aligned"),
                       ({"inst_table": dt.ptr + 2}, "aligned"), ({"state": st(inter=state.inter.ptr + 4)}, "aligned"),
                       ({"state": st(area_d=state.area_d.ptr + 4)}, "aligned"), ({"state": st(area_g=state.area_g.ptr + 4)}, "aligned"),
                       ({"state": st(frames_d=state.frames_d.ptr + 2)}, "aligned")):
        rc, msg = frame(**over)
        assert rc == -1 and word in msg, (over, rc, msg)
    for over, word in (({"n_tracks": 7}, "tracks"), ({"n_tracks": -1}, "tracks"), ({"n_gt": 6}, "ground-truth"), ({"iou_thresholds": None}, "null"),
                       ({"flags": None}, "null"), ({"rows": None}, "only one"), ({"n_rows": None}, "only one"), ({"num_categories": 0}, "num_categories"),
                       ({"track_scores": None}, "null"), ({"track_category": None}, "null"), ({"gt_rows": None}, "null"),
                       ({"rows": None, "n_rows": None, "iou": None}, "no output"), ({"state": None}, "null"), ({"state": st(area_d=None)}, "null"),
                       ({"rows": rows.arr.ptr + 4}, "misaligned"), ({"iou": iou.arr.ptr + 4}, "misaligned"), ({"track_scores": sc.ptr + 2}, "misaligned"),
                       ({"gt_rows": tb.ptr + 2}, "misaligned"), ({"n_rows": n_rows.arr.ptr + 2}, "misaligned"),
                       ({"state": st(frames_d=state.frames_d.ptr + 2)}, "aligned")):
        rc, msg = finish(**over)
        assert rc == -1 and word in msg, (over, rc, msg)
    for s in (None, st(max_tracks=101), st(max_gt=-1), st(area_g=None)):
        assert ctx.lib.odise_hip_video_eval_reset(ctx.h, C.byref(s) if s is not None else None) == -1
    ctx.sync()
    for o in (rows, n_rows, flags, iou):
        o.read(intact=True)
    assert (state.buf.numpy() == 0x5A).all()
    # the same descriptors, valid
    ctx.video_eval_reset(state)
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    assert frame()[0] == 0 and finish()[0] == 0
    ctx.sync()
    assert int(n_rows.read()[0]) == 6 and int(flags.read()[0]) == 0
    want, _ = spec_counts(frames[:1], 6, 5)
    assert (iou.read() == want.iou()).all()


@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


def test_the_head_forward_source_equals_the_dense_form(small, ctx):
    """Two frames = the two images of one batch, sampled from the mask logits; against the dense path on the instance masks."""
    hip, h, w = small, 500, 502
    topk = int(hip.test_topk_per_image)
    hip.keep_instance_selection = True
    try:
        out = hip.forward([{"image": image_u8(h, w, seed=1)}, {"image": image_u8(h, w, seed=2)}])
    finally:
        hip.keep_instance_selection = False
    sel = hip.last_selection
    insts = [o["instances"] for o in out]
    assert sel["topk"] == topk and all(len(i["scores"]) > 3 for i in insts)
    rng = np.random.default_rng(3)
    slots = [rng.permutation(topk).astype(np.int32) for _ in range(2)]
    gts = [[(j, rle_gt((insts[b]["pred_masks"][j] > .5).astype(np.uint8))) for j in range(3)] for b in range(2)]
    states = []
    for dense in (False, True):
        ev = HipVideoInstanceEvaluator(ctx, {k: k for k in range(len(GROUPS))}, [str(k) for k in range(len(GROUPS))], max_tracks=topk, max_gt=4)
        ev.begin_video(0, [])
        for b in range(2):
            table = sel["inst_table"].view((1 + 2 * topk,), np.int32, b * (1 + 2 * topk) * 4)
            if dense:
                m = np.zeros((topk, h, w), np.uint8)
                m[:len(insts[b]["scores"])] = insts[b]["pred_masks"] > .5
                ev.process_frame(b, (h, w), slots[b], masks=ctx.to_device(m), table_row=table, annotations=gts[b])
            else:
                ev.process_frame(b, (h, w), slots[b], table_row=table, scores_row=sel["inst_scores"].view((topk,), np.float32, b * topk * 4), topk=topk,
                                 b=b, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][b], annotations=gts[b])
        assert int(ev.flags.numpy()[0]) == 0
        states.append(ev.state.numpy())
    assert all((a == b).all() for a, b in zip(*states)) and states[0][0].any()
    # the geometry errors of odise_hip_instance_rle, against the logits of this forward: refused, accumulators and flags untouched
    (ph, pw), (ih, iw) = sel["pad_hw"], sel["img_hw"][0]
    state = ctx.video_eval_state(topk, 4)
    state.buf.copy_from(np.full(state.buf.shape, 0x5A, np.uint8))
    flags = Guarded(ctx, (1,), np.int32)
    gt = ctx.instance_gt_to_device(None, *VE.pack_segmentations([seg for _, seg in gts[0]], (h, w))[:2])
    dslot, gslot = ctx.to_device(slots[0]), ctx.to_device(np.arange(3, dtype=np.int32))

    def logits_frame(b, p_h, p_w, i_h, i_w, o_h=h, o_w=w):
        d = VideoFrameDesc()
        d.h, d.w, d.topk, d.inst_table, d.inst_scores, d.det_slot = o_h, o_w, topk, sel["inst_table"].ptr, sel["inst_scores"].ptr, dslot.ptr
        d.b, d.pad_h, d.pad_w, d.img_h, d.img_w = b, p_h, p_w, i_h, i_w
        d.gt_runs, d.gt_offsets, d.n_gt, d.gt_slot, d.st, d.flags = gt["runs"].ptr, gt["offsets"].ptr, 3, gslot.ptr, C.addressof(state.struct), flags.arr.ptr
        return ctx.lib.odise_hip_video_eval_frame(ctx.h, C.byref(d))

    for bad in ((-1, ph, pw, ih, iw), (2, ph, pw, ih, iw), (0, ph + 4, pw, ih, iw), (0, ph, pw - 4, ih, iw), (0, ph, pw, 0, iw), (0, ph, pw, ih, pw + 1),
                (0, ph, pw, ph + 1, iw), (0, ph, pw, ih, iw, 0, w), (0, ph, pw, ih, iw, 40000, 40000)):
        assert logits_frame(*bad) == -1, bad
    ctx.sync()
    flags.read(intact=True)
    assert (state.buf.numpy() == 0x5A).all()
    ctx.video_eval_reset(state)                                                  # the same descriptor, valid
    ctx.lib.odise_hip_memset(ctx.h, flags.arr.ptr, 0, 4)
    assert logits_frame(0, ph, pw, ih, iw) == 0
    assert int(flags.read()[0]) == 0 and state.numpy()[1].any()
    frames = []
    for b in range(2):
        n = len(insts[b]["scores"])
        frames.append(((insts[b]["pred_masks"] > .5).astype(np.uint8), n, slots[b], gts[b]))
    want, _ = spec_counts(frames, topk, 4)
    assert (states[0][0] == want.inter).all() and (states[0][1] == want.area_d).all() and (states[0][3] == want.frames_d).all()


def test_the_front_door_on_the_device_equals_the_specification(ctx, tmp_path):
    """`--device gpu` of python -m odise_amd.video_eval: dense masks without a table, the placeholder frame of a video without results,
    a video of more than 100 tracks walked in two parts (count_gt False, the host accumulate for a repeated video number)."""
    from video_cases import write_pair
    for crowded in (False, True):
        rp, gp = write_pair(tmp_path, True, crowded=crowded)
        want, got = VE.evaluate_files(rp, gp, "cpu"), VE.evaluate_files(rp, gp, "gpu", ctx=ctx)
        assert got["stats"].tobytes() == want["stats"].tobytes() and got["results"].keys() == want["results"].keys()
        assert all(got["results"][k] == want["results"][k] or (got["results"][k] != got["results"][k] and want["results"][k] != want["results"][k])
                   for k in want["results"])
        assert 0 < want["stats"][0] <= 1
    rp, gp = write_pair(tmp_path, False)
    assert VE.evaluate_files(rp, gp, "gpu", ctx=ctx)["stats"].tobytes() == VE.evaluate_files(rp, gp, "cpu")["stats"].tobytes()


def test_evaluate_before_any_video(ctx):
    ev = HipVideoInstanceEvaluator(ctx, {0: 0, 1: 1}, ["a", "b"], max_tracks=6, max_gt=5)
    out = ev.evaluate()["segm"]
    p, r = IE.accumulate(np.zeros(0, IE.ROW_DTYPE), np.zeros((2, 4), np.int64), 2)
    assert ev.precision.tobytes() == p.tobytes() and ev.recall.tobytes() == r.tobytes() and (p == -1).all() and out["AP"] != out["AP"]
    assert len(ev.rows()) == 0
