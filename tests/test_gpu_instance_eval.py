"""Instance masks against ground truth on the device (odise_amd/csrc/inst_eval.hip): `odise_hip_mask_iou` and `odise_hip_instance_eval`
against the host restatement (odise_amd/instance_eval.py, itself pinned by tests/test_instance_eval_cpu.py) - integers equal, doubles
bit for bit, rows byte for byte - on crafted masks, on the small model's mask logits, and `HipInstanceSegEvaluator` end to end."""
import math

import numpy as np
import pytest
import torch

import inst_cases as IC
from odise_amd import coco_rle as R
from odise_amd import instance_eval as IE
from odise_amd._lib import F32, U8
from odise_amd.instance_seg_eval import HipInstanceSegEvaluator
from small_model import GROUPS, build_small, image_u8

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))

CANARY = 0xA5
PAD = 256          # canary bytes on either side of an output


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


def _mask_iou(ctx, masks, counts, iscrowd=None):
    """-> (iou, inter, area_d, area_g, flags) through guarded outputs"""
    n, (h, w), n_gt = len(masks), masks.shape[1:], len(counts)
    gt = ctx.instance_gt_to_device(np.zeros((n_gt, 3), np.int32), np.concatenate([np.asarray(c, np.uint32) for c in counts] + [np.zeros(0, np.uint32)]),
                                   np.concatenate(([0], np.cumsum([len(c) for c in counts]))).astype(np.int64))
    crowd = ctx.to_device(np.asarray(iscrowd, np.uint8)) if iscrowd is not None else None
    out = [Guarded(ctx, (n, n_gt), np.float64), Guarded(ctx, (n, n_gt), np.int32), Guarded(ctx, (n,), np.int64), Guarded(ctx, (n_gt,), np.int64),
           Guarded(ctx, (1,), np.int32)]
    ctx.lib.odise_hip_memset(ctx.h, out[4].arr.ptr, 0, 4)
    dev = ctx.to_device(masks)
    rc = ctx.lib.odise_hip_mask_iou(ctx.h, dev.ptr, F32 if masks.dtype == np.float32 else U8, n, h, w, gt["runs"].ptr, gt["offsets"].ptr, n_gt,
                                    crowd.ptr if crowd is not None else None, *[o.arr.ptr for o in out])
    assert rc == 0, ctx.lib.odise_hip_last_error()
    ctx.sync()
    return out


def _check_iou(ctx, masks, counts, iscrowd=None, flag=0):
    iou, inter, area_d, area_g, flags = _mask_iou(ctx, masks, counts, iscrowd)
    h, w = masks.shape[1:]
    d = masks != 0
    g = np.stack([IE.decode_runs(c, h, w) for c in counts]).astype(bool)
    want_inter = (d.reshape(len(d), 1, -1) & g.reshape(1, len(g), -1)).sum(2) if len(d) * len(g) * h * w < 1 << 26 else \
        np.stack([(di.reshape(1, -1) & g.reshape(len(g), -1)).sum(1) for di in d])
    np.testing.assert_array_equal(inter.read(), want_inter)
    np.testing.assert_array_equal(area_d.read(), d.reshape(len(d), -1).sum(1))
    np.testing.assert_array_equal(area_g.read(), g.reshape(len(g), -1).sum(1))
    want = IE.mask_iou(masks, counts, iscrowd)
    got = iou.read()
    assert got.tobytes() == want.tobytes(), np.abs(got - want).max()
    assert int(flags.read()[0]) == flag


@pytest.mark.parametrize("h,w", [(1, 1), (1, 130), (130, 1), (63, 5), (64, 5), (65, 5), (200, 300)])
def test_mask_iou_on_the_mask_set(ctx, h, w):
    ms = IC.mask_set(h, w)
    counts = [R.mask_counts(m) for m in ms]
    crowd = [k % 3 == 1 for k in range(len(ms))]
    _check_iou(ctx, ms, counts, crowd)
    _check_iou(ctx, ms.astype(np.float32) * np.float32(0.75), [IC.with_zero_runs(c, k) for k, c in enumerate(counts)])


def test_mask_iou_across_the_pair_tiles(ctx):
    """100 x 300 masks: two tile rows of 64 detections, ten tile columns of 32 ground truths, the last of each ragged; 1200 noise-like runs
    per ground truth take the decoder through more than one chunk of 1024 runs."""
    g = np.random.default_rng(3)
    h, w = 65, 37
    d = (g.random((100, h, w)) < 0.4).astype(np.uint8)
    gt = (g.random((300, h, w)) < 0.5).astype(np.uint8)
    gt[::50] = 0
    counts = [R.mask_counts(m) for m in gt]
    assert max(len(c) for c in counts) > 1024
    _check_iou(ctx, d, counts, (g.random(300) < 0.2))


def test_mask_iou_empty_sides_write_nothing(ctx):
    ms = IC.mask_set(20, 9)
    for n, n_gt in ((0, 3), (3, 0)):
        out = [Guarded(ctx, (max(n, 1), max(n_gt, 1)), np.float64), Guarded(ctx, (1,), np.int32)]
        gt = ctx.instance_gt_to_device(np.zeros((3, 3), np.int32), np.concatenate([R.mask_counts(m).astype(np.uint32) for m in ms[:3]]),
                                       np.concatenate(([0], np.cumsum([len(R.mask_counts(m)) for m in ms[:3]]))).astype(np.int64))
        dev = ctx.to_device(ms[:3])
        assert ctx.lib.odise_hip_mask_iou(ctx.h, dev.ptr, U8, n, 20, 9, gt["runs"].ptr, gt["offsets"].ptr, n_gt, None, out[0].arr.ptr, None, None, None,
                                          out[1].arr.ptr) == 0
        ctx.sync()
        for o in out:
            o.read(intact=True)


@pytest.mark.parametrize("delta", [-7, +7, +100000])
def test_runs_that_do_not_sum_to_the_mask_raise_flag_1_and_stay_inside(ctx, delta):
    """The counts of one ground truth sum to less / more than h * w (once by far more): flag 1, every output inside its buffer, the other
    masks' values as always, and the call returns."""
    h, w = 65, 5
    ms = IC.mask_set(h, w)
    counts = [R.mask_counts(m).copy() for m in ms]
    bad = 7                                                                  # the blobs: several runs
    k = len(counts[bad]) // 2
    counts[bad][k] = max(0, counts[bad][k] + delta) if delta < 0 else counts[bad][k] + delta
    assert int(counts[bad].sum()) != h * w
    _check_iou(ctx, ms, counts, flag=IE.FLAG_BAD_RUNS)


# ---- instance_eval on crafted dense masks ----------------------------------------------------------------------------------------------
def _pad_case(c, topk):
    n = len(c["masks"])
    masks = np.zeros((topk,) + c["masks"].shape[1:], np.uint8)
    masks[:n] = c["masks"]
    table = np.zeros(1 + 2 * topk, np.int32)
    table[0] = n
    table[1 + topk:1 + topk + n] = c["classes"]
    scores = np.zeros(topk, np.float32)
    scores[:n] = c["scores"]
    return masks, table, scores


def _want_rows(c, image, topk):
    table, runs, offs = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"])
    full = np.zeros(topk, IE.ROW_DTYPE)
    full[:len(rows)] = rows
    return full, len(rows), flags, (table, runs, offs)


def _dense_eval(ctx, c, image, rows, n_rows, flags, topk=None, dtype=np.uint8, gt=None):
    topk = topk or len(c["masks"])
    masks, table, scores = _pad_case(c, topk)
    if gt is None:
        gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    dgt = ctx.instance_gt_to_device(*gt)
    ctx.instance_eval(masks.shape[1:], ctx.to_device(table), ctx.to_device(scores), topk, dgt, c["K"], image, rows, n_rows, flags,
                      masks=ctx.to_device(masks.astype(dtype)))
    ctx.sync()


@pytest.mark.parametrize("name", sorted(IC.matching_cases()) + ["random"])
def test_instance_eval_rows_equal_the_host_loop(ctx, name):
    c = IC.random_case() if name == "random" else IC.matching_cases()[name]
    topk = 100 if name == "random" else len(c["masks"]) + 3                 # rows past n are zeroed
    rows, n_rows, flags = Guarded(ctx, (topk,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), ctx.zeros((1,), np.int32)
    _dense_eval(ctx, c, 17, rows.arr, n_rows.arr, flags, topk, np.float32 if name == "random" else np.uint8)
    want, n, f, _ = _want_rows(c, 17, topk)
    assert f == 0 and int(flags.numpy()[0]) == 0 and int(n_rows.read()[0]) == n == len(c["masks"])
    got = rows.read()
    for field in IE.ROW_DTYPE.names:
        np.testing.assert_array_equal(got[field], want[field], err_msg=field)
    assert got.tobytes() == want.tobytes()


def test_a_second_picture_leaves_the_first_rows_alone_and_flags_empty_a_picture(ctx):
    a, b = IC.random_case(seed=8, n=40, n_gt=20), IC.random_case(seed=9, n=25, n_gt=0)
    topk = 40
    buf = ctx.zeros((3 * topk,), IE.ROW_DTYPE)
    counts, flags = ctx.zeros((3,), np.int32), ctx.zeros((1,), np.int32)
    slot = lambda i: (buf.view((topk,), IE.ROW_DTYPE, i * topk * 32), counts.view((1,), np.int32, 4 * i))
    _dense_eval(ctx, a, 0, *slot(0), flags, topk)
    first = buf.numpy()[:topk].copy()
    _dense_eval(ctx, b, 1, *slot(1), flags, topk)                            # no ground truth at all: every detection unmatched
    host = buf.numpy()
    assert host[:topk].tobytes() == first.tobytes() == _want_rows(a, 0, topk)[0].tobytes()
    assert host[topk:2 * topk].tobytes() == _want_rows(b, 1, topk)[0].tobytes()
    assert list(counts.numpy()) == [40, 25, 0] and int(flags.numpy()[0]) == 0
    # flag 2: a class outside [0, K); flag 4: a ground-truth category outside it; flag 1: bad runs.  Each gives n_rows = 0 and zeroed rows.
    gt = IE.gt_rows(a["annotations"], {k: k for k in range(a["K"])})
    bad_cls = dict(a, classes=np.where(np.arange(40) == 5, a["K"], a["classes"]).astype(np.int32))
    bad_cat = (np.where(np.arange(60).reshape(20, 3) == 6, a["K"] + 1, gt[0]).astype(np.int32), gt[1], gt[2])
    bad_crowd = (np.where(np.arange(60).reshape(20, 3) == 7, 2, gt[0]).astype(np.int32), gt[1], gt[2])
    runs = gt[1].copy()
    runs[3] += 1
    for case, g, want in ((bad_cls, gt, 2), (a, bad_cat, 4), (a, bad_crowd, 4), (a, (gt[0], runs, gt[2]), 1)):
        check = ctx.lib.odise_hip_memset(ctx.h, flags.ptr, 0, 4)
        assert check == 0
        ctx.lib.odise_hip_memset(ctx.h, buf.ptr, 0xFF, buf.nbytes)
        ctx.lib.odise_hip_memset(ctx.h, counts.ptr, 0xFF, counts.nbytes)
        _dense_eval(ctx, case, 2, *slot(2), flags, topk, gt=g)
        assert int(flags.numpy()[0]) == want and int(counts.numpy()[2]) == 0
        host = buf.numpy().view(np.uint8).reshape(3, -1)
        assert not host[2].any() and (host[:2] == 0xFF).all()


def test_bad_arguments_write_nothing(ctx):
    from odise_amd._lib import InstEvalDesc
    import ctypes as C
    c = IC.matching_cases()["areas"]
    masks, table, scores = _pad_case(c, 101)
    gt = ctx.instance_gt_to_device(*IE.gt_rows(c["annotations"], {0: 0}))
    rows, n_rows, flags = Guarded(ctx, (101,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
    dm, dt, ds = ctx.to_device(masks), ctx.to_device(table), ctx.to_device(scores)
    thr = np.ascontiguousarray(IE.IOU_THRS)

    def call(**over):
        d = InstEvalDesc()
        d.h, d.w, d.masks, d.dtype, d.inst_table, d.inst_scores, d.topk = IC.H, IC.W, dm.ptr, U8, dt.ptr, ds.ptr, 2
        d.gt_runs, d.gt_offsets, d.gt_rows, d.n_gt, d.num_categories = gt["runs"].ptr, gt["offsets"].ptr, gt["rows"].ptr, 1, 1
        d.iou_thresholds, d.rows, d.n_rows, d.flags = thr.ctypes.data, rows.arr.ptr, n_rows.arr.ptr, flags.arr.ptr
        for k, v in over.items():
            setattr(d, k, v)
        rc = ctx.lib.odise_hip_instance_eval(ctx.h, C.byref(d))
        return rc, ctx.lib.odise_hip_last_error().decode()

    for over, word in (({"topk": 101}, "topk"), ({"topk": 0}, "topk"), ({"n_gt": 1025}, "ground-truth"), ({"rows": None}, "null"),
                       ({"gt_runs": None}, "null"), ({"h": 0}, "size"), ({"dtype": 0}, "dtype")):
        rc, msg = call(**over)
        assert rc != 0 and word in msg, (over, rc, msg)
    ctx.sync()
    for o in (rows, n_rows, flags):
        o.read(intact=True)
    assert call()[0] == 0                                                   # the same descriptor, valid
    ctx.sync()
    assert int(n_rows.read()[0]) == 2


@pytest.mark.parametrize("dtype", [np.float64, np.int32])
def test_masks_of_an_unsupported_dtype_raise_and_write_nothing(ctx, dtype):
    """The smallest legal call but for the dtype of its masks: refused by the binding, before the library is called."""
    gt = ctx.instance_gt_to_device(np.zeros((0, 3), np.int32), np.zeros(0, np.uint32), np.zeros(1, np.int64))
    rows, n_rows, flags = Guarded(ctx, (1,), IE.ROW_DTYPE), Guarded(ctx, (1,), np.int32), Guarded(ctx, (1,), np.int32)
    with pytest.raises(ValueError, match="dtype"):
        ctx.instance_eval((1, 1), ctx.zeros((3,), np.int32), ctx.zeros((1,), np.float32), 1, gt, 1, 0, rows.arr, n_rows.arr, flags.arr,
                          masks=ctx.to_device(np.ones((1, 1, 1), dtype)))
    ctx.sync()
    for o in (rows, n_rows, flags):
        o.read(intact=True)


# ---- the small model: from the mask logits ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


def _annotations_from(masks, classes, shift=3):
    """Ground truth made of the picture's own predictions, so that matches exist: a mask shifted by a few pixels, two merged, one made a
    crowd, one with a class of its own."""
    m = masks > 0.5
    k = len(m)
    anns = [IC.ann(np.roll(m[0], shift, axis=1), int(classes[0])), IC.ann(m[1 % k] | m[2 % k], int(classes[1 % k])),
            IC.ann(m[3 % k], int(classes[3 % k]), iscrowd=1), IC.ann(np.roll(m[4 % k], -shift, axis=0), int(classes[5 % k]), compressed=False),
            IC.ann(m[6 % k], int(classes[6 % k]), area=50000.0)]
    return anns


@pytest.mark.parametrize("h,w", [(512, 512),      # x4 form
                                 (500, 502)])     # ragged: the generic sampler
def test_logits_path_equals_the_dense_form(small, ctx, h, w):
    hip, K = small, len(GROUPS)
    topk = int(hip.test_topk_per_image)
    hip.keep_instance_selection = True
    try:
        inst = hip.forward([{"image": image_u8(h, w, seed=h + w)}])[0]["instances"]
    finally:
        hip.keep_instance_selection = False
    sel = hip.last_selection
    n = len(inst["scores"])
    assert n > 6 and sel["topk"] == topk and sel["out_hw"] == [(h, w)]
    anns = _annotations_from(inst["pred_masks"], inst["pred_classes"])
    gt = ctx.instance_gt_to_device(*IE.gt_rows(anns, {k: k for k in range(K)}))
    rows = [ctx.zeros((topk,), IE.ROW_DTYPE) for _ in range(2)]
    n_rows, flags = ctx.zeros((2,), np.int32), ctx.zeros((1,), np.int32)
    table, scores = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)
    ctx.instance_eval((h, w), table, scores, topk, gt, K, 4, rows[0], n_rows.view((1,), np.int32), flags, b=0, pad_hw=sel["pad_hw"],
                      img_hw=sel["img_hw"][0])
    dense = np.zeros((topk, h, w), np.uint8)
    dense[:n] = inst["pred_masks"] > 0.5
    ctx.instance_eval((h, w), table, scores, topk, gt, K, 4, rows[1], n_rows.view((1,), np.int32, 4), flags, masks=ctx.to_device(dense))
    a, b = rows[0].numpy(), rows[1].numpy()
    assert list(n_rows.numpy()) == [n, n] and int(flags.numpy()[0]) == 0
    assert a.tobytes() == b.tobytes()
    assert (a["matched"] & ~a["ignored"]).any() and a["ignored"].any()
    c = IC.case(list(dense[:n]), inst["scores"], inst["pred_classes"], anns, K)
    assert a.tobytes() == _want_rows(c, 4, topk)[0].tobytes()


def test_evaluator_end_to_end(small, ctx):
    """Three pictures through HipInstanceSegEvaluator.process right behind the model call; evaluate() equals the host restatement fed
    with the host masks."""
    hip, K = small, len(GROUPS)
    names = [f"class{k}" for k in range(K)]
    ev = HipInstanceSegEvaluator(ctx, {100 + k: k for k in range(K)}, names, topk=int(hip.test_topk_per_image))
    ev.CHUNK = 2                                                            # three pictures cross a block of the row buffer
    ev.reset()
    host_rows, npig = [], np.zeros((K, 4), np.int64)
    hip.keep_instance_selection = True
    try:
        for i, (h, w) in enumerate(((512, 512), (320, 448), (500, 502))):
            inst = hip.forward([{"image": image_u8(h, w, seed=40 + i)}])[0]["instances"]
            anns = _annotations_from(inst["pred_masks"], inst["pred_classes"], shift=2 + i)
            c = IC.case(list((inst["pred_masks"] > 0.5).astype(np.uint8)), inst["scores"], inst["pred_classes"], anns, K)
            want, n, f, (table, _, _) = _want_rows(c, i, len(inst["scores"]))
            assert f == 0
            host_rows.append(want[:n])
            npig += IE.npig(table, K)
            for a in anns:
                a["category_id"] += 100                                     # dataset ids
            ev.process_selection(hip.last_selection, [anns], [i])
    finally:
        hip.keep_instance_selection = False
    got = ev.evaluate()
    want = IE.results(*IE.accumulate(np.concatenate(host_rows), npig, K), names)
    assert ev.rows().tobytes() == np.concatenate(host_rows).tobytes()
    assert set(got) == set(want) and not math.isnan(got["AP"]) and got["AP"] > 0
    for k in want:
        assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), k
