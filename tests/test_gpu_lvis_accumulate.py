"""GPU: odise_hip_lvis_accumulate (csrc/inst_accum.hip at 300 rows per slot and one cut) against lvis_eval.accumulate, byte for byte, on
seeded rows in the manner of tests/accum_cases.py; the flags; `HipLvisEvaluator.evaluate` against lvis_eval.results of the numpy rows."""
import numpy as np
import pytest

import accum_cases as AC
from lvis_cases import ann, rect
from odise_amd import instance_eval as IE
from odise_amd import lvis_eval as LE
from odise_amd.lvis_seg_eval import HipLvisEvaluator
from odise_amd.runtime import InstanceAccumulateError

pytestmark = pytest.mark.gpu

TOPK, K = 300, 5
COUNTS = (0, 1, 64, 65, 129, 257, 300)     # around the 64-lane chunks of a slot, and a full one


def block(g, pictures):
    """accum_cases.block at 300 rows per slot: junk where no row exists."""
    rows = np.zeros((len(pictures), TOPK), IE.ROW_DTYPE)
    rows["category"], rows["score"] = 1 << 20, np.nan
    rows["matched"] = rows["ignored"] = np.uint64(AC.MASK40)
    rows["image"] = g.integers(-5, 5, (len(pictures), TOPK))
    counts = np.zeros(len(pictures), np.int32)
    for s, p in enumerate(pictures):
        rows[s, :len(p)], counts[s] = p, len(p)
    return rows.reshape(-1), counts


def case(seed=0, spoil=None):
    """Seven pictures with COUNTS rows over two blocks (4 + 3 slots), image numbers descending across them; scores in sixteenths (ties
    within and across pictures) with +inf, -inf, -0 and 0 among them."""
    g = np.random.default_rng(seed)
    pics = []
    for i, n in enumerate(COUNTS):
        s = (g.integers(0, 17, n) / 16).astype(np.float32)
        if n >= 64:
            s[:4] = (np.inf, -np.inf, -0.0, 0.0)
        pics.append(AC.picture(g, 20 - 3 * i, g.integers(0, K, n), scores=s))
    if spoil:
        spoil(pics)
    blocks = [block(g, pics[:4]), block(g, pics[4:])]
    rows = np.concatenate(pics)
    per = np.bincount(rows["category"][(rows["category"] >= 0) & (rows["category"] < K)], minlength=K)
    npig = np.maximum(1, (per[:, None] * g.uniform(0.2, 0.6, (K, 4))).astype(np.int64))
    npig[4, 2] = 0
    return blocks, rows, npig


def test_device_equals_the_host_function_byte_for_byte(ctx):
    for seed in (0, 1):
        blocks, rows, npig = case(seed)
        assert np.signbit(rows["score"][rows["score"] == 0]).any() and np.isinf(rows["score"]).any()
        want_p, want_r = LE.accumulate(rows, npig, K)
        p, r = ctx.lvis_accumulate([(ctx.to_device(a), ctx.to_device(n)) for a, n in blocks], npig, K, TOPK)
        assert p.shape == (10, 101, K, 4) and r.shape == (10, K, 4)
        bad = np.argwhere(p != want_p)
        assert p.tobytes() == want_p.tobytes(), (len(bad), bad[:5].tolist())
        assert r.tobytes() == want_r.tobytes() and (p[:, :, 4, 2] == -1).all() and (p > 0).any() and (p[:, :, :4] >= 0).all()


def test_flags_fill_both_outputs_with_minus_one(ctx):
    def bad_class(pics): pics[4]["category"][70] = K
    def nan_score(pics): pics[5]["score"][200] = np.nan
    for flag, spoil in ((IE.ACCUM_FLAG_BAD_CLASS, bad_class), (IE.ACCUM_FLAG_NAN_SCORE, nan_score)):
        blocks, _, npig = case(2, spoil)
        with pytest.raises(InstanceAccumulateError) as e:
            ctx.lvis_accumulate(blocks, npig, K, TOPK)
        assert e.value.flags == flag and e.value.precision.shape == (10, 101, K, 4) and (e.value.precision == -1).all() and (e.value.recall == -1).all()


def test_topk_301_is_refused(ctx):
    with pytest.raises(RuntimeError, match=r"lvis_accumulate: topk 301 \(1\.\.300\)"):
        ctx.lvis_accumulate([(np.zeros(301, IE.ROW_DTYPE), np.zeros(1, np.int32))], np.ones((1, 4), np.int64), 1, 301)
    with pytest.raises(RuntimeError, match=r"instance_accumulate: topk 101 \(1\.\.100\)"):      # the cap of 100 stays where it was
        ctx.instance_accumulate([(np.zeros(101, IE.ROW_DTYPE), np.zeros(1, np.int32))], np.ones((1, 4), np.int64), 1, 101)


def test_the_evaluator_on_three_pictures(ctx):
    h, w, k = 40, 50, 4
    ids = {10: 0, 20: 1, 30: 2, 40: 3}
    a, b, c = rect(h, w, 2, 12, 3, 13), rect(h, w, 20, 30, 20, 40), rect(h, w, 5, 25, 5, 25)
    shifted = np.roll(a, 1, axis=1)
    pictures = [([(a, .9, 0), (b, .8, 1), (b, .7, 2), (shifted, .7, 0)], [ann(a, 10), ann(shifted, 10, ignore=1)], [30], []),
                ([(c, .6, 2), (b, .6, 1), (a, .5, 1)], [ann(c, 30), ann(b, 20)], [], [20]),
                ([], [ann(b, 10)], [20], [40])]
    ev = HipLvisEvaluator(ctx, ids, ["ten", "twenty", "thirty", "forty"], ["f", "c", "r", "r"])
    ev.CHUNK = 2                                                             # three pictures cross a block of the row buffer
    ev.reset()
    with pytest.raises(ValueError, match="neg_category_ids"):
        ev.process_masks(np.zeros((0, h, w), np.uint8), [], [], [], [99], [], 0)
    rows, npig = [], np.zeros((k, 4), np.int64)
    for i, (dets, anns, neg, nex) in enumerate(pictures):
        masks = np.stack([d[0] for d in dets]) if dets else np.zeros((0, h, w), np.uint8)
        scores, classes = [d[1] for d in dets], [d[2] for d in dets]
        ev.process_masks(masks, scores, classes, anns, neg, nex, 10 - i)
        table = LE.gt_rows(anns, ids)[0]
        npig += LE.npig(table, k)
        got, f = LE.image_rows(masks, scores, classes, [IE.annotation_counts(x["segmentation"]) for x in anns], table, [ids[x] for x in neg],
                               [ids[x] for x in nex], 10 - i, num_categories=k)
        assert f == 0
        rows.append(got)
    rows = np.concatenate(rows)
    assert ev.rows().tobytes() == rows.tobytes() and len(rows) == 6 and (ev._npig == npig).all()
    want = LE.results(*LE.accumulate(rows, npig, k), ["f", "c", "r", "r"])
    dev, host = ev.evaluate(accumulate_on="device"), ev.evaluate(accumulate_on="host")
    assert dev == host == {"segm": want} and 0 < want["AP"] < 100 and want["APr"] > 0
