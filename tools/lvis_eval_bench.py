"""Cost of one picture of the LVIS evaluator at 1024x1024, 300 detections against 20 ground truths, K = 1203:

  lvis_dense      odise_hip_lvis_eval on 300 dense uint8 masks: 300 packs, 300 x 20 intersections, the walk at 300 detections
  lvis_logits     the same call on a table of 300 (query, class) pairs over the mask logits of a head forward: every distinct query is
                  packed, counted and intersected once.  The head is the small test model (tests/small_model.py: 20 queries, not the 100 of
                  the full model), so this is the shared pack at 20 distinct masks
  instance_100    odise_hip_instance_eval at topk 100 on the first 100 of the dense masks: the call an evaluator made before
  accumulate      odise_hip_lvis_accumulate on 500 pictures of 300 rows

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context, warmed up first, the median of `--repeats`
such measurements with their spread beside it; the rows of the timed dense configuration are compared with the host restatement at a
reduced size before anything is timed.  Prints one JSON line; --out also writes it.

    python tools/lvis_eval_bench.py --out profiles/lvis_eval_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from odise_amd import coco_rle as R  # noqa: E402
from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd import lvis_eval as LE  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def blobs(h, w, seed):
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y, x = np.ogrid[:h, :w]
    for _ in range(3):
        cy, cx, ry, rx = g.integers(0, h), g.integers(0, w), g.integers(16, h // 3), g.integers(16, w // 3)
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


def device_ms(ctx, fn, reps, repeats):
    for _ in range(5):
        fn()
    ctx.sync()
    out = []
    for _ in range(repeats):
        ctx.timer_start()
        for _ in range(reps):
            fn()
        out.append(ctx.timer_stop() / reps)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--pictures", type=int, default=500)
    ap.add_argument("--no-logits", action="store_true", help="skip the head forward of the small model")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    h = w = a.size
    K, topk, n_gt = 1203, 300, 20
    g = np.random.default_rng(0)
    base = np.stack([blobs(h, w, 100 + s) for s in range(100)])
    masks = base[np.arange(topk) % 100]                            # 300 detections over 100 distinct masks, as the head gives them
    gts = [blobs(h, w, s) for s in range(n_gt)]
    cats = (np.arange(n_gt) * 61) % K
    anns = [{"category_id": int(cats[s]), "area": float(m.sum()), "segmentation": {"size": [h, w], "counts": R.counts_to_string(R.mask_counts(m))}}
            for s, m in enumerate(gts)]
    table, runs, offs = LE.gt_rows(anns, {k: k for k in range(K)})
    classes = np.where(g.random(topk) < .6, cats[g.integers(0, n_gt, topk)], g.integers(0, K, topk)).astype(np.int32)
    neg = sorted({int(c) for c in g.integers(0, K, 40)})
    nex = sorted({int(c) for c in cats[:3]})
    gt = ctx.instance_gt_to_device(table, runs, offs, lvis_bits=(LE.category_bits(neg, K), LE.category_bits(nex, K)))
    itab = np.zeros(1 + 2 * topk, np.int32)
    itab[0], itab[1:1 + topk], itab[1 + topk:] = topk, np.arange(topk), classes
    scores = g.random(topk).astype(np.float32)
    dm, dtab, dsc = ctx.to_device(masks), ctx.to_device(itab), ctx.to_device(scores)
    t100 = np.zeros(201, np.int32)
    t100[0], t100[1:101], t100[101:] = 100, np.arange(100), classes[:100]
    dm100, dtab100, dsc100 = ctx.to_device(masks[:100]), ctx.to_device(t100), ctx.to_device(scores[:100])
    rows, n_rows, flags = ctx.zeros((topk,), IE.ROW_DTYPE), ctx.zeros((1,), np.int32), ctx.zeros((1,), np.int32)

    def lvis_dense():
        ctx.lvis_eval((h, w), dtab, dsc, topk, gt, K, 0, rows, n_rows, flags, masks=dm)

    def instance_100():
        ctx.instance_eval((h, w), dtab100, dsc100, 100, gt, K, 0, rows, n_rows, flags, masks=dm100)

    # the dense configuration against the host restatement, at every 8th pixel (the host IoU is a Python loop)
    sm, sg = masks[:, ::8, ::8], [m[::8, ::8] for m in gts]
    s_anns = [{"category_id": int(cats[s]), "area": float(m.sum()), "segmentation": R.encode(np.ascontiguousarray(m))} for s, m in enumerate(sg)]
    s_table, s_runs, s_offs = LE.gt_rows(s_anns, {k: k for k in range(K)})
    s_gt = ctx.instance_gt_to_device(s_table, s_runs, s_offs, lvis_bits=(LE.category_bits(neg, K), LE.category_bits(nex, K)))
    ctx.lvis_eval(sm.shape[1:], dtab, dsc, topk, s_gt, K, 0, rows, n_rows, flags, masks=ctx.to_device(np.ascontiguousarray(sm)))
    want, wf = LE.image_rows(sm, scores, classes, [IE.annotation_counts(x["segmentation"]) for x in s_anns], s_table, neg, nex, 0, num_categories=K)
    n = int(n_rows.numpy()[0])
    assert wf == 0 and int(flags.numpy()[0]) == 0 and n == len(want) > 0 and rows.numpy()[:n].tobytes() == want.tobytes()

    med = lambda v: float(np.median(v))
    r = {"size": [h, w], "detections": topk, "n_gt": n_gt, "K": K, "kept_rows_checked": n, "reps": a.reps, "repeats": a.repeats}
    timed = [("lvis_dense", lvis_dense), ("instance_100", instance_100)]
    if not a.no_logits:
        from small_model import build_small, image_u8
        hip = build_small(ctx)
        hip.keep_instance_selection = True
        hip.forward([{"image": image_u8(500, 502, seed=1)}])
        sel = hip.last_selection
        Q = 20
        qtab = itab.copy()
        qtab[1:1 + topk] = np.arange(topk) % Q
        dq = ctx.to_device(qtab)
        timed.append(("lvis_logits", lambda: ctx.lvis_eval((h, w), dq, dsc, topk, gt, K, 0, rows, n_rows, flags, b=0, pad_hw=sel["pad_hw"],
                                                           img_hw=sel["img_hw"][0])))
        r["logits_queries"] = Q
    for name, fn in timed:
        v = device_ms(ctx, fn, a.reps, a.repeats)
        r[name + "_ms"], r[name + "_ms_runs"] = round(med(v), 4), [round(x, 4) for x in v]
    assert int(flags.numpy()[0]) == 0

    P = a.pictures
    acc = np.zeros((P, topk), IE.ROW_DTYPE)
    acc["score"], acc["category"] = g.random((P, topk)), g.integers(0, K, (P, topk))
    acc["image"] = np.arange(P)[:, None]
    acc["matched"], acc["ignored"] = g.integers(0, 1 << 40, (P, topk)), g.integers(0, 1 << 40, (P, topk)) & g.integers(0, 1 << 40, (P, topk))
    acc = np.take_along_axis(acc, np.argsort(-acc["score"], axis=1, kind="stable"), axis=1)
    blocks = [(ctx.to_device(acc.reshape(-1)), ctx.to_device(np.full(P, topk, np.int32)))]
    npig = ctx.to_device(g.integers(1, 50, (K, 4)).astype(np.int64))
    v = []
    for i in range(2 + a.repeats):                                  # the call reads back: wall time around it, the first two are warm-up
        ctx.sync()
        ctx.timer_start()
        ctx.lvis_accumulate(blocks, npig, K, topk)
        v.append(ctx.timer_stop())
    v = v[2:]
    r.update(accumulate_pictures=P, lvis_accumulate_ms=round(med(v), 4), lvis_accumulate_ms_runs=[round(x, 4) for x in v])
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
