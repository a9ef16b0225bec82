"""Cost of the segm evaluator's per-picture work at 1024x1024, 100 detections against 64 ground truths:

  eval         odise_hip_instance_eval from the mask logits: pack, ground-truth decode, intersections, areas, matching
  eval_no_gt   the same call with no ground truth (pack, areas, matching of 100 unmatched detections): eval - eval_no_gt is what the
               decode and the 100 x 64 x 16 K word pairs of the intersections cost
  rle          odise_hip_instance_rle on the same selection - the call the evaluation no longer needs - with a string buffer that holds
               every string, so its write pass runs

The expectation to confirm or correct: the call is bounded by the pack stage it shares with `rle`, the intersections are a few tens of
microseconds of integer work.  Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up
first); the rows of the timed configuration are compared with the host restatement before anything is timed.  The selection comes from
the small synthetic model (tests/small_model.py) with the panoptic head off (20 queries x 11 classes: the top-k holds exactly 100
masks); the ground truth is 64 smooth masks (unions of ellipses, a few thousand runs each), some crowds, over the model's classes.
Prints one JSON line; --out also writes it.

    python tools/inst_eval_bench.py --out profiles/inst_eval_bench.json
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
from odise_amd.runtime import Context  # noqa: E402
from small_model import GROUPS, build_small, image_u8  # noqa: E402


def blobs(h, w, seed):
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y, x = np.ogrid[:h, :w]
    for _ in range(3):
        cy, cx, ry, rx = g.integers(0, h), g.integers(0, w), g.integers(16, h // 3), g.integers(16, w // 3)
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    hip = build_small(ctx, panoptic_on=False)
    h = w = a.size
    K, topk, n_gt = len(GROUPS), int(hip.test_topk_per_image), 64
    hip.keep_instance_selection = True
    inst = hip.forward([{"image": image_u8(h, w, seed=h + w)}])[0]["instances"]
    sel = hip.last_selection
    n = len(inst["scores"])
    g = np.random.default_rng(0)
    gts = [blobs(h, w, s) for s in range(n_gt)]
    anns = [{"category_id": int(g.integers(0, K)), "iscrowd": int(s % 9 == 4), "area": float(m.sum()),
             "segmentation": {"size": [h, w], "counts": R.counts_to_string(R.mask_counts(m))}} for s, m in enumerate(gts)]
    table, runs, offs = IE.gt_rows(anns, {k: k for k in range(K)})
    gt = ctx.instance_gt_to_device(table, runs, offs)
    no_gt = ctx.instance_gt_to_device(table[:0], runs[:0], offs[:1])
    rows, n_rows, flags = ctx.zeros((topk,), IE.ROW_DTYPE), ctx.zeros((1,), np.int32), ctx.zeros((1,), np.int32)
    itab, isc = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)

    def run(which):
        ctx.instance_eval((h, w), itab, isc, topk, which, K, 0, rows, n_rows, flags, b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0])

    run(gt)
    counts = [runs[offs[i]:offs[i + 1]] for i in range(n_gt)]
    want, f = IE.image_rows(inst["pred_masks"] > 0.5, inst["scores"], inst["pred_classes"], counts, table, 0, num_categories=K)
    got = rows.numpy()
    assert f == 0 and int(flags.numpy()[0]) == 0 and int(n_rows.numpy()[0]) == n == len(want)
    assert got[:n].tobytes() == want.tobytes(), "device rows and host restatement disagree"
    eval_ms = device_ms(ctx, lambda: run(gt), a.reps)
    no_gt_ms = device_ms(ctx, lambda: run(no_gt), a.reps)

    rles, _ = ctx.instance_rle(0, itab, topk, sel["pad_hw"], (h, w), (h, w))
    need = sum(len(r["counts"]) for r in rles)
    bufs = (ctx.empty((max(need, 1),), np.uint8), ctx.empty((topk + 1,), np.int64), ctx.empty((topk,), np.int64))
    rle_ms = device_ms(ctx, lambda: ctx.instance_rle_async(0, itab, topk, sel["pad_hw"], (h, w), (h, w), bufs=bufs), a.reps)
    r = {"size": [h, w], "detections": n, "n_gt": n_gt, "gt_runs": int(runs.size), "instance_eval_ms": round(eval_ms, 4),
         "instance_eval_no_gt_ms": round(no_gt_ms, 4), "decode_plus_intersections_ms": round(eval_ms - no_gt_ms, 4),
         "instance_rle_ms": round(rle_ms, 4), "eval_over_rle": round(eval_ms / rle_ms, 3),
         "matched_rows": int(np.count_nonzero(got["matched"])), "rle_bytes": int(need), "reps": a.reps}
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
