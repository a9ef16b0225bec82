"""Cost of polygon ground truth in the segm evaluator at 1024x1024, 100 detections against 64 ground truths of about 40 vertices each:

  eval_poly    odise_hip_instance_eval_poly: the ground truth rasterised from its polygons (csrc/poly.hip), then intersections and matching
  eval_rle     odise_hip_instance_eval on the same masks handed over as run lengths - the path the polygons had to be converted for
  host         the host reference (coco_poly.annotation_to_counts) over the same 64 annotations, for scale

The claim to check: rasterising costs the same order as the run-length decode it replaces.  Device times are HIP events around `--reps`
back-to-back calls on an otherwise idle context (warmed up first); the rows of both forms are compared with each other before anything
is timed.  The detections are dense masks (jittered ground truth), so no model is loaded.  Prints one JSON line; --out also writes it.

    python tools/poly_bench.py --out profiles/poly_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from odise_amd import coco_poly as P  # noqa: E402
from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def blob_polygon(g, h, w, k=40):
    """A star-shaped polygon of k vertices: a wobbling radius around a random centre."""
    cy, cx = g.uniform(.15 * h, .85 * h), g.uniform(.15 * w, .85 * w)
    r = g.uniform(.04, .22) * min(h, w) * (1 + .25 * g.standard_normal(k)).clip(.4, 1.6)
    a = np.sort(g.uniform(0, 2 * np.pi, k))
    return [float(v) for v in np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1).reshape(-1)]


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
    h = w = a.size
    K, topk, n_gt = 8, 100, 64
    g = np.random.default_rng(0)
    polys = [blob_polygon(g, h, w) for _ in range(n_gt)]
    t0 = time.perf_counter()
    counts = [P.annotation_to_counts([p], h, w) for p in polys]
    host_ms = (time.perf_counter() - t0) * 1e3
    cats = [int(g.integers(0, K)) for _ in range(n_gt)]
    base = [{"category_id": cats[i], "iscrowd": int(i % 9 == 4), "area": float(counts[i][1::2].sum())} for i in range(n_gt)]
    ident = {k: k for k in range(K)}
    gt_poly = ctx.instance_gt_to_device(*IE.gt_rows([dict(b, segmentation=[p]) for b, p in zip(base, polys)], ident, polygons=True, hw=(h, w)))
    gt_rle = ctx.instance_gt_to_device(*IE.gt_rows([dict(b, segmentation={"size": [h, w], "counts": [int(v) for v in c]})
                                                   for b, c in zip(base, counts)], ident))
    masks = np.zeros((topk, h, w), np.uint8)
    for i in range(topk):                                                   # detections: ground-truth masks moved by a few pixels
        m = IE.decode_runs(counts[i % n_gt], h, w)
        masks[i] = np.roll(m, (int(g.integers(-9, 10)), int(g.integers(-9, 10))), (0, 1))
    table = np.zeros(1 + 2 * topk, np.int32)
    table[0] = topk
    table[1 + topk:] = [cats[i % n_gt] for i in range(topk)]
    scores = g.random(topk).astype(np.float32)
    dm, dt, ds = ctx.to_device(masks), ctx.to_device(table), ctx.to_device(scores)
    rows = [ctx.zeros((topk,), IE.ROW_DTYPE) for _ in range(2)]
    n_rows, flags = ctx.zeros((1,), np.int32), ctx.zeros((1,), np.int32)

    def run(gt, out):
        ctx.instance_eval((h, w), dt, ds, topk, gt, K, 0, out, n_rows, flags, masks=dm)

    run(gt_poly, rows[0])
    run(gt_rle, rows[1])
    got = rows[0].numpy()
    assert int(flags.numpy()[0]) == 0 and int(n_rows.numpy()[0]) == topk
    assert got.tobytes() == rows[1].numpy().tobytes(), "polygon and run-length ground truth disagree"
    poly_ms = device_ms(ctx, lambda: run(gt_poly, rows[0]), a.reps)
    rle_ms = device_ms(ctx, lambda: run(gt_rle, rows[1]), a.reps)
    r = {"size": [h, w], "detections": topk, "n_gt": n_gt, "vertices": sum(len(p) // 2 for p in polys), "gt_runs": int(sum(len(c) for c in counts)),
         "instance_eval_poly_ms": round(poly_ms, 4), "instance_eval_rle_ms": round(rle_ms, 4), "poly_over_rle": round(poly_ms / rle_ms, 3),
         "host_reference_ms": round(host_ms, 1), "matched_rows": int(np.count_nonzero(got["matched"])), "reps": a.reps}
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
