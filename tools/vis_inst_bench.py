"""Cost of drawing one instance result and of one semantic record, at 1024x1024 and 1280x1280, 100 instances (discs and boxes of
mixed sizes, heavy overlap) given as dense masks:

  draw_anchors / draw_overlay / draw_both   odise_hip_instance_draw asked for the anchors and the order, for the picture, for all three
                   (dense masks: every variant starts with the same pack of [100, h, w] bytes into words)
  rle              odise_hip_rle_encode on the same dense masks: it shares the pack stage, the yardstick for it
  pack_alone       draw asked for the order only: pack + column counts + rank, the part every variant pays
  semantic_record  odise_hip_semantic_record on a smooth label map of 100 classes (100 x 100 pair cells fit the histogram's LDS)
  pair_histogram   odise_hip_pair_histogram on the same map (as both inputs): the "one pass over the map" yardstick
  host             the numpy restatement of the same drawing (instance_overlay + instance_anchors), one CPU thread

The expectation to confirm or refute: the overlay (about 100 bits and 3 bytes read, 3 bytes written per pixel) costs less than the
pack stage that feeds it (100 bytes read per pixel), i.e. draw_overlay - pack_alone < pack_alone.

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up first); the outputs are compared
with the restatement before they are timed.  Prints one JSON line per size; --out also writes them.

    python tools/vis_inst_bench.py --out profiles/vis_inst_bench.json
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

from odise_amd import visualize as V  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def instance_masks(h, w, n=100, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    masks = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), int(rng.integers(h // 40, h // 5))
        masks[i] = ((y - cy) ** 2 + (x - cx) ** 2 <= r * r) if i % 2 else ((abs(y - cy) <= r) & (abs(x - cx) <= r // 2))
    return masks


def smooth_labels(h, w, K=100, cell=(97, 131), seed=0):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, K, (h // cell[0] + 2, w // cell[1] + 2))
    return np.kron(coarse, np.ones(cell, np.int64))[31:31 + h, 57:57 + w].astype(np.int32)


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def one_size(ctx, h, w, reps):
    n = 100
    masks = instance_masks(h, w, n)
    scores = np.random.default_rng(1).random(n).astype(np.float32)
    image = np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8)
    colors = np.random.default_rng(3).integers(0, 256, (n, 3), dtype=np.uint8)
    edges = V.instance_edge_colors(colors)
    d_masks, d_scores, d_image = ctx.to_device(masks), ctx.to_device(scores), ctx.to_device(image)
    d_colors, d_edges = ctx.to_device(colors), ctx.to_device(edges)
    kw = dict(masks=d_masks, min_score=0.1, image=d_image, colors=d_colors, edge_colors=d_edges, alpha256=128)
    res = ctx.instance_draw((h, w), n, None, d_scores, **kw)

    host = []
    for _ in range(1):
        t0 = time.perf_counter()
        want_pic = V.instance_overlay(image, masks, colors, edges, 128, scores, 0.1)
        want_anchors = V.instance_anchors(masks, scores, 0.1)
        host.append(time.perf_counter() - t0)
    assert res["out"].numpy().tobytes() == want_pic.tobytes(), "device and host pictures disagree"
    assert res["anchors"].numpy().tobytes() == want_anchors.tobytes(), "device and host anchors disagree"
    assert res["order"].numpy().tobytes() == V.instance_order(masks, scores, 0.1).tobytes(), "device and host orders disagree"

    out, anchors, order = res["out"], res["anchors"], res["order"]
    t = {}
    t["draw_anchors"] = device_ms(ctx, lambda: ctx.instance_draw((h, w), n, None, d_scores, want=("anchors", "order"), anchors=anchors, order=order, **kw), reps)
    t["draw_overlay"] = device_ms(ctx, lambda: ctx.instance_draw((h, w), n, None, d_scores, want=("out",), out=out, **kw), reps)
    t["draw_both"] = device_ms(ctx, lambda: ctx.instance_draw((h, w), n, None, d_scores, out=out, anchors=anchors, order=order, **kw), reps)
    t["pack_alone"] = device_ms(ctx, lambda: ctx.instance_draw((h, w), n, None, d_scores, want=("order",), order=order, **kw), reps)
    bufs = (ctx.empty((Context.RLE_BYTES_PER_MASK * n,), np.uint8), ctx.empty((n + 1,), np.int64), ctx.empty((n,), np.int64))
    t["rle"] = device_ms(ctx, lambda: ctx.rle_encode_async(d_masks, bufs=bufs), reps)

    K = 100
    labels = smooth_labels(h, w, K)
    d_labels = ctx.to_device(labels)
    rec = ctx.semantic_record(d_labels, K)
    assert rec.numpy().tobytes() == V.semantic_record(labels, K).tobytes(), "device and host records disagree"
    t["semantic_record"] = device_ms(ctx, lambda: ctx.semantic_record(d_labels, K, rec), reps)
    hist = ctx.zeros((K, K), np.int32)
    t["pair_histogram"] = device_ms(ctx, lambda: ctx.pair_histogram(d_labels, d_labels, K, K, hist), reps)

    r = {"size": [h, w], "instances": n, "kept": int((res["order"].numpy() >= 0).sum())}
    r.update({k + "_ms": round(v, 4) for k, v in t.items()})
    r["overlay_minus_pack_ms"] = round(t["draw_overlay"] - t["pack_alone"], 4)
    r["overlay_costs_less_than_pack"] = bool(t["draw_overlay"] - t["pack_alone"] < t["pack_alone"])
    r["semantic_record_over_histogram"] = round(t["semantic_record"] / t["pair_histogram"], 2)
    r["host_restatement_ms"] = round(min(host) * 1e3, 1)
    r["reps"] = reps
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    lines = []
    for h, w in ((1024, 1024), (1280, 1280)):
        r = one_size(ctx, h, w, a.reps)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
