"""Cost of one frame of the box colour tracker against the mask tracker it can stand in for, and of drawing with boxes against drawing
without, at 1024x1024 and 1280x1280, 20 and 100 instances a frame - the masks of tools/inst_track_bench.py (discs and boxes that drift two
pixels a frame), dense uint8, ttl 8, every instance matching its predecessor (`steady`) or none (`filled`: the classes turn):

  boxes_track   (a) odise_hip_instance_boxes of the masks, then odise_hip_box_track_frame on the boxes: what a --track-boxes frame adds
  mask_track    (b) odise_hip_inst_track_frame on the same frames
  draw_boxes    (c) odise_hip_instance_draw_boxes (overlay, anchors and order) against odise_hip_instance_draw of the same masks
  box_track     odise_hip_box_track_frame alone: one block

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context after eight warm-up frames.  The colours of
the first frames of the smallest configuration are compared with the restatement before anything is timed.  Prints one JSON line per
configuration; --out also writes them.

    python tools/box_track_bench.py --out profiles/box_track_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from inst_track_bench import PERIOD, TTL, WARMUP, device_ms, instance_masks, table_of  # noqa: E402
from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd import video as VD  # noqa: E402
from odise_amd import visualize as V  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def one(ctx, h, w, n, reps, check):
    host_masks = [instance_masks(h, w, n, 2 * t) for t in range(2)]
    masks = [ctx.to_device(m) for m in host_masks]
    scores = ctx.to_device(np.full(n, 0.9, np.float32))
    base = np.arange(n) % PERIOD
    turning = [ctx.to_device(table_of(n, (base + t) % PERIOD)) for t in range(PERIOD)]
    colors, boxes = ctx.zeros((n, 3), np.uint8), ctx.zeros((n, 4), np.float32)
    out = {"size": [h, w], "instances": n, "ttl": TTL, "reps": reps}

    for state in ("filled", "steady"):
        frame = (lambda t: (masks[0], turning[t % PERIOD])) if state == "filled" else (lambda t: (masks[t % 2], turning[0]))
        btrk, mtrk, host = ctx.box_track_create(n, TTL), ctx.inst_track_create((h, w), n, TTL), VD.BoxColorTracker(TTL)

        def box_frame(t):
            m, tab = frame(t)
            ctx.instance_boxes((h, w), n, tab, masks=m, boxes=boxes)
            ctx.box_track_frame(btrk, boxes, tab, scores, 0.5, colors)

        for t in range(WARMUP):
            box_frame(t)
            ctx.inst_track_frame(mtrk, frame(t)[1], scores, masks=frame(t)[0], min_score=0.5)
            if check and t < 3:
                hm = host_masks[0] if state == "filled" else host_masks[t % 2]
                want = host.assign((base + t) % PERIOD if state == "filled" else base, np.full(n, 0.9, np.float32), IE.mask_boxes(hm), 0.5)
                assert colors.numpy().tobytes() == want.tobytes(), ("device and host colours disagree", state, t)
        out[f"boxes_track_{state}_ms"] = round(device_ms(ctx, lambda i: box_frame(WARMUP + i), reps), 4)
        out[f"box_track_{state}_ms"] = round(device_ms(ctx, lambda i: ctx.box_track_frame(btrk, boxes, frame(WARMUP + i)[1], scores, 0.5, colors), reps), 4)
        out[f"mask_track_{state}_ms"] = round(device_ms(ctx, lambda i: ctx.inst_track_frame(mtrk, frame(WARMUP + i)[1], scores, masks=frame(WARMUP + i)[0],
                                                                                              min_score=0.5, colors=colors), reps), 4)
        out[f"{state}_mask_over_boxes"] = round(out[f"mask_track_{state}_ms"] / out[f"boxes_track_{state}_ms"], 2)
        btrk.close()
        mtrk.close()

    image = ctx.to_device(np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8))
    edges = ctx.to_device(V.instance_edge_colors(colors.numpy()))
    kw = dict(table_row=turning[0], scores_row=scores, min_score=0.5, image=image, colors=colors, edge_colors=edges)
    res = ctx.instance_draw((h, w), n, masks=masks[0], **kw)
    keep = dict(out=res["out"], anchors=res["anchors"], order=res["order"])
    ctx.instance_boxes((h, w), n, turning[0], masks=masks[0], boxes=boxes)
    bw = V.default_box_width(h, w)
    out["instance_draw_ms"] = round(device_ms(ctx, lambda i: ctx.instance_draw((h, w), n, masks=masks[0], **kw, **keep), reps), 4)
    out["instance_draw_boxes_ms"] = round(device_ms(ctx, lambda i: ctx.instance_draw_boxes((h, w), n, boxes, bw, 128, 1000, masks=masks[0], **kw, **keep), reps), 4)
    out["box_width"] = bw
    out["draw_boxes_over_draw"] = round(out["instance_draw_boxes_ms"] / out["instance_draw_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    lines = []
    for h, w in ((1024, 1024), (1280, 1280)):
        for n in (20, 100):
            r = one(ctx, h, w, n, a.reps, check=(h, n) == (1024, 20))
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
