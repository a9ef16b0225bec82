"""Cost of one frame of the instance-mask colour tracker (odise_hip_inst_track_frame), at 1024x1024 and 1280x1280, 20 and 100 smooth
synthetic instances a frame (discs and boxes that drift two pixels a frame), dense uint8 masks, ttl 8:

  track      odise_hip_inst_track_frame - pack, areas, gathered intersection, match - in two states of the live list:
             `filled`  nothing ever matches (the classes turn from frame to frame with period 9), so after eight warm-up frames the list
                       holds 8 x n rows and no tile leaves on the class test: 8 n x n pairs over w * ceil(h / 64) words each;
             `steady`  every instance matches its predecessor, so the list holds n rows: a clip that tracks.
  draw       odise_hip_instance_draw (overlay, anchors and order) of the same masks: the call the tracker's colours feed.
  panoptic   odise_hip_track_frame on a comparable panoptic record (n things in a grid that drifts two pixels a frame, steady).

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up first).  The colours of the first
frames of the smallest configuration are compared with the restatement before anything is timed.  Prints one JSON line per configuration;
--out also writes them.

    python tools/inst_track_bench.py --out profiles/inst_track_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from odise_amd import video as VD  # noqa: E402
from odise_amd import visualize as V  # noqa: E402
from odise_amd._lib import MAX_SEGMENTS, record_len, split_record  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402

TTL, WARMUP, PERIOD = 8, 8, 9


def instance_masks(h, w, n, shift, seed=0):
    """uint8 [n,h,w]: discs and boxes of the seed, moved `shift` pixels to the right"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    masks = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cy, cx, r = int(rng.integers(0, h)), int(rng.integers(0, w)) + shift, int(rng.integers(h // 40, h // 5))
        masks[i] = ((y - cy) ** 2 + (x - cx) ** 2 <= r * r) if i % 2 else ((abs(y - cy) <= r) & (abs(x - cx) <= r // 2))
    return masks


def table_of(n, classes):
    t = np.zeros(1 + 2 * n, np.int32)
    t[0] = n
    t[1 + n:] = classes
    return t


def panoptic_record(h, w, n, t):
    g = int(np.ceil(np.sqrt(n)))
    ys, xs = np.arange(h)[:, None] * g // h, (np.arange(w)[None, :] + 2 * t) % w * g // w
    ids = np.minimum(1 + ys * g + xs, n).astype(np.int32)
    rec = np.zeros(record_len(h, w), np.int32)
    rec[:h * w], rec[h * w] = ids.reshape(-1), n
    rec[h * w + 1:h * w + 1 + 3 * n] = np.array([(k + 1, 1, k % PERIOD) for k in range(n)], np.int32).reshape(-1)
    return rec


def device_ms(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for k in range(reps):
        fn(k)
    return ctx.timer_stop() / reps


def one(ctx, h, w, n, reps, check):
    host_masks = [instance_masks(h, w, n, 2 * t) for t in range(2)]
    masks = [ctx.to_device(m) for m in host_masks]
    scores = ctx.to_device(np.full(n, 0.9, np.float32))
    base = np.arange(n) % PERIOD
    turning = [ctx.to_device(table_of(n, (base + t) % PERIOD)) for t in range(PERIOD)]
    colors, n_live = ctx.zeros((n, 3), np.uint8), ctx.zeros((1,), np.int32)
    live = ctx.zeros((8 * MAX_SEGMENTS,), VD.TRACK_ROW_DTYPE)
    out = {"size": [h, w], "instances": n, "ttl": TTL, "reps": reps}

    for state in ("filled", "steady"):
        trk, host = ctx.inst_track_create((h, w), n, TTL), VD.InstanceColorTracker(TTL)
        frame = (lambda t: (masks[0], turning[t % PERIOD])) if state == "filled" else (lambda t: (masks[t % 2], turning[0]))
        for t in range(WARMUP):
            m, tab = frame(t)
            ctx.inst_track_frame(trk, tab, scores, masks=m, min_score=0.5, colors=colors, live=live, n_live=n_live)
            if check and t < 3:
                hm = host_masks[0] if state == "filled" else host_masks[t % 2]
                want = host.assign((base + t) % PERIOD if state == "filled" else base, np.full(n, 0.9, np.float32), hm, 0.5)
                assert colors.numpy().tobytes() == want.tobytes(), ("device and host colours disagree", state, t)
        rows = int(n_live.numpy()[0])
        assert n <= rows <= WARMUP * n, (state, rows)   # reported: two different shapes of one class may match by chance
        ms = device_ms(ctx, lambda i: ctx.inst_track_frame(trk, frame(WARMUP + i)[1], scores, masks=frame(WARMUP + i)[0], min_score=0.5, colors=colors), reps)
        out[f"track_{state}_ms"], out[f"{state}_live_rows"] = round(ms, 4), rows
        trk.close()

    image = ctx.to_device(np.random.default_rng(2).integers(0, 256, (h, w, 3), dtype=np.uint8))
    edges = ctx.to_device(V.instance_edge_colors(colors.numpy()))
    res = ctx.instance_draw((h, w), n, turning[0], scores, masks=masks[0], min_score=0.5, image=image, colors=colors, edge_colors=edges)
    out["instance_draw_ms"] = round(device_ms(ctx, lambda i: ctx.instance_draw((h, w), n, turning[0], scores, masks=masks[i % 2], min_score=0.5, image=image,
                                                                               colors=colors, edge_colors=edges, out=res["out"], anchors=res["anchors"],
                                                                               order=res["order"]), reps), 4)

    recs = [split_record(ctx.to_device(panoptic_record(h, w, n, t)), (h, w)) for t in range(2)]
    ptrk, pcolors = ctx.track_create((h, w), TTL), ctx.zeros((MAX_SEGMENTS, 3), np.uint8)
    for t in range(WARMUP):
        ctx.track_frame(ptrk, *recs[t % 2], pcolors)
    out["panoptic_track_ms"] = round(device_ms(ctx, lambda i: ctx.track_frame(ptrk, *recs[i % 2], pcolors), reps), 4)
    ptrk.close()
    out["filled_over_draw"] = round(out["track_filled_ms"] / out["instance_draw_ms"], 2)
    out["steady_over_draw"] = round(out["track_steady_ms"] / out["instance_draw_ms"], 2)
    out["steady_over_panoptic"] = round(out["track_steady_ms"] / out["panoptic_track_ms"], 2)
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
