"""Cost of one frame of the colour tracker, at 1024x1024 and 1280x1280, smooth synthetic maps of 20 things and 10 stuff segments (a 6 x 5
grid of blocks that drifts two pixels a frame):

  track      odise_hip_track_frame - two launches - in two states of the live list:
             `filled`  nothing ever matches (the categories turn from frame to frame), so after eight warm-up frames the list holds 8 x 20
                       rows and the pixel pass reads all eight retained byte maps next to the new int32 map (12 bytes per pixel + 1 written);
             `steady`  every thing matches its predecessor, so one retained map is live (5 bytes per pixel + 1 written): a clip that tracks.
  histogram  odise_hip_pair_histogram on two consecutive frames as pre-indexed int32 maps (8 bytes per pixel): the bare per-pixel part, the
             yardstick.  The expectation to confirm or refute: a frame costs a small multiple of it, and a fixed per-call cost dominates.
  host       what the call replaces: the device-to-host copy of the record and video.ColorTracker.assign of one frame on a filled list
             (numpy, one CPU thread)

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up first); the colours of the warm-up
frames are compared with the restatement before anything is timed.  Prints one JSON line per size; --out also writes them.

    python tools/track_bench.py --out profiles/track_bench.json
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

from odise_amd import video as VD  # noqa: E402
from odise_amd._lib import MAX_SEGMENTS, record_len, split_record  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402

THINGS, STUFF, WARMUP, PERIOD = 20, 10, 8, 9


def frame(h, w, t, turning):
    """(ids [h,w], table [30,3]) of frame t: blocks of a 6 x 5 grid, ids 1..30, the first 20 things; the picture drifts 2 t pixels."""
    ys, xs = np.arange(h)[:, None] * 5 // h, (np.arange(w)[None, :] + 2 * t) % w * 6 // w
    ids = (1 + ys * 6 + xs).astype(np.int32)
    table = np.array([(k + 1, 1 if k < THINGS else 0, (k + t) % PERIOD if turning and k < THINGS else k % PERIOD) for k in range(THINGS + STUFF)],
                     np.int32)
    return ids, table


def record(ids, table):
    rec = np.zeros(record_len(*ids.shape), np.int32)
    rec[:ids.size], rec[ids.size] = ids.reshape(-1), len(table)
    rec[ids.size + 1:ids.size + 1 + table.size] = table.reshape(-1)
    return rec


def device_ms(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for k in range(reps):
        fn(k)
    return ctx.timer_stop() / reps


def tracked(ctx, h, w, reps, turning):
    """-> (ms per frame, live rows when the timing starts); the warm-up frames are checked against the restatement."""
    frames = [frame(h, w, t, turning) for t in range(PERIOD if turning else 2)]     # the timed calls cycle through these
    recs = [ctx.to_device(record(*f)) for f in frames]
    views = [split_record(r, (h, w)) for r in recs]
    tracker, host = ctx.track_create((h, w)), VD.ColorTracker()
    colors, n_live = ctx.zeros((MAX_SEGMENTS, 3), np.uint8), ctx.zeros((1,), np.int32)
    live = ctx.zeros((8 * MAX_SEGMENTS,), VD.TRACK_ROW_DTYPE)
    for t in range(WARMUP):
        k = t % len(frames)
        ctx.track_frame(tracker, *views[k], colors, live=live, n_live=n_live)
        want = host.assign(*frames[k], np.zeros((THINGS + STUFF, 3), np.uint8))
        assert colors.numpy()[:THINGS + STUFF].tobytes() == want.tobytes(), ("device and host colours disagree", t)
    filled = int(n_live.numpy()[0])
    assert filled == len(host.live) == (WARMUP * THINGS if turning else THINGS), filled
    ms = device_ms(ctx, lambda i: ctx.track_frame(tracker, *views[(WARMUP + i) % len(frames)], colors), reps)
    tracker.close()
    return ms, filled, host, frames, recs


def one_size(ctx, h, w, reps):
    filled_ms, filled_rows, host, frames, recs = tracked(ctx, h, w, reps, True)
    steady_ms, steady_rows, _, _, _ = tracked(ctx, h, w, reps, False)

    n = THINGS + STUFF + 1
    a, b = (ctx.to_device(np.where(f[0] <= THINGS, f[0], 0).astype(np.int32)) for f in frames[:2])      # 0 = no instance, 1 + row
    hist = ctx.zeros((n, n), np.int32)
    for _ in range(3):
        ctx.pair_histogram(a, b, n, n, hist)
    histogram = device_ms(ctx, lambda i: ctx.pair_histogram(a, b, n, n, hist), reps)
    assert int(hist.numpy().sum()) == (reps + 3) * h * w

    runs = []
    for t in range(WARMUP, WARMUP + 3):                                           # the next frames of the filled host tracker
        k = t % len(frames)
        t0 = time.perf_counter()
        got = recs[k].numpy()
        t1 = time.perf_counter()
        host.assign(got[:h * w].reshape(h, w), got[h * w + 1:h * w + 1 + 3 * (THINGS + STUFF)].reshape(-1, 3))
        runs.append((t1 - t0, time.perf_counter() - t1))
    copy_ms, assign_ms = (min(x[k] for x in runs) * 1e3 for k in (0, 1))
    return {"size": [h, w], "things": THINGS, "stuff": STUFF, "track_filled_ms": round(filled_ms, 4), "filled_live_rows": filled_rows,
            "track_steady_ms": round(steady_ms, 4), "steady_live_rows": steady_rows, "pair_histogram_ms": round(histogram, 4),
            "filled_over_histogram": round(filled_ms / histogram, 3), "steady_over_histogram": round(steady_ms / histogram, 3),
            "filled_GBps": round(13 * h * w / filled_ms / 1e6, 1), "steady_GBps": round(6 * h * w / steady_ms / 1e6, 1),
            "histogram_GBps": round(8 * h * w / histogram / 1e6, 1), "host_copy_ms": round(copy_ms, 3), "host_assign_ms": round(assign_ms, 1),
            "reps": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=200)
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
