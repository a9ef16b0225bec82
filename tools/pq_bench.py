"""Cost of one picture of the panoptic evaluator, at 1024x1024 and 1280x1280, smooth synthetic maps with about 30 ground-truth and 20
predicted segments (tests/pq_cases.py):

  fused      odise_hip_panoptic_quality: RGB ground truth (3 bytes per pixel) + panoptic ids (4), id translation, pair counts, matching,
             the add into the statistics - two launches
  histogram  odise_hip_pair_histogram on the same picture as two pre-indexed int32 maps (8 bytes per pixel): the per-pixel pass that existed
             before, which nothing on the device could feed and which stops at the counts - the yardstick.  The expectation to confirm or
             refute: fused stays close to it (the translation and the matching launch cost less than the second 4-byte map).
  host       what the call replaces: the device-to-host copy of the record and panoptic_quality.image_stats (np.unique over 64-bit keys, the
             Python matching loop) on one CPU thread

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up first); the fused result is
compared with the restatement before it is timed.  Prints one JSON line per size; --out also writes them.

    python tools/pq_bench.py --out profiles/pq_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from odise_amd import panoptic_quality as PQ  # noqa: E402
from odise_amd._lib import MAX_SEGMENTS  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402
from pq_cases import blocky_case, slot_map  # noqa: E402


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def one_size(ctx, h, w, reps):
    case = blocky_case(h + w, h, w, 30, 20, cell=(97, 131))
    case.assert_every_rule_fires()
    ref, _ = case.stats()
    rec, rgb = ctx.to_device(case.record(MAX_SEGMENTS)), ctx.to_device(case.rgb())
    stats, flags = ctx.panoptic_quality_record(rec, (h, w), rgb, case.gt_rows, case.C)
    assert stats.numpy().tobytes() == ref.to_records().tobytes() and int(flags.numpy()[0]) == 0, "device and host statistics disagree"
    fused = device_ms(ctx, lambda: ctx.panoptic_quality_record(rec, (h, w), rgb, case.gt_rows, case.C, stats, flags), reps)
    gt_ids = ctx.to_device(case.pan_gt)
    fused_i32 = device_ms(ctx, lambda: ctx.panoptic_quality_record(rec, (h, w), gt_ids, case.gt_rows, case.C, stats, flags), reps)

    na, nb = len(case.gt_rows) + 2, len(case.pred_rows) + 2
    a = ctx.to_device(slot_map(case.pan_gt, case.gt_rows[:, 0]).astype(np.int32).reshape(h, w))
    b = ctx.to_device(slot_map(case.pan_pred, case.pred_rows[:, 0]).astype(np.int32).reshape(h, w))
    hist = ctx.zeros((na, nb), np.int32)
    histogram = device_ms(ctx, lambda: ctx.pair_histogram(a, b, na, nb, hist), reps)
    assert int(hist.numpy().sum()) == (reps + 3) * h * w

    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = rec.numpy()
        t1 = time.perf_counter()
        n = int(got[h * w])
        PQ.image_stats(case.pan_gt, case.gt_rows, got[:h * w], got[h * w + 1:h * w + 1 + 3 * n].reshape(n, 3), case.C)
        host.append((t1 - t0, time.perf_counter() - t1))
    copy_ms, stats_ms = (min(x[k] for x in host) * 1e3 for k in (0, 1))
    return {"size": [h, w], "n_gt": len(case.gt_rows), "n_pred": len(case.pred_rows), "fused_ms": round(fused, 4),
            "fused_int32_gt_ms": round(fused_i32, 4), "pair_histogram_ms": round(histogram, 4), "fused_over_histogram": round(fused / histogram, 3),
            "fused_GBps": round(7 * h * w / fused / 1e6, 1), "histogram_GBps": round(8 * h * w / histogram / 1e6, 1),
            "host_copy_ms": round(copy_ms, 3), "host_image_stats_ms": round(stats_ms, 1), "reps": reps}


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
