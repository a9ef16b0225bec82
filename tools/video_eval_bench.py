"""Cost of one frame of the video evaluator at 1024x1024, 100 detections (dense uint8 masks) against 20 ground truths:

  frame        odise_hip_video_eval_frame: pack, ground-truth decode, the intersections added through the slot tables, areas
  instance     odise_hip_instance_eval on the same picture: the same pack, decode and intersections, then the match, which the frame
               call leaves to the end of the video
  finish       odise_hip_video_eval_finish of 100 tracks against 20 ground-truth tracks (once per video)

The two per-frame calls share everything but their last step, so `frame` is expected at or below `instance`; the number to read is the
difference.  Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context, warmed up first, the median of
`--repeats` such measurements with their spread beside it; the sums of the timed configuration are compared with the host restatement
before anything is timed.  Prints one JSON line; --out also writes it.

    python tools/video_eval_bench.py --out profiles/video_eval_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from odise_amd import coco_rle as R  # noqa: E402
from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd import video_eval as VE  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    h = w = a.size
    K, topk, n_gt = 4, 100, 20
    g = np.random.default_rng(0)
    masks = np.stack([blobs(h, w, 100 + s) for s in range(topk)])
    gts = [blobs(h, w, s) for s in range(n_gt)]
    anns = [{"category_id": int(s % K), "iscrowd": int(s % 9 == 4), "area": float(m.sum()),
             "segmentation": {"size": [h, w], "counts": R.counts_to_string(R.mask_counts(m))}} for s, m in enumerate(gts)]
    table, runs, offs = IE.gt_rows(anns, {k: k for k in range(K)})
    gt = ctx.instance_gt_to_device(table, runs, offs)
    itab = np.zeros(1 + 2 * topk, np.int32)
    itab[0], itab[1 + topk:] = topk, np.arange(topk) % K
    scores = g.random(topk).astype(np.float32)
    dm, dtab, dsc = ctx.to_device(masks), ctx.to_device(itab), ctx.to_device(scores)
    det_slot, gt_slot = ctx.to_device(g.permutation(topk).astype(np.int32)), ctx.to_device(g.permutation(n_gt).astype(np.int32))
    state = ctx.video_eval_state(topk, n_gt)
    rows, n_rows, flags = ctx.zeros((topk,), IE.ROW_DTYPE), ctx.zeros((1,), np.int32), ctx.zeros((1,), np.int32)

    def frame():
        ctx.video_eval_frame(state, (h, w), topk, det_slot, gt, gt_slot, flags, table_row=dtab, masks=dm)

    def instance():
        ctx.instance_eval((h, w), dtab, dsc, topk, gt, K, 0, rows, n_rows, flags, masks=dm)

    def finish():
        ctx.video_eval_finish(state, topk, dsc, dtab.view((topk,), np.int32, 4 * (1 + topk)), gt["rows"], n_gt, K, 0, rows, n_rows, flags)

    ctx.video_eval_reset(state)
    frame()
    want = VE.Counts(topk, n_gt)
    want.add_frame(masks, det_slot.numpy(), np.stack(gts), gt_slot.numpy())
    inter, area_d, area_g, frames_d = state.numpy()
    assert int(flags.numpy()[0]) == 0 and (inter == want.inter).all() and (area_d == want.area_d).all() and (area_g == want.area_g).all()
    med = lambda v: float(np.median(v))
    fr, ins, fin = (device_ms(ctx, f, a.reps, a.repeats) for f in (frame, instance, finish))
    r = {"size": [h, w], "detections": topk, "n_gt": n_gt, "gt_runs": int(runs.size),
         "video_eval_frame_ms": round(med(fr), 4), "video_eval_frame_ms_runs": [round(x, 4) for x in fr],
         "instance_eval_ms": round(med(ins), 4), "instance_eval_ms_runs": [round(x, 4) for x in ins],
         "frame_minus_instance_ms": round(med(fr) - med(ins), 4),
         "video_eval_finish_ms": round(med(fin), 4), "video_eval_finish_ms_runs": [round(x, 4) for x in fin], "reps": a.reps, "repeats": a.repeats}
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
