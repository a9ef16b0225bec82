"""What Boundary AP costs beside segm: one picture of the evaluator at 1024x1024, topk 100 against 20 smooth ground truths.

  segm           odise_hip_instance_eval_poly from the mask logits (pack, ground-truth decode, intersections, areas, matching)
  segm_boundary  odise_hip_instance_eval_boundary with the segm and the boundary task: the same, plus the erosion of the topk + n_gt
                 packed masks (csrc/inst_boundary.hip), a second intersection / area pass on the boundary words and a second match walk

The two calls alternate for --runs rounds after a warm-up; a round is HIP events around --reps back-to-back calls on an otherwise idle
context, and the figure is the median over the rounds.  The boundary rows are compared with the host restatement before anything is
timed.  The selection comes from the small synthetic model (tests/small_model.py) with the panoptic head off (the top-k holds exactly 100
masks).  Prints one JSON line; --out also writes it.

    python tools/boundary_ap_bench.py --out profiles/boundary_ap_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from inst_eval_bench import blobs, device_ms  # noqa: E402
from odise_amd import coco_rle as R  # noqa: E402
from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402
from small_model import GROUPS, build_small, image_u8  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--n-gt", type=int, default=20)
    ap.add_argument("--radius", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    hip = build_small(ctx, panoptic_on=False)
    h = w = a.size
    K, topk, n_gt = len(GROUPS), int(hip.test_topk_per_image), a.n_gt
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
    rows = {t: ctx.zeros((topk,), IE.ROW_DTYPE) for t in ("segm", "boundary")}
    n_rows, flags = {t: ctx.zeros((1,), np.int32) for t in ("segm", "boundary")}, ctx.zeros((1,), np.int32)
    itab, isc = sel["inst_table"].view((1 + 2 * topk,), np.int32), sel["inst_scores"].view((topk,), np.float32)
    geom = dict(b=0, pad_hw=sel["pad_hw"], img_hw=sel["img_hw"][0])
    calls = {
        "segm": lambda: ctx.instance_eval((h, w), itab, isc, topk, gt, K, 0, rows["segm"], n_rows["segm"], flags, **geom),
        "segm_boundary": lambda: ctx.instance_eval((h, w), itab, isc, topk, gt, K, 0, rows["segm"], n_rows["segm"], flags,
                                                   boundary=(rows["boundary"], n_rows["boundary"], a.radius), **geom),
    }
    calls["segm_boundary"]()
    counts = [runs[offs[i]:offs[i + 1]] for i in range(n_gt)]
    masks = inst["pred_masks"] > 0.5
    for t in ("segm", "boundary"):
        want, f = IE.image_rows(masks, inst["scores"], inst["pred_classes"], counts, table, 0, num_categories=K, iou_type=t, radius=a.radius)
        assert f == 0 and int(flags.numpy()[0]) == 0 and int(n_rows[t].numpy()[0]) == n == len(want)
        assert rows[t].numpy()[:n].tobytes() == want.tobytes(), f"{t}: device rows and host restatement disagree"
    for fn in calls.values():                                               # warm-up beyond device_ms' own three calls
        device_ms(ctx, fn, a.reps)
    ms = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, fn in calls.items():
            ms[k].append(round(device_ms(ctx, fn, a.reps), 4))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = {"size": [h, w], "detections": n, "n_gt": n_gt, "radius": a.radius if a.radius > 0 else ctx.boundary_radius(h, w), "reps": a.reps,
         "runs": a.runs, "median_ms": med, "min_ms": {k: min(v) for k, v in ms.items()}, "max_ms": {k: max(v) for k, v in ms.items()},
         "boundary_over_segm": round(med["segm_boundary"] / med["segm"], 3),
         "boundary_minus_segm_ms": round(med["segm_boundary"] - med["segm"], 4),
         "matched_rows": {t: int(np.count_nonzero(rows[t].numpy()["matched"])) for t in rows}}
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
