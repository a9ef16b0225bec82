"""Cost of one whole SemSegEvaluator.process step on the device (odise_hip_semantic_eval), per picture at 1024x1024 and 1280x1280, on smooth
maps (constant rectangles of ~100 pixels a side):

  scores  K = 150 (ADE-150) from the score tensor fp32 [K,H,W]: arg-max once, both confusion matrices, the per-class RLE strings
  labels  K = 847 (ADE-847) from the int32 label map of the fused arg-max: the confusion matrix (719 104 cells: the global-memory side of
          the histogram; no Boundary IoU at 255 classes and more) and the strings

Each is timed with and without the RLE part.  Beside them:
  parent  odise_hip_semantic_boundary_confusion on the same scores from a library built at the PARENT commit (--parent-tree: a checkout of
          it with its library built), parent and result processes alternating, --runs each; the parent's own spread (max - min) is the
          margin a difference has to exceed.
  host    what the RLE part replaces: the copy of the label map to the host plus semseg_eval.encode_json_sem_seg on one CPU thread.

Expectations, written down before the first run:
  (a) with scores the counting part costs no more than the parent's call beyond its spread: the arg-max is still taken once and dominates
      (600 bytes read per pixel against 4 written for the kept labels);
  (b) the RLE part adds less than the counting part costs.
Device times are HIP events around --reps back-to-back calls after a warm-up call.  The timed strings are compared with the host rows.

    python tools/semseg_eval_bench.py --parent-tree _old_tree --out profiles/semseg_eval_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1024, 1024), (1280, 1280))


def blocky(rng, h, w, K, cell):
    small = rng.integers(0, K, (h // cell[0] + 1, w // cell[1] + 1))
    return np.kron(small, np.ones(cell, np.int64))[:h, :w].astype(np.int32)


def inputs(h, w, K):
    rng = np.random.default_rng(h + w + K)
    pred, gt = blocky(rng, h, w, K, (97, 131)), blocky(rng, h, w, K, (113, 89))
    gt[: h // 25, -w // 8:] = K
    return pred, gt


def scores_of(pred, K):
    rng = np.random.default_rng(1)
    sem = rng.random((K,) + pred.shape, dtype=np.float32) * 0.5
    np.put_along_axis(sem, pred[None], 1.0, axis=0)
    return sem


def device_ms(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def worker(tree, side, reps):
    """One process on one library: `tree`'s package and the library built in it."""
    sys.path.insert(0, tree)
    from odise_amd.runtime import Context
    ctx = Context(0)
    out = []
    for h, w in SIZES:
        K = 150
        pred, gt = inputs(h, w, K)
        d_sem, d_gt = ctx.to_device(scores_of(pred, K)), ctx.to_device(gt)
        conf, b_conf = ctx.zeros((K + 1, K + 1), np.int64), ctx.zeros((K + 1, K + 1), np.int64)
        r = {"size": [h, w], "reps": reps}
        r["boundary_confusion_ms"] = round(device_ms(ctx, lambda: ctx.semantic_boundary_confusion(d_sem, d_gt, conf, b_conf), reps), 4)
        if side == "result":
            from odise_amd import semseg_eval as SE

            flags = ctx.zeros((1,), np.int32)
            bufs = (ctx.empty((ctx.sem_rle_bytes((h, w)),), np.uint8), ctx.empty((1 + 847,), np.int32), ctx.empty((2 * 847 + 1,), np.int64))

            def call(p, K, g, c, b, rle):                               # every class may be present: no retry inside the timed loop
                return ctx.semantic_eval_async(p, K, g, conf=c, b_conf=b, flags=flags, rle=rle, max_classes=K, bufs=bufs)
            r["scores_K150_count_ms"] = round(device_ms(ctx, lambda: call(d_sem, K, d_gt, conf, b_conf, False), reps), 4)
            r["scores_K150_count_rle_ms"] = round(device_ms(ctx, lambda: call(d_sem, K, d_gt, conf, b_conf, True), reps), 4)
            classes, rles, _ = call(d_sem, K, d_gt, conf, b_conf, True).result()
            d_lab = ctx.to_device(pred)
            t0 = time.perf_counter()
            rows = SE.encode_json_sem_seg(d_lab.numpy(), "f")
            r["host_copy_and_encode_json_sem_seg_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert SE.rows_from_rle(classes, rles, "f") == rows, "device and host strings disagree (scores)"
            r["scores_K150_classes"], r["scores_K150_string_bytes"] = len(rows), sum(len(x["segmentation"]["counts"]) for x in rows)
            del d_sem
            K = 847
            pred, gt = inputs(h, w, K)
            d_lab, d_gt = ctx.to_device(pred), ctx.to_device(gt)
            big = ctx.zeros((K + 1, K + 1), np.int64)
            r["labels_K847_count_ms"] = round(device_ms(ctx, lambda: call(d_lab, K, d_gt, big, None, False), reps), 4)
            r["labels_K847_count_rle_ms"] = round(device_ms(ctx, lambda: call(d_lab, K, d_gt, big, None, True), reps), 4)
            r["labels_K847_rle_ms"] = round(device_ms(ctx, lambda: call(d_lab, K, None, None, None, True), reps), 4)
            pend = call(d_lab, K, None, None, None, True)
            classes, rles, _ = pend.result()
            assert int(flags.numpy()[0]) == 0
            t0 = time.perf_counter()
            rows = SE.encode_json_sem_seg(d_lab.numpy(), "f")
            r["labels_K847_host_copy_and_encode_json_sem_seg_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            assert SE.rows_from_rle(classes, rles, "f") == rows, "device and host strings disagree (labels)"
            assert np.array_equal(big.numpy(), 2 * (reps + 1) * SE.confusion(pred, gt, K)), "device and host confusion counts disagree"
            r["labels_K847_classes"], r["labels_K847_string_bytes"], r["labels_K847_launches"] = len(rows), sum(len(x["segmentation"]["counts"]) for x in rows), pend.launches
        out.append(r)
    ctx.close()
    print("WORKER " + json.dumps(out), flush=True)


def run_worker(tree, side, reps):
    env = dict(os.environ)
    env.pop("ODISE_HIP_LIB", None)                                   # each tree loads the library built in it
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", side, "--tree", tree, "--reps", str(reps)], capture_output=True, text=True,
                       env=env, timeout=900)
    if p.returncode != 0:
        raise RuntimeError(f"{side} worker failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("WORKER ")][-1]
    return json.loads(line[len("WORKER "):])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with odise_amd/lib/libodise_hip.so built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, choices=("parent", "result"))
    ap.add_argument("--tree", default=HERE)
    a = ap.parse_args()
    if a.worker:
        return worker(os.path.abspath(a.tree), a.worker, a.reps)
    parent, result = [], []
    for _ in range(a.runs):                                          # alternating: drift of the machine lands on both sides
        if a.parent_tree:
            parent.append(run_worker(os.path.abspath(a.parent_tree), "parent", a.reps))
        result.append(run_worker(HERE, "result", a.reps))
    lines = []
    for i, size in enumerate(SIZES):
        res = {k: [run[i][k] for run in result] for k in result[0][i] if k.endswith("_ms")}
        med = {k: float(np.median(v)) for k, v in res.items()}
        line = {"size": list(size), "reps": a.reps, "runs": a.runs, "result": res, "result_median": med,
                "counts": {k: result[0][i][k] for k in result[0][i] if not k.endswith("_ms") and k not in ("size", "reps")}}
        if parent:
            pv = [run[i]["boundary_confusion_ms"] for run in parent]
            spread = round(max(pv) - min(pv), 4)
            pm = float(np.median(pv))
            line["parent"] = {"boundary_confusion_ms": pv, "median": pm, "spread": spread}
            line["expectation_a_counting_no_more_than_parent_beyond_spread"] = {
                "same_call_result_minus_parent_ms": round(med["boundary_confusion_ms"] - pm, 4),
                "semantic_eval_count_minus_parent_ms": round(med["scores_K150_count_ms"] - pm, 4),
                "confirmed": bool(med["scores_K150_count_ms"] - pm <= spread)}
        rle_s = med["scores_K150_count_rle_ms"] - med["scores_K150_count_ms"]
        rle_l = med["labels_K847_count_rle_ms"] - med["labels_K847_count_ms"]
        line["expectation_b_rle_adds_less_than_counting_costs"] = {
            "scores_K150": {"rle_adds_ms": round(rle_s, 4), "counting_ms": med["scores_K150_count_ms"], "confirmed": bool(rle_s < med["scores_K150_count_ms"])},
            "labels_K847": {"rle_adds_ms": round(rle_l, 4), "counting_ms": med["labels_K847_count_ms"], "confirmed": bool(rle_l < med["labels_K847_count_ms"])}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"method": "parent and result processes alternate, --runs each; medians; the parent's spread (max - min) is the margin", "lines": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
