"""Cost of the semantic PQ statistics beside the evaluator step: one picture of odise_hip_semantic_eval_pq of this tree against
odise_hip_semantic_eval of the PARENT commit's library on the same inputs - K = 150 and K = 847 at 1024x1024 and 1280x1280, smooth maps
of ~100-pixel rectangles (the maps of tools/semseg_eval_bench.py), from the int32 label map and from a one-hot score tensor.  Two forms
of the step: `count` (the confusion matrix, and the boundary matrix for K <= 254) and `step` (the same plus the per-class RLE strings,
what HipSemSegEvaluator.process enqueues).  `--reps` calls between HIP events after a warm-up, on an otherwise idle context.

The two libraries alternate, `--runs` runs each, every run in a process of its own (a process loads one library); the parent's own
spread (max - min of its runs) is the margin a difference has to exceed to mean anything.  This tree's plain call is timed as well: it
is the parent's code and should sit inside that margin.  The added work is one more read of the two int32 maps and two small launches.

    python -m odise_amd.build                                   # this tree
    (build the parent commit's tree the same way, elsewhere)
    python tools/semseg_pq_bench.py --parent-lib /path/to/parent/libodise_hip.so --out profiles/semseg_pq_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1024, 1024), (1280, 1280))
KS = (150, 847)


def blocky(rng, h, w, K, cell):
    small = rng.integers(0, K, (h // cell[0] + 1, w // cell[1] + 1))
    return np.kron(small, np.ones(cell, np.int64))[:h, :w].astype(np.int32)


def inputs(h, w, K):
    rng = np.random.default_rng(h + w + K)
    pred, other = blocky(rng, h, w, K, (97, 131)), blocky(rng, h, w, K, (113, 89))
    gt = np.where(blocky(rng, h, w, 2, (113, 89)) == 1, pred, other).astype(np.int32)   # about half the cells agree: matches, fn and fp all occur
    gt[: h // 25, -w // 8:] = K
    return pred, gt


def one_hot_scores(ctx, pred, K):
    """float32 [K,h,w] on the device with 1.0 at the label and 0.0 elsewhere, uploaded plane by plane (only the planes of present classes)."""
    from odise_amd._lib import check
    h, w = pred.shape
    sem = ctx.zeros((K, h, w), np.float32)
    ctx.sync()
    for k in np.unique(pred):
        plane = np.ascontiguousarray((pred == k).astype(np.float32))
        check(ctx.lib.odise_hip_memcpy_h2d(ctx.h, C.c_void_p(sem.ptr + int(k) * h * w * 4), plane.ctypes.data_as(C.c_void_p), C.c_size_t(plane.nbytes)), "memcpy_h2d")
    return sem


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def leg(lib_path, reps):
    """One process, one library: {"HxW_K_route": {"count_ms", "step_ms", and with the new call "count_pq_ms", "step_pq_ms"}}."""
    from odise_amd._lib import load
    lib = load(lib_path, allow_missing=True)   # the parent's library lacks the new calls; the first load decides for the process
    from odise_amd import semseg_pq as SP
    from odise_amd.panoptic_quality import STAT_DTYPE, PQStats
    from odise_amd.runtime import Context
    ctx = Context(0)
    has_pq = hasattr(lib, "odise_hip_semantic_eval_pq")
    out = {}
    for h, w in SIZES:
        for K in KS:
            pred, gt = inputs(h, w, K)
            d_gt, d_lab = ctx.to_device(gt), ctx.to_device(pred)
            want = SP.picture_stats(pred, gt, K)[0] if has_pq else None
            for route in ("labels", "scores"):
                d_pred = d_lab if route == "labels" else one_hot_scores(ctx, pred, K)
                conf = ctx.zeros((K + 1, K + 1), np.int64)
                b_conf = ctx.zeros((K + 1, K + 1), np.int64) if K <= 254 else None
                flags = ctx.zeros((1,), np.int32)
                bufs = (ctx.empty((ctx.sem_rle_bytes((h, w)),), np.uint8), ctx.empty((1 + K,), np.int32), ctx.empty((2 * K + 1,), np.int64))

                def call(rle, stats=None):                                   # every class may be present: no retry inside the timed loop
                    kw = {"pq_stats": stats} if stats is not None else {}
                    return ctx.semantic_eval_async(d_pred, K, d_gt, conf=conf, b_conf=b_conf, flags=flags, rle=rle, max_classes=K, bufs=bufs, **kw)
                r = {"count_ms": device_ms(ctx, lambda: call(False), reps), "step_ms": device_ms(ctx, lambda: call(True), reps)}
                if has_pq:
                    stats = ctx.zeros((K,), STAT_DTYPE)
                    p = call(True, stats)
                    assert p.launches == 1 and PQStats.from_records(stats.numpy()) == want and int(flags.numpy()[0]) == 0, "device and host statistics disagree"
                    r["tp"], r["fp"], r["fn"] = int(want.tp.sum()), int(want.fp.sum()), int(want.fn.sum())
                    r["count_pq_ms"] = device_ms(ctx, lambda: call(False, stats), reps)
                    r["step_pq_ms"] = device_ms(ctx, lambda: call(True, stats), reps)
                out[f"{h}x{w}_K{K}_{route}"] = r
                del d_pred
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-lib", required=True, help="libodise_hip.so built from the parent commit")
    ap.add_argument("--lib", default=os.path.join(ROOT, "odise_amd", "lib", "libodise_hip.so"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        print("LEG " + json.dumps(leg(a.leg, a.reps)), flush=True)
        return
    runs = {"parent": [], "this": []}
    for _ in range(a.runs):
        for name, path in (("parent", a.parent_lib), ("this", a.lib)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-lib", a.parent_lib, "--reps", str(a.reps), "--leg", path],
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"{name} leg failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[name].append(json.loads(next(l for l in p.stdout.splitlines() if l.startswith("LEG "))[4:]))
    med = statistics.median
    lines = []
    for key in runs["this"][0]:
        size, K, route = key.split("_")
        line = {"size": [int(v) for v in size.split("x")], "K": int(K[1:]), "from": route, "reps": a.reps,
                **{k: runs["this"][0][key][k] for k in ("tp", "fp", "fn")}}
        for form in ("count", "step"):
            parent = [r[key][form + "_ms"] for r in runs["parent"]]
            plain = [r[key][form + "_ms"] for r in runs["this"]]
            pq = [r[key][form + "_pq_ms"] for r in runs["this"]]
            line.update({f"parent_{form}_ms": [round(v, 4) for v in parent], f"parent_{form}_spread_ms": round(max(parent) - min(parent), 4),
                         f"this_{form}_ms": [round(v, 4) for v in plain], f"this_{form}_pq_ms": [round(v, 4) for v in pq],
                         f"{form}_over_parent": round(med(plain) / med(parent), 3), f"{form}_pq_over_parent": round(med(pq) / med(parent), 3),
                         f"{form}_pq_minus_parent_ms": round(med(pq) - med(parent), 4)})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
