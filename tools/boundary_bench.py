"""Cost of one SemSegEvaluator.process step with the Boundary IoU counters, per picture at K = 150 (ADE-150), 1024x1024 and 1280x1280:

  fused     odise_hip_semantic_boundary_confusion: arg-max + confusion counts + both boundary maps + boundary confusion counts
  parent    odise_hip_semantic_confusion on the same inputs: the arg-max sweep (4 K bytes per pixel) and the confusion counts alone - the
            yardstick.  The two erosions touch a few bytes per pixel per pass, so fused / parent far above 1 would mean the minimum filter
            pays per pixel for its radius.
  boundary  odise_hip_label_boundary of the int32 ground truth alone (pack + minimum passes + unpack of ONE map)

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context.  The label maps are smooth (constant
rectangles of ~100 pixels a side), the scores one-hot plus noise below the winner; the timed result is compared with the host restatement
(odise_amd/sem_boundary.py), whose time on one CPU thread is recorded beside it.  Prints one JSON line per size; --out also writes them.

    python tools/boundary_bench.py --out profiles/boundary_bench.json
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

from odise_amd import sem_boundary as S  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def blocky(rng, h, w, K, cell):
    small = rng.integers(0, K, (h // cell[0] + 1, w // cell[1] + 1))
    return np.kron(small, np.ones(cell, np.int64))[:h, :w].astype(np.int32)


def device_ms(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def one_size(ctx, h, w, K, reps):
    rng = np.random.default_rng(h + w)
    pred, gt = blocky(rng, h, w, K, (97, 131)), blocky(rng, h, w, K, (113, 89))
    gt[: h // 25, -w // 8:] = 255
    sem = (rng.random((K, h, w), dtype=np.float32) * 0.5)
    np.put_along_axis(sem, pred[None], 1.0, axis=0)
    d_sem, d_gt = ctx.to_device(sem), ctx.to_device(gt)
    del sem
    n = K + 1
    conf, b_conf, conf_p = (ctx.zeros((n, n), np.int64) for _ in range(3))
    out = ctx.empty((h, w), np.int32)
    fused = device_ms(ctx, lambda: ctx.semantic_boundary_confusion(d_sem, d_gt, conf, b_conf), reps)
    parent = device_ms(ctx, lambda: ctx.semantic_confusion(d_sem, d_gt, conf_p), reps)
    only_b = device_ms(ctx, lambda: ctx.semantic_boundary_confusion(d_sem, d_gt, None, b_conf), reps)
    boundary = device_ms(ctx, lambda: ctx.label_boundary(d_gt, K, out=out), reps)
    t0 = time.perf_counter()
    ref_b = S.boundary_confusion(pred, gt, K)
    host_ms = (time.perf_counter() - t0) * 1e3
    calls = reps + 1
    assert np.array_equal(conf.numpy(), conf_p.numpy()), "fused and parent confusion counts disagree"
    assert np.array_equal(b_conf.numpy(), 2 * calls * ref_b), "device and host boundary counts disagree"
    assert np.array_equal(out.numpy(), S.mask_to_boundary(S.clamp_labels(gt, K))), "device and host boundary maps disagree"
    return {"size": [h, w], "K": K, "radius": ctx.boundary_radius(h, w), "fused_ms": round(fused, 4), "parent_confusion_ms": round(parent, 4),
            "fused_over_parent": round(fused / parent, 3), "fused_without_conf_ms": round(only_b, 4), "label_boundary_ms": round(boundary, 4),
            "host_numpy_boundary_confusion_ms": round(host_ms, 1), "boundary_pixels": int(h * w - ref_b[0, 0]), "reps": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    lines = []
    for h, w in ((1024, 1024), (1280, 1280)):
        r = one_size(ctx, h, w, 150, a.reps)
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
