"""Cost of the segm evaluator's per-mask work for one picture's instance selection (topk = 100) at 1024x1024 and 1024x1536:

  fused   odise_hip_instance_rle: the COCO RLE strings straight from the mask logits (rle.hip pack / count / offsets / write)
  x4      odise_hip_instance_masks (instance_masks_x4_kernel, the fp32 [n, oh, ow] masks of the default path) + the D2H copy of that
          tensor, which detectron2's instances_to_coco_json starts from
  host    odise_amd.coco_rle.encode of the same masks on the CPU (pycocotools' algorithm in numpy; pycocotools itself is C)

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context; the copy and the host encoder are host clocks.
The timed RLE calls get a string buffer of the size the first (untimed) call reported, so every timed call writes its strings.
The selection comes from the small synthetic model (tests/small_model.py) with the panoptic head off (20 queries x 11 classes = 220
candidates: the top-k holds exactly 100 masks).  Its random weights make noise-like masks (about one run per ten pixels), far more runs
than a trained model's blobs; the count / write passes grow with the runs, so the same passes are also timed on 100 smooth masks
(random ellipses) through odise_hip_rle_encode ("smooth_*").  Prints one JSON line per size; --out also writes them to a file.

    python tools/rle_bench.py --out rle_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from odise_amd import coco_rle as R  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402
from small_model import build_small, image_u8  # noqa: E402


def blobs(h, w, seed):
    """A smooth mask: the union of three random ellipses."""
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y, x = np.ogrid[:h, :w]
    for _ in range(3):
        cy, cx, ry, rx = g.integers(0, h), g.integers(0, w), g.integers(16, h // 3), g.integers(16, w // 3)
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


def device_ms(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def one_size(ctx, hip, h, w, reps):
    topk = hip.test_topk_per_image
    res = hip.forward([{"image": image_u8(h, w, seed=h + w)}])[0]["instances"]     # default path: the fp32 masks and the table of this picture
    n = len(res["scores"])
    table = hip._pool[("inst_table", np.dtype(np.int32).str)].view((1 + 2 * topk,), np.int32)
    pad = (-(-h // 64) * 64, -(-w // 64) * 64)

    def timed_bufs(pending_fn):
        """Buffers that hold every string: sized by a first call's offsets[n] (its retry), so no timed call skips the write pass."""
        rles, _ = pending_fn(None).result()
        need = sum(len(r["counts"]) for r in rles)
        return (ctx.empty((max(need, 1),), np.uint8), ctx.empty((topk + 1,), np.int64), ctx.empty((topk,), np.int64)), need

    fused_call = lambda b: ctx.instance_rle_async(0, table, topk, pad, (h, w), (h, w), bufs=b)   # noqa: E731
    bufs, need = timed_bufs(fused_call)
    fused = device_ms(ctx, lambda: fused_call(bufs), reps)
    pend = fused_call(bufs)
    rles, area = pend.result()
    assert int(pend.off.numpy()[-1]) == need <= bufs[0].nbytes     # the timed configuration wrote the strings (no retry)
    out = ctx.empty((n, h, w), np.float32)
    idx = table.ptr + 4   # the selected query indices follow the count
    x4 = device_ms(ctx, lambda: ctx.lib.odise_hip_instance_masks(ctx.h, 0, C.c_void_p(idx), n, pad[0], pad[1], h, w, h, w, out.ptr), reps)
    ctx.sync()
    t0 = time.perf_counter()
    masks = out.numpy()
    d2h = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = [R.encode(m) for m in masks]
    host_ms = (time.perf_counter() - t0) * 1e3
    assert rles == host and np.array_equal(masks, res["pred_masks"]), "fused RLE and host encoder disagree"
    rle_bytes = sum(len(r["counts"]) for r in rles)
    smooth = np.stack([blobs(h, w, s) for s in range(topk)])
    sdev = ctx.to_device(smooth)
    smooth_call = lambda b: ctx.rle_encode_async(sdev, bufs=b)   # noqa: E731
    sbufs, sneed = timed_bufs(smooth_call)
    smooth_ms = device_ms(ctx, lambda: smooth_call(sbufs), reps)
    spend = smooth_call(sbufs)
    srles, _ = spend.result()
    assert int(spend.off.numpy()[-1]) == sneed <= sbufs[0].nbytes
    assert srles[:5] == [R.encode(m) for m in smooth[:5]]
    return {"size": [h, w], "masks": n, "fused_rle_ms": round(fused, 4), "x4_masks_ms": round(x4, 4), "d2h_ms": round(d2h, 3),
            "x4_plus_d2h_ms": round(x4 + d2h, 3), "host_encode_ms": round(host_ms, 1), "mask_tensor_bytes": int(masks.nbytes),
            "rle_bytes": int(rle_bytes), "mean_runs_per_mask": round(float(np.mean([len(R.string_to_counts(r["counts"])) for r in rles[:10]])), 1),
            "area_checksum": int(area.sum()), "smooth_masks": topk, "smooth_rle_encode_u8_ms": round(smooth_ms, 4),
            "smooth_rle_bytes": int(sum(len(r["counts"]) for r in srles)),
            "smooth_mean_runs_per_mask": round(float(np.mean([len(R.string_to_counts(r["counts"])) for r in srles])), 1), "reps": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    hip = build_small(ctx, panoptic_on=False)
    lines = []
    for h, w in ((1024, 1024), (1024, 1536)):
        r = one_size(ctx, hip, h, w, a.reps)
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
