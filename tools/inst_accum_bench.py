"""Cost of COCOeval.accumulate for the segm evaluator, on the device (odise_hip_instance_accumulate) and on the host
(instance_eval.accumulate), on three sets of random rows - 100 per picture, random categories, scores, match and ignore bits, a fixed seed:

    200 pictures,  K = 80     20 k rows
    2000 pictures, K = 100    200 k rows   (ADE val)
    5000 pictures, K = 80     500 k rows   (COCO val)
    the last again with a quarter of the rows in one category (COCO's `person` is about that)

The rows lie on the device in the evaluator's layout (blocks of 64 pictures).  Device times are HIP events around `--reps` back-to-back
calls on an otherwise idle context, warmed up first (the read-back of the result is not in them; it is 7.8 MB at K = 80); the host time is
one call of the numpy function on the same rows, on the same machine.  The result of the timed configuration is compared with the
host's, byte for byte, before anything is timed.

The expectation to confirm or correct, written down before the first run: sorting 500 k keys (five 8-bit passes over 12-byte pairs) and
walking the rows a few times is a few hundred MB of traffic, so the call should take single-digit milliseconds - at least a hundred
times less than the host's 1.7 s.  The cell stage gives a category to 12 blocks of 10 waves, each of which walks the category's rows
64 at a time, so its time follows the LONGEST category, not the row count: uniform random categories are its best case.
Prints one JSON line; --out also writes it.

    python tools/inst_accum_bench.py --out profiles/inst_accum_bench.json
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

from odise_amd import instance_eval as IE  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402

SETS = ((200, 80, 0.0), (2000, 100, 0.0), (5000, 80, 0.0), (5000, 80, 0.25))      # pictures, K, share of category 0 beyond its draw
TOPK, CHUNK = 100, 64


def rows_of(pictures: int, K: int, seed: int, skew: float = 0.0):
    """-> (blocks [(rows [CHUNK * TOPK], counts [CHUNK])], compact rows, npig)"""
    g = np.random.default_rng(seed)
    rows = np.zeros((pictures, TOPK), IE.ROW_DTYPE)
    rows["score"] = -np.sort(-g.random((pictures, TOPK), np.float32), axis=1)
    rows["category"] = np.where(g.random((pictures, TOPK)) < skew, 0, g.integers(0, K, (pictures, TOPK)))
    rows["area"] = g.integers(1, 1 << 18, (pictures, TOPK))
    rows["image"] = np.arange(pictures)[:, None]
    rows["matched"] = g.integers(0, 1 << 40, (pictures, TOPK), dtype=np.uint64)
    rows["ignored"] = g.integers(0, 1 << 40, (pictures, TOPK), dtype=np.uint64) & g.integers(0, 1 << 40, (pictures, TOPK), dtype=np.uint64)
    npig = np.maximum(1, (np.bincount(rows["category"].reshape(-1), minlength=K)[:, None] * g.uniform(0.3, 0.6, (K, 4))).astype(np.int64))
    blocks = []
    for p0 in range(0, pictures, CHUNK):
        part = rows[p0:p0 + CHUNK]
        padded = np.zeros((CHUNK, TOPK), IE.ROW_DTYPE)
        padded[:len(part)] = part
        counts = np.zeros(CHUNK, np.int32)
        counts[:len(part)] = TOPK
        blocks.append((padded.reshape(-1), counts))
    return blocks, rows.reshape(-1), npig


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    sets = []
    for pictures, K, skew in SETS:
        blocks, rows, npig = rows_of(pictures, K, seed=pictures + K, skew=skew)
        dev = [(ctx.to_device(r), ctx.to_device(c)) for r, c in blocks]
        t0 = time.perf_counter()
        want = IE.accumulate(rows, npig, K)
        host_s = time.perf_counter() - t0
        got = ctx.instance_accumulate(dev, npig, K, TOPK)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), "device and host disagree"
        # the bare call, on buffers that stay: what the evaluator's call costs without the read-back
        import ctypes as C
        from odise_amd._lib import InstAccumDesc, check
        npig_d, thr_d = ctx.to_device(npig), ctx.to_device(IE.REC_THRS)
        precision, recall, flags = ctx.empty(want[0].shape, np.float64), ctx.empty(want[1].shape, np.float64), ctx.zeros((1,), np.int32)
        rp, cp = (C.c_void_p * len(dev))(*[r.ptr for r, _ in dev]), (C.c_void_p * len(dev))(*[c.ptr for _, c in dev])
        sl = (C.c_int32 * len(dev))(*[CHUNK] * len(dev))
        d = InstAccumDesc()
        d.n_blocks, d.rows, d.counts, d.slots = len(dev), C.addressof(rp), C.addressof(cp), C.addressof(sl)
        d.topk, d.num_categories, d.npig, d.rec_thrs, d.n_rec = TOPK, K, npig_d.ptr, thr_d.ptr, len(IE.REC_THRS)
        d.precision, d.recall, d.flags = precision.ptr, recall.ptr, flags.ptr

        def call():
            check(ctx.lib.odise_hip_instance_accumulate(ctx.h, C.byref(d)), "instance_accumulate")

        for _ in range(3):
            call()
        ctx.sync()
        ctx.timer_start()
        for _ in range(a.reps):
            call()
        ms = ctx.timer_stop() / a.reps
        assert precision.numpy().tobytes() == want[0].tobytes() and int(flags.numpy()[0]) == 0
        t0 = time.perf_counter()
        ctx.instance_accumulate(dev, npig, K, TOPK)
        call_ms = (time.perf_counter() - t0) * 1e3
        sets.append({"pictures": pictures, "K": K, "rows": int(rows.size), "longest_category": int(np.bincount(rows["category"]).max()),
                     "device_ms": round(ms, 4), "device_call_with_readback_ms": round(call_ms, 3), "host_ms": round(host_s * 1e3, 1),
                     "host_over_device": round(host_s * 1e3 / ms, 1)})
    r = {"sets": sets, "reps": a.reps, "expectation": "single-digit milliseconds at 500 k rows; the skewed set slower than the uniform one",
         "expectation_held": bool(max(x["device_ms"] for x in sets) < 10.0)}
    print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
