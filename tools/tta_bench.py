"""Kernel time of odise_hip_tta_finish (arg-max form, csrc/tta.hip) against the existing single-view semantic_argmax_kernel on the same
picture, at K = 150 / 1024 x 1024 and K = 847 / 1280 x 1280, 100 queries, for A = 1, 2 and 6 views.

  single   semantic_argmax_kernel (a pixel's whole S row in registers) on the operands of a one-view handle: the yardstick.  It is reached
           through odise_hip_lab_tta_single_argmax, which exists in the measurement build only:
               python -m odise_amd.build --tools && ODISE_HIP_LIB=odise_amd/lib/libodise_hip_tools.so python tools/tta_bench.py --out ...
  finish   tta_finish_kernel on a handle of A views (the depth A x 104 walked from memory, 5 or 6 class tiles of accumulators a pass)

At A = 1 both read the same S and PT bits and their arg-max maps are compared bit for bit before anything is timed.  The expectation to
confirm or refute: `finish` at A = 1 within the run-to-run spread of `single`, and time roughly proportional to the depth for A > 1.

Times are HIP events around `--reps` back-to-back launches on an otherwise idle context, after warm-up launches of the same shape; every
figure is taken `--rounds` times, the two kernels of A = 1 alternating round by round, and the JSON line holds the median and the
(min, max) of the rounds: the spread.  The views are smooth random fields through odise_hip_set_head_masks (no network runs).

    python tools/tta_bench.py --out profiles/tta_bench.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from odise_amd._lib import check  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402

Q, WARMUP = 100, 3
SHAPES = ((150, 1024), (847, 1280))     # (classes, side of the square picture)
VIEWS = (1, 2, 6)


def category_head(ctx):
    """A 16-wide category head: the classification stage has to exist before a vocabulary can be set (as in tests/test_gpu_tta.py)."""
    rng = np.random.default_rng(11)
    for key, arr in (("category_head.text_proj.weight", rng.standard_normal((16, 16)) / 4), ("category_head.text_proj.bias", np.zeros(16)),
                     ("category_head.null_embed", rng.standard_normal((1, 16)))):
        arr = np.ascontiguousarray(arr, np.float32)
        shape = (C.c_int64 * arr.ndim)(*arr.shape)
        check(ctx.lib.odise_hip_load_weight(ctx.h, key.encode(), arr.ctypes.data_as(C.POINTER(C.c_float)), shape, arr.ndim), key)
    check(ctx.lib.odise_hip_classify_build(ctx.h), "classify_build")


def vocabulary(ctx, K):
    rng = np.random.default_rng(K)
    cat, clp = (np.ascontiguousarray(rng.standard_normal((K, 16)), np.float32) for _ in range(2))
    gs, ov = np.ones(K, np.int32), np.zeros(K, np.int32)
    check(ctx.lib.odise_hip_set_vocabulary(ctx.h, cat.ctypes.data_as(C.c_void_p), clp.ctypes.data_as(C.c_void_p), K, 16, gs.ctypes.data_as(C.c_void_p),
                                           ov.ctypes.data_as(C.c_void_p), K, C.c_float(0.3), C.c_float(0.7)), "set_vocabulary")


def fill(ctx, handle, K, side, views, rng):
    """`views` views of Q smooth masks at side / 4 and random class rows into the handle, every second one mirrored."""
    g = side // 4
    for a in range(views):
        coarse = rng.standard_normal((Q, g // 16, g // 16)).astype(np.float32) * 6
        logits = ctx.to_device(np.ascontiguousarray(np.kron(coarse, np.ones((16, 16), np.float32))[None]))
        check(ctx.lib.odise_hip_set_head_masks(ctx.h, logits, 1, Q, g, g), "set_head_masks")
        mc = rng.standard_normal((Q, K + 1)).astype(np.float32) * 3
        cls = ctx.to_device(mc - np.log(np.exp(mc).sum(-1, keepdims=True)))
        handle.add_view(0, cls, (side, side), (side, side), a % 2 == 1)
        ctx.sync()                                                         # logits and cls are read by the launch


def device_ms(ctx, fn, reps):
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def one_shape(ctx, K, side, reps, rounds):
    vocabulary(ctx, K)
    rng = np.random.default_rng(side)
    out = ctx.empty((side, side), np.int32)
    line = {"K": K, "size": [side, side], "Q": Q, "Qpad": (Q + 7) // 8 * 8, "reps": reps, "rounds": rounds}
    have_single = hasattr(ctx.lib, "odise_hip_lab_tta_single_argmax")
    for A in VIEWS:
        handle = ctx.tta_create((side, side), K, Q, A)
        fill(ctx, handle, K, side, A, rng)
        finish = lambda: handle.finish(sem_argmax=out)  # noqa: E731
        kernels = {"finish": finish}
        if A == 1 and have_single:
            ref = ctx.empty((side, side), np.int32)
            kernels["single"] = lambda: check(ctx.lib.odise_hip_lab_tta_single_argmax(ctx.h, C.c_void_p(handle.handle), ref), "single_argmax")
            kernels["single"]()
            finish()
            ctx.sync()
            assert np.array_equal(ref.numpy(), out.numpy()), "tta_finish at one view and semantic_argmax_kernel disagree"
        for fn in kernels.values():
            for _ in range(WARMUP):
                fn()
        ms = {name: [] for name in kernels}
        for _ in range(rounds):                                            # alternating: a drift of the machine hits both alike
            for name, fn in kernels.items():
                ms[name].append(device_ms(ctx, fn, reps))
        depth = A * line["Qpad"]
        line[f"A{A}"] = {"depth": depth, "S_cat_MB": round(side * side * depth * 2 / 1e6, 1), **{name: stats(v) for name, v in ms.items()}}
        handle.close()
    if "single" in line["A1"]:
        s, f = line["A1"]["single"], line["A1"]["finish"]
        line["A1_finish_over_single"] = round(f["median_ms"] / s["median_ms"], 3)
        line["single_spread"] = round((s["max_ms"] - s["min_ms"]) / s["median_ms"], 3)
    for A in VIEWS[1:]:
        line[f"A{A}_over_A1"] = round(line[f"A{A}"]["finish"]["median_ms"] / line["A1"]["finish"]["median_ms"], 3)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = Context(0)
    if not hasattr(ctx.lib, "odise_hip_lab_tta_single_argmax"):
        print("product library: semantic_argmax_kernel is not reachable on its own, only tta_finish is timed (see the module docstring)", file=sys.stderr)
    category_head(ctx)
    lines = []
    for K, side in SHAPES:
        r = one_shape(ctx, K, side, a.reps, a.rounds)
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
