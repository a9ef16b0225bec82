"""Cost of Boundary PQ beside PQ: odise_hip_panoptic_quality_boundary of this tree against odise_hip_panoptic_quality of the PARENT
commit's library on the same pictures as tools/pq_bench.py (1024x1024 and 1280x1280, about 30 ground-truth and 20 predicted segments with
the staged pairs of tests/pq_boundary_cases.py, RGB ground truth), `--reps` calls between HIP events on an otherwise idle context.

The two libraries alternate, three runs each, every run in a process of its own (a process loads one library); the parent's own spread
(max - min of its three runs) is the margin a difference has to exceed to mean anything.  This tree's plain call is timed as well: it
shares the pixel pass with the parent's and should sit inside that margin.

    python -m odise_amd.build                                   # this tree
    (build the parent commit's tree the same way, elsewhere)
    python tools/pq_boundary_bench.py --parent-lib /path/to/parent/libodise_hip.so --out profiles/pq_boundary_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1024, 1024), (1280, 1280))


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def leg(lib_path, reps):
    """One process, one library: {"HxW": {"plain_ms", "boundary_ms" (when the library has the call)}}."""
    from odise_amd._lib import MAX_SEGMENTS, load
    lib = load(lib_path, allow_missing=True)   # the parent's library lacks the new calls; the first load decides for the process
    from odise_amd.runtime import Context
    from pq_boundary_cases import boundary_case
    ctx = Context(0)
    out = {}
    for h, w in SIZES:
        case = boundary_case(h + w, h, w, 30, 20, cell=(97, 131))
        rec, rgb = ctx.to_device(case.record(MAX_SEGMENTS)), ctx.to_device(case.rgb())
        ref, _ = case.stats()
        stats, flags = ctx.panoptic_quality_record(rec, (h, w), rgb, case.gt_rows, case.C)
        assert stats.numpy().tobytes() == ref.to_records().tobytes() and int(flags.numpy()[0]) == 0, "device and host statistics disagree"
        r = {"plain_ms": device_ms(ctx, lambda: ctx.panoptic_quality_record(rec, (h, w), rgb, case.gt_rows, case.C, stats, flags), reps)}
        if hasattr(lib, "odise_hip_panoptic_quality_boundary"):
            tr = case.assert_boundary_rules_fire()
            b_ref, _ = case.boundary_stats()
            stats, b_stats, flags = ctx.panoptic_quality_boundary_record(rec, (h, w), rgb, case.gt_rows, case.C)
            assert stats.numpy().tobytes() == ref.to_records().tobytes() and b_stats.numpy().tobytes() == b_ref.to_records().tobytes()
            r["boundary_ms"] = device_ms(ctx, lambda: ctx.panoptic_quality_boundary_record(rec, (h, w), rgb, case.gt_rows, case.C, stats, b_stats, flags), reps)
            r["radius"], r["demoted"], r["lowered"] = ctx.boundary_radius(h, w), tr["demoted"], tr["lowered"]
        out[f"{h}x{w}"] = r
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-lib", required=True, help="libodise_hip.so built from the parent commit")
    ap.add_argument("--lib", default=os.path.join(ROOT, "odise_amd", "lib", "libodise_hip.so"))
    ap.add_argument("--reps", type=int, default=200)
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
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit(f"{name} leg failed ({p.returncode}):\n{p.stdout}\n{p.stderr}")
            runs[name].append(json.loads(next(l for l in p.stdout.splitlines() if l.startswith("LEG "))[4:]))
    lines = []
    for h, w in SIZES:
        k = f"{h}x{w}"
        parent = [r[k]["plain_ms"] for r in runs["parent"]]
        plain = [r[k]["plain_ms"] for r in runs["this"]]
        boundary = [r[k]["boundary_ms"] for r in runs["this"]]
        med = statistics.median
        line = {"size": [h, w], "radius": runs["this"][0][k]["radius"], "reps": a.reps,
                "parent_pq_ms": [round(v, 4) for v in parent], "parent_spread_ms": round(max(parent) - min(parent), 4),
                "this_pq_ms": [round(v, 4) for v in plain], "this_boundary_ms": [round(v, 4) for v in boundary],
                "pq_over_parent": round(med(plain) / med(parent), 3), "boundary_over_parent": round(med(boundary) / med(parent), 3),
                "demoted": runs["this"][0][k]["demoted"], "lowered": runs["this"][0][k]["lowered"]}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
