"""Cost of drawing one panoptic result, at 1024x1024 and 1280x1280, smooth synthetic maps of about 20 segments (half stuff, half things):

  components  odise_hip_connected_components alone: tile labelling in LDS, border unions, flatten
  anchors     odise_hip_segment_anchors: the same plus areas, selection, order, histograms and medians
  overlay     odise_hip_panoptic_overlay: one pass over ids (4 bytes per pixel) and picture (3 in, 3 out)
  histogram   odise_hip_pair_histogram on the same map (as both of its inputs): the "one pass over the map" yardstick.  The expectation
              to confirm or refute: labelling costs a small multiple of it, and the overlay is launch-bound at these sizes.
  host        what the anchors call replaces: the device-to-host copy of the record, scipy.ndimage.label per stuff id with a 3x3
              structure and np.median on np.nonzero, on one CPU thread

Device times are HIP events around `--reps` back-to-back calls on an otherwise idle context (warmed up first); roots and anchors are
compared with the scipy formulation before they are timed.  Prints one JSON line per size; --out also writes them.

    python tools/vis_bench.py --out profiles/vis_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from odise_amd import visualize as V  # noqa: E402
from odise_amd._lib import RECORD_TABLE_LEN, split_record  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402


def smooth_map(h, w, n_ids=20, cell=(173, 211), seed=0):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, n_ids + 1, (h // cell[0] + 2, w // cell[1] + 2))
    ids = np.kron(coarse, np.ones(cell, np.int64))[31:31 + h, 57:57 + w].astype(np.int32)
    segments = [(int(i), int(i) % 2, int(i) % 7) for i in np.unique(ids) if i > 0]
    return ids, segments


def host_roots(ids):
    index = np.arange(ids.size).reshape(ids.shape)
    roots = np.full(ids.shape, -1, np.int32)
    for l in np.unique(ids):
        if l > 0:
            lab, n = ndimage.label(ids == l, structure=np.ones((3, 3), int))
            mins = np.asarray(ndimage.minimum(index, lab, np.arange(1, n + 1)), np.int64)
            roots[lab > 0] = mins[lab[lab > 0] - 1]
    return roots


def host_anchors(ids, segments, small, large):
    out = []
    for r, (i, isthing, _) in enumerate(segments):
        mask = ids == i
        if not mask.any():
            continue
        picks = [mask]
        if not isthing:
            lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
            areas = np.bincount(lab.ravel())[1:]
            k = int(np.argmax(areas))
            picks = [lab == c + 1 for c in range(n) if c == k or areas[c] > large] if areas[k] >= small else []
        for m in picks:
            ys, xs = np.nonzero(m)
            my, mx = np.median(np.nonzero(m), axis=1)
            out.append((r, len(ys), int(2 * mx), int(2 * my), xs.min(), ys.min(), xs.max(), ys.max()))
    return np.array(out, V.ANCHOR_DTYPE)


def device_ms(ctx, fn, reps):
    for _ in range(3):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def one_size(ctx, h, w, reps):
    ids, segments = smooth_map(h, w)
    table = np.zeros(RECORD_TABLE_LEN, np.int32)
    table[0] = len(segments)
    table[1:1 + 3 * len(segments)] = np.asarray(segments, np.int32).reshape(-1)
    rec = ctx.to_device(np.concatenate([ids.reshape(-1), table]))
    d_ids, d_table = split_record(rec, (h, w))
    small, large = V.SMALL_AREA, 30000              # 30000: some "other" components qualify at these sizes
    roots = ctx.empty((h, w), np.int32)
    ctx.connected_components(d_ids, roots)
    assert np.array_equal(roots.numpy(), host_roots(ids)), "device and host components disagree"
    want = host_anchors(ids, segments, small, large)
    anchors, count = ctx.segment_anchors(d_ids, d_table, small, large, 256)
    assert int(count.numpy()[0]) == len(want) and anchors.numpy()[:len(want)].tobytes() == want.tobytes(), "device and host anchors disagree"

    components = device_ms(ctx, lambda: ctx.connected_components(d_ids, roots), reps)
    anch = device_ms(ctx, lambda: ctx.segment_anchors(d_ids, d_table, small, large, 256, anchors, count), reps)
    image = ctx.to_device(np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8))
    colors = ctx.to_device(V.segment_colors(segments))
    out = ctx.empty((h, w, 3), np.uint8)
    overlay = device_ms(ctx, lambda: ctx.panoptic_overlay(image, d_ids, d_table, colors, 128, (0, 0, 0), out), reps)
    nid = int(ids.max()) + 1
    hist = ctx.zeros((nid, nid), np.int32)
    histogram = device_ms(ctx, lambda: ctx.pair_histogram(d_ids, d_ids, nid, nid, hist), reps)

    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        got = rec.numpy()
        t1 = time.perf_counter()
        host_anchors(got[:h * w].reshape(h, w), segments, small, large)
        host.append((t1 - t0, time.perf_counter() - t1))
    copy_ms, host_ms = (min(x[k] for x in host) * 1e3 for k in (0, 1))
    return {"size": [h, w], "segments": len(segments), "components": int(len(np.unique(host_roots(ids))) - (ids <= 0).any()), "anchors": len(want),
            "components_ms": round(components, 4), "anchors_ms": round(anch, 4), "overlay_ms": round(overlay, 4),
            "pair_histogram_ms": round(histogram, 4), "components_over_histogram": round(components / histogram, 2),
            "anchors_over_histogram": round(anch / histogram, 2), "overlay_GBps": round(10 * h * w / overlay / 1e6, 1),
            "host_copy_ms": round(copy_ms, 3), "host_label_median_ms": round(host_ms, 1), "reps": reps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
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
