"""GPU: HipSemSegEvaluator.process on a prediction buffer that the caller overwrites right after the call, as the model's pooled output
buffers are by the next forward.  The pictures need both retries of the call (more classes than MAX_SEGMENTS, strings longer than the default
capacity), which read the prediction again: they must have run before process() returns."""
import numpy as np
import pytest

from odise_amd import semseg_eval as SE
from odise_amd._lib import MAX_SEGMENTS
from semseg_cases import blobs

pytestmark = pytest.mark.gpu

K, H, W = 150, 65, 67


def pictures():
    yy, xx = np.mgrid[0:H, 0:W]
    busy = ((yy * W + xx) % K).astype(np.int32)                 # all 150 classes, a change at every pixel: both retries
    checker = ((yy + 2 * xx) % 3 * 70).astype(np.int32)         # three classes, a change at every pixel: the retry for the size
    calm = blobs(H, W, K, seed=7).astype(np.int32)              # no retry
    return [busy, checker, calm, busy[::-1].copy()]


def host(maps, gts):
    conf = sum(SE.confusion(m, np.where(g == 255, K, g), K) for m, g in zip(maps, gts))
    rows = [r for i, m in enumerate(maps) for r in SE.encode_json_sem_seg(m, f"{i}.png")]
    return conf, rows


@pytest.mark.parametrize("route", ["labels", "scores"])
def test_process_on_a_reused_buffer_with_pictures_that_need_the_retries(ctx, route):
    maps = pictures()
    gts = [np.where(np.random.default_rng(i).random(m.shape) < 0.8, m, 255).astype(np.int32) for i, m in enumerate(maps)]
    assert len(np.unique(maps[0])) == K > MAX_SEGMENTS
    assert sum(len(r["segmentation"]["counts"]) for r in SE.encode_json_sem_seg(maps[1], "x")) > ctx.sem_rle_bytes((H, W))
    up = (lambda m: (np.arange(K)[:, None, None] == m[None]).astype(np.float32)) if route == "scores" else (lambda m: m)
    pooled = ctx.to_device(up(maps[0]))                         # ONE buffer for every picture
    ev = SE.HipSemSegEvaluator(ctx, [f"c{c}" for c in range(K)], 255, "reuse", compute_boundary_iou=False)
    for i, (m, g) in enumerate(zip(maps, gts)):
        pooled.copy_from(up(m))
        ev.process(pooled, g, f"{i}.png")
    pooled.copy_from(up(np.full((H, W), 5, np.int32)))
    launches = [p.launches for _, p in ev._pending]
    assert all(p.pred is None and not hasattr(p, "gt") for _, p in ev._pending)       # settled: nothing of the caller's is held
    res = ev.evaluate()
    conf, rows = host(maps, gts)
    assert launches == [3, 2, 1, 3] == [p.launches for _, p in ev._pending]            # evaluate() launched nothing more
    assert np.array_equal(ev.conf_matrix, conf) and ev.predictions == rows
    assert repr(res) == repr({"reuse/sem_seg": SE.results(conf, None, ev.class_names)})


def test_process_with_pred_kept_defers_the_retries_to_evaluate(ctx):
    maps = pictures()[:2]
    gts = [m.copy() for m in maps]
    ev = SE.HipSemSegEvaluator(ctx, [f"c{c}" for c in range(K)], 255, "kept", compute_boundary_iou=False)
    for i, (m, g) in enumerate(zip(maps, gts)):
        ev.process(ctx.to_device(m), ctx.to_device(g), f"{i}.png", pred_kept=True)
    assert [p.launches for _, p in ev._pending] == [1, 1] and all(p.pred is not None and not hasattr(p, "gt") for _, p in ev._pending)
    ev.evaluate()
    conf, rows = host(maps, gts)
    assert [p.launches for _, p in ev._pending] == [3, 2]
    assert np.array_equal(ev.conf_matrix, conf) and ev.predictions == rows
