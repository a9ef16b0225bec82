"""GPU: the Boundary IoU counters of SemSegEvaluator (csrc/eval_ops.hip: odise_hip_label_boundary, odise_hip_semantic_boundary_confusion)
against the host restatement (odise_amd/sem_boundary.py).  Integer work: every comparison is exact."""
import numpy as np
import pytest

from odise_amd import sem_boundary as S

pytestmark = pytest.mark.gpu


def blocky(rng, h, w, K, cell=(11, 13)):
    small = rng.integers(0, K + 1, (h // cell[0] + 1, w // cell[1] + 1))
    return np.kron(small, np.ones(cell, np.int64))[:h, :w].astype(np.int32)


def scores(rng, pred, K):
    """fp32 [K, h, w] whose first-maximum arg-max is `pred` (values < K), with exact ties above the winner's index."""
    h, w = pred.shape
    sem = rng.standard_normal((K, h, w)).astype(np.float32)
    top = sem.max(axis=0) + 1.0
    np.put_along_axis(sem, pred[None], top[None], axis=0)
    tie = np.minimum(pred + 1, K - 1)                       # a later class with the same score must not win
    np.put_along_axis(sem, tie[None], top[None], axis=0)
    assert np.array_equal(sem.argmax(axis=0), pred)
    return sem


# (h, w, radius or 0 = the formula): one erosion; no side a multiple of 4 or of the block; windows across blocks; a window wider than half
# the picture; a radius larger than the picture (everything eroded); a width of one dword row and less
@pytest.mark.parametrize("h,w,r", [(5, 7, 0), (67, 131, 3), (200, 333, 0), (96, 160, 40), (24, 40, 64), (33, 1, 1), (1, 1, 0), (40, 86, 21)])
def test_label_boundary_matches_host(ctx, h, w, r):
    K = 150
    rng = np.random.default_rng(h * w + r)
    m = blocky(rng, h, w, K)
    m[rng.random((h, w)) < 0.02] = 255          # outside [0, K] -> K
    m[0, 0] = -3
    if (h, w, r) == (5, 7, 0):
        assert S.boundary_radius(h, w) == 1
    if (h, w, r) == (200, 333, 0):
        assert S.boundary_radius(h, w) == 8
    ref = S.mask_to_boundary(S.clamp_labels(m, K), r)
    got = ctx.label_boundary(ctx.to_device(m), K, r).numpy()
    np.testing.assert_array_equal(got, ref)
    if (h, w, r) == (24, 40, 64):
        np.testing.assert_array_equal(got, S.clamp_labels(m, K))


@pytest.mark.parametrize("r", [1, 4, 5, 16, 21, 22])
def test_minimum_travels_exactly_the_radius(ctx, r):
    h, w, K = 101, 117, 254
    m = np.full((h, w), 200, np.int32)
    m[50, 58] = 7
    got = ctx.label_boundary(ctx.to_device(m), K, r).numpy()
    inner = np.zeros((h, w), bool)
    inner[r:h - r, r:w - r] = True
    ys, xs = np.ogrid[:h, :w]
    near = (abs(ys - 50) <= r) & (abs(xs - 58) <= r)
    ref = np.where(inner, np.where(near, 193, 0), 200)
    ref[50, 58] = 0 if inner[50, 58] else 7
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got, S.mask_to_boundary(m, r))


@pytest.mark.parametrize("h,w", [(67, 131), (200, 333)])
@pytest.mark.parametrize("K", [3, 150, 254])
def test_semantic_boundary_confusion_matches_host(ctx, K, h, w):
    rng = np.random.default_rng(K + h)
    pred = blocky(rng, h, w, K - 1)
    gt = blocky(rng, h, w, K - 1, cell=(9, 17))
    gt[rng.random((h, w)) < 0.1] = 255
    sem, g = ctx.to_device(scores(rng, pred, K)), ctx.to_device(gt)
    ref_b = S.boundary_confusion(pred, gt, K)
    ref_c = ctx.semantic_confusion(sem, g).numpy()           # the existing entry point on the same inputs
    assert ref_c.sum() == h * w and ref_b.sum() == h * w
    conf, b_conf = ctx.semantic_boundary_confusion(sem, g)
    assert conf is None
    np.testing.assert_array_equal(b_conf.numpy(), ref_b)
    conf = ctx.zeros((K + 1, K + 1), np.int64)
    conf, b_conf = ctx.semantic_boundary_confusion(sem, g, conf, b_conf)   # accumulates: second call on b_conf, first on conf
    np.testing.assert_array_equal(conf.numpy(), ref_c)
    np.testing.assert_array_equal(b_conf.numpy(), 2 * ref_b)
    conf, b_conf = ctx.semantic_boundary_confusion(sem, g, conf, b_conf)
    np.testing.assert_array_equal(conf.numpy(), 2 * ref_c)
    np.testing.assert_array_equal(b_conf.numpy(), 3 * ref_b)
    assert int(b_conf.numpy().sum()) == 3 * h * w
    # an explicit radius is honoured
    _, b5 = ctx.semantic_boundary_confusion(sem, g, radius=5)
    np.testing.assert_array_equal(b5.numpy(), S.boundary_confusion(pred, gt, K, 5))


def test_255_classes_are_refused_and_nothing_is_written(ctx):
    K, h, w = 255, 16, 20
    rng = np.random.default_rng(0)
    sem = ctx.to_device(rng.standard_normal((K, h, w)).astype(np.float32))
    gt = ctx.to_device(rng.integers(0, K, (h, w)).astype(np.int32))
    conf, b_conf = ctx.zeros((K + 1, K + 1), np.int64), ctx.zeros((K + 1, K + 1), np.int64)
    with pytest.raises(RuntimeError, match="Boundary IoU"):
        ctx.semantic_boundary_confusion(sem, gt, conf, b_conf)
    out = ctx.zeros((h, w), np.int32)
    with pytest.raises(RuntimeError, match="Boundary IoU"):
        ctx.label_boundary(gt, K, out=out)
    ctx.sync()
    assert not conf.numpy().any() and not b_conf.numpy().any() and not out.numpy().any()
    assert ctx.boundary_radius(1024, 1024) == 29
    with pytest.raises(RuntimeError):
        ctx.boundary_radius(0, 4)


def test_production_shape_1024(ctx):
    K, h, w = 150, 1024, 1024
    rng = np.random.default_rng(1024)
    pred = blocky(rng, h, w, K - 1, cell=(97, 131))
    gt = blocky(rng, h, w, K - 1, cell=(113, 89))
    gt[:40, 900:] = 255
    assert ctx.boundary_radius(h, w) == 29
    got = ctx.label_boundary(ctx.to_device(gt), K).numpy()
    np.testing.assert_array_equal(got, S.mask_to_boundary(S.clamp_labels(gt, K)))
    # one-hot scores: exactly one maximum per pixel
    sem = np.zeros((K, h, w), np.float32)
    np.put_along_axis(sem, pred[None], 1.0, axis=0)
    conf, b_conf = ctx.semantic_boundary_confusion(ctx.to_device(sem), ctx.to_device(gt), ctx.zeros((K + 1, K + 1), np.int64))
    np.testing.assert_array_equal(b_conf.numpy(), S.boundary_confusion(pred, gt, K))
    ref_c = np.zeros((K + 1, K + 1), np.int64)
    np.add.at(ref_c, (pred.reshape(-1), S.clamp_labels(gt, K).reshape(-1)), 1)
    np.testing.assert_array_equal(conf.numpy(), ref_c)
