"""GPU: the eval-loop helpers are bit-exact integer / byte work: resize against Pillow itself and against the
pinned oracle, confusion matrix and segment-pair histogram against numpy."""
import numpy as np
import pytest

from oracle.eval_ops import pair_histogram, pil_resize_bilinear_u8, resize_shortest_edge_shape, semantic_confusion

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("h,w,oh,ow", [(37, 53, 74, 106), (120, 90, 64, 48), (64, 64, 64, 31), (50, 70, 123, 70), (33, 47, 8, 5), (16, 16, 16, 16),
                                       (480, 640, 1024, 1365), (1500, 2000, 768, 1024)])
def test_resize_is_bit_identical_to_pillow(ctx, h, w, oh, ow):
    from PIL import Image
    rng = np.random.default_rng(h + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = ctx.resize_bilinear_u8(ctx.to_device(img), oh, ow).numpy()
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    np.testing.assert_array_equal(got, ref)
    if h * w < 20000:
        np.testing.assert_array_equal(got, pil_resize_bilinear_u8(img, oh, ow))


def test_shortest_edge_resize_to_chw_float(ctx):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)
    oh, ow = resize_shortest_edge_shape(300, 400, 512, 1280)
    assert (oh, ow) == (512, 683)
    d = ctx.resize_bilinear_u8(ctx.to_device(img), oh, ow)
    chw = ctx.u8_hwc_to_f32_chw(d, 1.0 / 255.0).numpy()
    ref = d.numpy().transpose(2, 0, 1).astype(np.float32) * np.float32(1.0 / 255.0)
    np.testing.assert_array_equal(chw, ref)


@pytest.mark.parametrize("K,h,w", [(5, 33, 47), (150, 256, 300), (133, 512, 512)])
def test_semantic_confusion_matches_numpy(ctx, K, h, w):
    rng = np.random.default_rng(K)
    sem = rng.standard_normal((K, h, w)).astype(np.float32)
    gt = rng.integers(0, K, (h, w)).astype(np.int32)
    gt[rng.random((h, w)) < 0.1] = 255
    ref = semantic_confusion(sem, gt)
    g = gt.copy()
    g[g == 255] = K
    conf = ctx.semantic_confusion(ctx.to_device(sem), ctx.to_device(g))
    conf = ctx.semantic_confusion(ctx.to_device(sem), ctx.to_device(g), conf)   # accumulates
    np.testing.assert_array_equal(conf.numpy(), 2 * ref)


@pytest.mark.parametrize("na,nb", [(7, 12), (101, 200)])
def test_pair_histogram_matches_numpy(ctx, na, nb):
    rng = np.random.default_rng(na)
    a = rng.integers(0, na, (400, 500)).astype(np.int32)
    b = rng.integers(0, nb, (400, 500)).astype(np.int32)
    got = ctx.pair_histogram(ctx.to_device(a), ctx.to_device(b), na, nb).numpy()
    np.testing.assert_array_equal(got, pair_histogram(a, b, na, nb))


# The counting kernels keep a per-block histogram in LDS up to 12288 cells (csrc/lds_hist.h) and count in global memory above it.
# (K + 1)^2 cells: K = 109 (12100) is the last size in LDS, K = 110 (12321) the first in global memory; 150 and 254 are the evaluators' sizes.
@pytest.mark.parametrize("K", [109, 110, 150, 254])
def test_semantic_confusion_on_both_sides_of_the_histogram_limit(ctx, K):
    h, w = 67, 131
    rng = np.random.default_rng(K)
    sem = rng.standard_normal((K, h, w)).astype(np.float32)
    g = rng.integers(0, K, (h, w)).astype(np.int32)
    g[rng.random((h, w)) < 0.1] = K
    ref = np.zeros((K + 1, K + 1), np.int64)
    np.add.at(ref, (sem.argmax(axis=0).reshape(-1), g.reshape(-1)), 1)
    d_sem, d_g = ctx.to_device(sem), ctx.to_device(g)
    conf = ctx.semantic_confusion(d_sem, d_g)
    np.testing.assert_array_equal(conf.numpy(), ref)
    conf = ctx.semantic_confusion(d_sem, d_g, conf)                               # adds to what is there
    np.testing.assert_array_equal(conf.numpy(), 2 * ref)


@pytest.mark.parametrize("na,nb", [(7, 5), (130, 100)])                           # 35 cells; 13000 cells
def test_pair_histogram_on_both_sides_of_the_histogram_limit(ctx, na, nb):
    rng = np.random.default_rng(na)
    a = rng.integers(-2, na + 3, 1000).astype(np.int32)                           # some ids outside the range on either side: not counted
    b = rng.integers(-2, nb + 3, 1000).astype(np.int32)
    ok = (a >= 0) & (a < na) & (b >= 0) & (b < nb)
    assert 0 < ok.sum() < ok.size
    ref = np.zeros((na, nb), np.int32)
    np.add.at(ref, (a[ok], b[ok]), 1)
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    hist = ctx.pair_histogram(d_a, d_b, na, nb)
    np.testing.assert_array_equal(hist.numpy(), ref)
    hist = ctx.pair_histogram(d_a, d_b, na, nb, hist)
    np.testing.assert_array_equal(hist.numpy(), 2 * ref)
