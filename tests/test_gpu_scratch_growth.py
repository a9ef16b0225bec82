"""GPU: the context's scratch buffers (csrc/common.h DeviceScratch / scratch_reserve) grow under calls that are still in flight.

A context of its own, so that every buffer starts empty (the session context's are as large as whatever ran before).  Per owner the calls
go small -> large -> small; the large call is enqueued right behind the small one, with no synchronisation in between and every output
still on the device: the drain in front of the reallocation is what keeps the first call's reads valid.  Integer / byte work: every result
is compared exactly with the host restatement of its owner."""
import numpy as np
import pytest

from odise_amd import coco_rle as R
from odise_amd import sem_boundary as S
from odise_amd.runtime import Context
from test_gpu_sem_boundary import blocky, scores
from tests.test_oracle_jpeg import _jpeg, _picture, _pil

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def own():
    c = Context(0)
    yield c
    c.close()


def test_boundary_maps_grow_behind_calls_in_flight(own):
    """label_boundary at 5x7 (one map), semantic_boundary_confusion at 5x7 (two maps; with the 256-byte rounding of a map they still fit)
    and at 200x333 (grows), label_boundary at 5x7 again (the large buffer stays)."""
    ctx, K = own, 150
    rng = np.random.default_rng(57)
    small = blocky(rng, 5, 7, K, cell=(2, 3))
    small[0, 0], small[4, 6] = -3, 255                                    # outside [0, K] -> K
    pics = []
    for h, w in ((5, 7), (200, 333)):
        pred = blocky(rng, h, w, K - 1, cell=(2, 3) if h == 5 else (11, 13))
        gt = blocky(rng, h, w, K - 1, cell=(3, 2) if h == 5 else (9, 17))
        gt[rng.random((h, w)) < 0.1] = 255
        pics.append((pred, gt))
    # everything uploaded and every output allocated before the first call: nothing between the calls but the library's own work
    d_small = ctx.to_device(small)
    d_pics = [(ctx.to_device(scores(rng, pred, K)), ctx.to_device(gt)) for pred, gt in pics]
    out = [ctx.empty((5, 7), np.int32) for _ in range(2)]
    mats = [(ctx.zeros((K + 1, K + 1), np.int64), ctx.zeros((K + 1, K + 1), np.int64)) for _ in pics]
    ctx.sync()
    ctx.label_boundary(d_small, K, out=out[0])
    for (sem, gt), (conf, b_conf) in zip(d_pics, mats):
        ctx.semantic_boundary_confusion(sem, gt, conf, b_conf)
    ctx.label_boundary(d_small, K, out=out[1])
    ref = S.mask_to_boundary(S.clamp_labels(small, K))
    for o in out:
        np.testing.assert_array_equal(o.numpy(), ref)
    for (pred, gt), (conf, b_conf) in zip(pics, mats):
        np.testing.assert_array_equal(b_conf.numpy(), S.boundary_confusion(pred, gt, K), err_msg=str(pred.shape))
        ref_c = np.zeros((K + 1, K + 1), np.int64)
        np.add.at(ref_c, (pred.reshape(-1), S.clamp_labels(gt, K).reshape(-1)), 1)
        np.testing.assert_array_equal(conf.numpy(), ref_c, err_msg=str(pred.shape))


def test_rle_scratch_grows_behind_calls_in_flight(own):
    """rle_encode of 1 mask at 9x7, 5 masks at 130x70 (grows), 1 mask at 9x7 again."""
    ctx = own
    rng = np.random.default_rng(97)
    sets = [(rng.random((n, h, w)) < 0.4).astype(np.uint8) for n, h, w in ((1, 9, 7), (5, 130, 70), (1, 9, 7))]
    sets[1][0], sets[1][1] = 0, 1                                          # an empty and a full mask among the large ones
    dev = [ctx.to_device(m) for m in sets]
    bufs = [(ctx.empty((ctx.RLE_BYTES_PER_MASK * len(m),), np.uint8), ctx.empty((len(m) + 1,), np.int64), ctx.empty((len(m),), np.int64)) for m in sets]
    ctx.sync()
    pending = [ctx.rle_encode_async(d, bufs=b) for d, b in zip(dev, bufs)]
    for masks, p in zip(sets, pending):
        rles, area = p.result()
        assert rles == [R.encode(m) for m in masks], masks.shape
        np.testing.assert_array_equal(area, masks.reshape(len(masks), -1).sum(1))


def test_jpeg_staging_grows_behind_calls_in_flight(own):
    """The 37x52 / 768x1024 / 40x24 pictures of test_gpu_jpeg.py's buffer-reuse case, decoded back to back: the pinned staging buffer is
    guarded by the upload event, the device coefficients and planes by the drain."""
    ctx = own
    files = [_jpeg(_picture(37, 52, 5), mode="L", quality=80), _jpeg(_picture(768, 1024, 7), quality=85, subsampling=2),
             _jpeg(_picture(40, 24, 8), quality=70, subsampling=1)]
    outs = [ctx.empty(_pil(f).shape, np.uint8) for f in files]
    ctx.sync()
    got = [ctx.jpeg_decode(f, out=o) for f, o in zip(files, outs)]
    for f, g in zip(files, got):
        np.testing.assert_array_equal(g.numpy(), _pil(f))
