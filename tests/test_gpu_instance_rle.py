"""COCO RLE on the device (odise_amd/csrc/rle.hip): `odise_hip_rle_encode` byte for byte against the host restatement of pycocotools
(odise_amd/coco_rle.py), `odise_hip_instance_rle` (straight from the mask logits) against the fp32 masks of the default instance path,
the capacity contract, and `HipCategoryODISE.instance_rle` on the small model and on the full-size batch of four 1024^2 pictures."""
import ctypes as C

import numpy as np
import pytest
import torch

from odise_amd import coco_rle as R
from odise_amd._lib import F32, U8
from small_model import build_small, image_u8 as _image_u8

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))


# ---- full size: the benchmarked batch ----------------------------------------------------------------------------------------------------
def _records(res):
    return [R.instances_to_coco_json(r["instances"], i) for i, r in enumerate(res)]


def test_fullsize_batch_of_four_1024_and_encoder_prefetch(ctx, fullsize_model):
    """Runs first in this module: the full-size model is still the resident one after tests/test_gpu_fullsize_batch.py.
    Four 1024^2 pictures in one call (bench.py's default batch): the RLE records equal those of the fp32 masks, with no masks buffer; then
    the same pictures under other pointers as a prefetched batch (odise_hip_infer_prefetch) give the same records again."""
    from fullsize import build_models, category_head_state, image_u8, reference
    hip = fullsize_model
    ext, bb, head = build_models()                                           # COCO-133 over picture 0, as the fixture built it (memoised)
    _, heads, _ = reference(bb, head, ext, 1024, 133, 254)
    hip.load_category_head(category_head_state(heads))
    hip.set_vocabulary(heads.text_embed.numpy(), heads.clip_text_embed.numpy(), heads.group_sizes, heads.category_overlapping_mask.numpy(),
                       set(range(80)), heads.alpha, heads.beta)
    S, n = 1024, 4
    imgs = [np.ascontiguousarray(image_u8(S, S, seed).numpy()) for seed in range(n)]
    A = [ctx.to_device(i) for i in imgs]
    B = [ctx.to_device(i) for i in imgs]
    hw = [(S, S)] * n
    ref = _records(hip.infer_device(A, 1, hw, hw, to_host=True))
    assert sum(len(r) for r in ref) > 0

    def stats():
        v = [C.c_int() for _ in range(4)]
        assert ctx.lib.odise_hip_prefetch_stats(ctx.h, *[C.byref(x) for x in v]) == 0
        return tuple(x.value for x in v)

    hip.instance_rle = True
    try:
        with _BufLog(hip) as log:
            plain = _records(hip.infer_device(A, 1, hw, hw, to_host=True))
            s0 = stats()
            hip.prefetch_device(B, 1, hw)
            first = _records(hip.infer_device(A, 1, hw, hw, to_host=True))      # prepares B behind its own VAE lane
            second = _records(hip.infer_device(B, 1, hw, hw, to_host=True))     # starts from B's prefetched latent
            hits = stats()[1] - s0[1]
    finally:
        hip.instance_rle = False
    assert not any(t.startswith("masks") for t in log.tags), log.tags
    assert hits == 1, "the prefetched batch was not consumed"
    for what, got in (("plain", plain), ("while prefetching", first), ("prefetched", second)):
        for i in range(n):
            assert got[i] == ref[i], f"{what}: records of picture {i} differ"


# ---- rle_encode against the host encoder -------------------------------------------------------------------------------------------------
def _blobs(h, w, seed):
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    y, x = np.ogrid[:h, :w]
    for _ in range(5):
        cy, cx = g.integers(0, h), g.integers(0, w)
        ry, rx = g.integers(1, max(2, h // 3)), g.integers(1, max(2, w // 3))
        m |= (((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 < 1).astype(np.uint8)
    return m


def _mask_set(h, w):
    """zeros, ones, one pixel in each corner, checkerboard, random blobs, a coarse noise mask."""
    ms = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        ms.append(m)
    yy, xx = np.mgrid[:h, :w]
    ms.append(((yy + xx) % 2).astype(np.uint8))
    ms.append(_blobs(h, w, h * 7 + w))
    ms.append((np.random.default_rng(h + w).random((h, w)) < 0.5).astype(np.uint8))
    return np.stack(ms)


@pytest.mark.parametrize("h,w", [(1, 1), (1, 4097), (4097, 1), (683, 512), (1024, 1024), (1024, 1536)])
def test_rle_encode_matches_host_encoder(ctx, h, w):
    masks = _mask_set(h, w)
    want = [R.encode(m) for m in masks]
    want_area = masks.reshape(len(masks), -1).sum(1)
    for dt, host in (("uint8", masks), ("float32", masks.astype(np.float32) * np.float32(0.75))):   # any nonzero value is 1
        rles, area = ctx.rle_encode(ctx.to_device(host))
        for k, (a, b) in enumerate(zip(rles, want)):
            assert a == b, f"{dt} mask {k} of {h}x{w}: {a['counts'][:60]!r} != {b['counts'][:60]!r}"
        np.testing.assert_array_equal(area, want_area)
    rles, _ = ctx.rle_encode(ctx.to_device(masks.astype(bool)))
    assert rles == want


def test_rle_encode_more_masks_than_one_scan_block(ctx):
    """1100 masks: the exclusive scan of the string lengths runs over two 1024-mask chunks (rle_offsets_kernel's carry)."""
    g = np.random.default_rng(11)
    masks = (g.random((1100, 7, 5)) < 0.4).astype(np.uint8)
    masks[::97] = 0                                               # a few one-character strings among them
    want = [R.encode(m) for m in masks]
    rles, area = ctx.rle_encode(ctx.to_device(masks))
    assert rles == want
    np.testing.assert_array_equal(area, masks.reshape(len(masks), -1).sum(1))


def test_rle_encode_rejects_bad_arguments(ctx):
    off = ctx.empty((2,), np.int64)
    m = ctx.empty((1, 4, 4), np.float32)
    lib = ctx.lib
    assert lib.odise_hip_rle_encode(ctx.h, m.ptr, 0, 1, 4, 4, None, 0, off.ptr, None) != 0          # fp16 masks
    assert "dtype" in lib.odise_hip_last_error().decode()
    assert lib.odise_hip_rle_encode(ctx.h, m.ptr, F32, 1, 0, 4, None, 0, off.ptr, None) != 0        # empty mask
    assert lib.odise_hip_rle_encode(ctx.h, m.ptr, F32, 1, 4, 4, None, 16, off.ptr, None) != 0       # capacity without a buffer
    assert lib.odise_hip_rle_encode(ctx.h, m.ptr, U8, -1, 4, 4, None, 0, off.ptr, None) != 0


# ---- capacity ----------------------------------------------------------------------------------------------------------------------------
def test_capacity_too_small_leaves_the_buffer_alone_and_the_wrapper_retries(ctx):
    masks = np.stack([_blobs(300, 200, s) for s in range(6)])
    want = [R.encode(m) for m in masks]
    need = sum(len(r["counts"]) for r in want)
    dev = ctx.to_device(masks)
    cap = need // 2
    canary = np.full(need + 512, 0xA5, np.uint8)
    buf = ctx.to_device(canary)
    off = ctx.zeros((len(masks) + 1,), np.int64)
    area = ctx.zeros((len(masks),), np.int64)
    assert ctx.lib.odise_hip_rle_encode(ctx.h, dev.ptr, U8, len(masks), 300, 200, buf.ptr, cap, off.ptr, area.ptr) == 0
    o = off.numpy()
    np.testing.assert_array_equal(o, np.concatenate(([0], np.cumsum([len(r["counts"]) for r in want]))))   # complete although nothing fit
    np.testing.assert_array_equal(area.numpy(), masks.reshape(len(masks), -1).sum(1))
    np.testing.assert_array_equal(buf.numpy(), canary)                                                     # not a byte written
    # exactly enough: the strings, and the canary bytes past them untouched
    assert ctx.lib.odise_hip_rle_encode(ctx.h, dev.ptr, U8, len(masks), 300, 200, buf.ptr, need, off.ptr, area.ptr) == 0
    got = buf.numpy()
    assert got[:need].tobytes().decode() == "".join(r["counts"] for r in want)
    np.testing.assert_array_equal(got[need:], canary[need:])
    # the wrapper: first pass with a budget that is too small, then the exact size
    rles, a = ctx.rle_encode(dev, capacity=16)
    assert rles == want
    np.testing.assert_array_equal(a, masks.reshape(len(masks), -1).sum(1))


# ---- the small model: fused against unfused ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx):
    return build_small(ctx)


class _BufLog:
    """Records the pooled-buffer tags a call asks for (HipCategoryODISE._buf)."""

    def __init__(self, hip):
        self.hip, self.tags = hip, []

    def __enter__(self):
        orig = self.hip._buf

        def logged(tag, shape, dtype):
            self.tags.append(tag)
            return orig(tag, shape, dtype)
        self.hip._buf = logged
        return self

    def __exit__(self, *exc):
        del self.hip._buf


def _rle_forward(hip, batch):
    hip.instance_rle = True
    try:
        with _BufLog(hip) as log:
            res = hip.forward(batch)
    finally:
        hip.instance_rle = False
    assert not any(t.startswith("masks") for t in log.tags), log.tags
    return res


@pytest.mark.parametrize("h,w,oh,ow", [(512, 512, 512, 512),      # x4 path (output = image size, width % 4 == 0)
                                       (500, 502, 500, 502),      # generic path: width not a multiple of 4
                                       (512, 704, 256, 352)])     # generic path: resized output
def test_instance_rle_equals_the_fp32_masks(small, ctx, h, w, oh, ow):
    hip = small
    batch = [{"image": _image_u8(h, w, seed=h + w), "height": oh, "width": ow}]
    ref = hip.forward(batch)[0]["instances"]
    got = _rle_forward(hip, batch)[0]
    assert "pred_masks" not in got["instances"] and "sem_seg" in got and "panoptic_seg" in got
    inst = got["instances"]
    n = len(ref["scores"])
    assert n > 0 and len(inst["pred_masks_rle"]) == n
    for k in ("scores", "pred_classes", "query_index"):
        np.testing.assert_array_equal(inst[k], ref[k])
    masks = ref["pred_masks"]
    for i, rle in enumerate(inst["pred_masks_rle"]):
        assert rle["size"] == [oh, ow]
        np.testing.assert_array_equal(R.decode(rle), (masks[i] > 0.5).astype(np.uint8), err_msg=f"instance {i}")
    np.testing.assert_array_equal(inst["area"], (masks > 0.5).reshape(n, -1).sum(1))
    dev_rles, dev_area = ctx.rle_encode(ctx.to_device(masks))
    assert inst["pred_masks_rle"] == dev_rles
    np.testing.assert_array_equal(inst["area"], dev_area)
    assert R.instances_to_coco_json(got["instances"], 7) == R.instances_to_coco_json(ref, 7)


def test_instance_rle_direct_call_and_its_capacity_retry(small, ctx):
    """Context.instance_rle on the pooled instance table of the last call: a budget of 16 bytes for 100 masks takes the retry."""
    hip = small
    batch = [{"image": _image_u8(512, 512, seed=3)}]
    ref = hip.forward(batch)[0]["instances"]
    topk = hip.test_topk_per_image
    table = hip._pool[("inst_table", np.dtype(np.int32).str)].view((1 + 2 * topk,), np.int32)
    rles, area = ctx.instance_rle(0, table, topk, (512, 512), (512, 512), (512, 512), capacity=16)
    assert rles == [R.encode(m > 0.5) for m in ref["pred_masks"]]
    np.testing.assert_array_equal(area, (ref["pred_masks"] > 0.5).reshape(len(rles), -1).sum(1))
    assert ctx.lib.odise_hip_instance_rle(ctx.h, 5, table.ptr, topk, 512, 512, 512, 512, 512, 512, None, 0, table.ptr, None) != 0   # image 5 of 1
    assert "out of range" in ctx.lib.odise_hip_last_error().decode()
    assert ctx.lib.odise_hip_instance_rle(ctx.h, 0, table.ptr, topk, 576, 512, 512, 512, 512, 512, None, 0, table.ptr, None) != 0   # padding
    assert "padded size" in ctx.lib.odise_hip_last_error().decode()


def test_instance_rle_retry_grows_the_pooled_buffer(small, ctx):
    """A selection whose strings exceed the default budget is encoded once more into the pooled buffer, grown to the exact size; the next
    call of the same picture fits at once (no retry, no allocation)."""
    hip = small
    batch = [{"image": _image_u8(512, 512, seed=3)}]
    hip._pool.pop(("rle0", np.dtype(np.uint8).str), None)       # start from the default budget
    hip.instance_rle = True
    try:
        with _BufLog(hip) as first:
            a = hip.forward(batch)[0]
        with _BufLog(hip) as second:
            b = hip.forward(batch)[0]
    finally:
        hip.instance_rle = False
    need = sum(len(r["counts"]) for r in a["instances"]["pred_masks_rle"])
    if need > ctx.RLE_BYTES_PER_MASK * hip.test_topk_per_image:   # the synthetic masks are noise-like: this selection needs several MB
        assert first.tags.count("rle0") == 2, first.tags
    assert second.tags.count("rle0") == 1, second.tags
    assert R.instances_to_coco_json(a["instances"], 0) == R.instances_to_coco_json(b["instances"], 0)


def test_instance_rle_batch_of_unequal_pictures(small):
    hip = small
    batch = [{"image": _image_u8(512, 512, seed=1)}, {"image": _image_u8(320, 448, seed=2), "height": 160, "width": 224}]
    ref = hip.forward(batch)
    got = _rle_forward(hip, batch)
    for i in range(2):
        assert R.instances_to_coco_json(got[i]["instances"], i) == R.instances_to_coco_json(ref[i]["instances"], i)
