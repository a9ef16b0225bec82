"""CPU: tests/glue_reference.py (float64 numpy) against torch's own operators - F.interpolate, F.normalize, torch.softmax, sigmoid and
oracle.clip_vit.clip_preprocess - at the shapes tests/test_gpu_glue_ops.py uses, so the restatement is shown to BE the operation before any
kernel is held to it; and the properties of the crafted inputs that the GPU tests rely on (undecided shares, the single-key row, overlap
counts), asserted from the reference alone.

F.interpolate is compared in float32: torch takes the tap positions in the tensor's own type, so a float64 call moves every tap by the fp32
rounding of its coordinate (up to 4e-6 of a pixel here) - it is the fp32 taps that define what the device computes.  The distance then is
torch's own fp32 accumulation, bounded by the rule the GPU tests apply to fp32 outputs: 8 * 2^-24 * sum |weight * tap| (the two preprocess
operations subtract the mean and divide by the deviation in fp32 afterwards, one more rounding of that conditioning each: 10).  softmax,
normalize and the classification formula have no taps and are compared in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as G
import glue_reference as R
from oracle.clip_vit import clip_preprocess

U = G.U


def within(got, ref, cond, what, k=8.0):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = k * U * cond
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max err {err.max():.3e}, worst err / bound {worst:.3f}")
    assert got.shape == ref.shape and worst <= 1.0, what


@pytest.mark.parametrize("s", G.BICUBIC_S)
def test_bicubic_window_resize_is_torchs(s):
    img = G.bicubic_image(s)
    ref, cond = R.crop_resize_bicubic(img, G.BICUBIC_BOXES, s, G.CROP_S)
    win = torch.from_numpy(R.crop_extract(img, G.BICUBIC_BOXES, s).astype(np.float32))
    got = F.interpolate(win, size=(G.CROP_S, G.CROP_S), mode="bicubic", align_corners=False).numpy()
    within(got, ref, cond, f"bicubic {s} -> {G.CROP_S}")
    assert np.abs(ref).max() < G.OUTSIDE / 4, "the reference itself read outside a window"
    if s == G.CROP_S:   # weights 0, 1, 0, 0
        assert np.array_equal(ref, win.numpy().astype(np.float64))


def test_crop_extract_is_slicing():
    img = G.crop_image()
    ref = R.crop_extract(img, G.CROP_BOXES, G.CROP_S)
    t = torch.from_numpy(img)
    got = torch.stack([t[b, :, y:y + G.CROP_S, x:x + G.CROP_S] for b in range(img.shape[0]) for y, x in G.CROP_BOXES]).numpy()
    assert np.array_equal(ref, got.astype(np.float64))


@pytest.mark.parametrize("hw", G.PREPROCESS)
def test_clip_preprocess_is_the_oracles(hw):
    img = G.image01(G.rng(3), 2, *hw)
    ref, cond = R.clip_preprocess(img, G.CLIP_S)
    got = clip_preprocess(torch.from_numpy(img), G.CLIP_S).permute(0, 2, 3, 1).numpy()
    within(got, ref, cond, f"clip_preprocess {hw}", k=10.0)


def test_center_crop_rounds_halves_to_even():
    """112 x 122 at S = 56 resizes to width 61, margin 5: Python's round(2.5) = 2; rounding halves away from zero gives 3."""
    assert R.clip_resize_geometry(112, 122, 56) == (56, 61, 0, 2)
    assert R.clip_resize_geometry(80, 120, 56) == (56, 84, 0, 14) and R.clip_resize_geometry(120, 80, 56) == (84, 56, 14, 0)
    img = G.image01(G.rng(3), 2, 112, 122)
    ref, cond = R.clip_preprocess(img, 56)
    full = F.interpolate(torch.from_numpy(img), size=(56, 61), mode="bicubic", align_corners=False)
    shifted = ((full[:, :, :, 3:59].permute(0, 2, 3, 1).numpy() - R.CLIP_MEAN) / R.CLIP_STD)
    assert (np.abs(shifted - ref) > 100 * 8 * U * cond).mean() > 0.5, "a one-column shift must be far outside the tolerance"


@pytest.mark.parametrize("hw", G.BILINEAR_NORM)
def test_resize_bilinear_norm_is_torchs(hw):
    img = G.image01(G.rng(4), 2, *hw)
    ref, cond = R.resize_bilinear_norm(img, G.CLIP_S)
    x = F.interpolate(torch.from_numpy(img), size=(G.CLIP_S, G.CLIP_S), mode="bilinear", align_corners=False)
    mean, std = (torch.tensor(v.astype(np.float32)).view(1, 3, 1, 1) for v in (R.CLIP_MEAN, R.CLIP_STD))
    within(((x - mean) / std).permute(0, 2, 3, 1).numpy(), ref, cond, f"resize_bilinear_norm {hw}", k=10.0)


@pytest.mark.parametrize("src,dst", G.NEAREST)
def test_nearest_is_torchs(src, dst):
    x = G.f16(G.field(G.rng(5), (2, 8), *src))                                         # [N, C, H, W]
    got = F.interpolate(torch.from_numpy(x.astype(np.float32)), size=dst).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(R.upsample_nearest(np.moveaxis(x, 1, -1), *dst).astype(np.float32), got)


@pytest.mark.parametrize("src,dst", G.BILINEAR_ADD)
def test_bilinear_add_is_torchs(src, dst):
    g = G.rng(6)
    b = G.f16(G.field(g, (2, 8), *src)).astype(np.float32)
    a = G.f16(G.field(g, (2, 8), *dst)).astype(np.float32)
    ref, cond = R.bilinear_add(np.moveaxis(a, 1, -1), np.moveaxis(b, 1, -1), *dst)
    got = torch.from_numpy(a) + F.interpolate(torch.from_numpy(b), size=dst, mode="bilinear", align_corners=False)
    within(got.permute(0, 2, 3, 1).numpy(), ref, cond, f"bilinear_add {src} -> {dst}")


@pytest.mark.parametrize("name", list(G.STITCH))
def test_stitch_placements_have_the_overlap_counts(name):
    boxes, size = G.stitch_boxes(name)
    feat = G.field(G.rng(7), (2, len(boxes)), 8, 8 * 8).reshape(2, len(boxes), 8, 8, 8)
    ref, _, cnt = R.stitch(feat, boxes, size, size)
    want = {"k4_12": {1, 2, 4}, "k9_16": {1, 2, 4}, "k9_12": {1, 2, 3, 4, 6, 9}, "k4_16_hole": {0, 1, 2, 4}}[name]
    assert set(np.unique(cnt).tolist()) == want
    # count_mat as the reference builds it: overlap-add of ones
    ones = torch.zeros(size, size)
    acc = torch.zeros(2, size, size, 8, dtype=torch.float64)
    for k, (y, x) in enumerate(boxes):
        ones[y:y + 8, x:x + 8] += 1
        acc[:, y:y + 8, x:x + 8] += torch.from_numpy(feat[:, k])
    assert np.array_equal(cnt, ones.numpy().astype(np.int64))
    covered = cnt > 0
    assert np.allclose(ref[:, covered], (acc / ones[None, :, :, None].clamp(min=1)).numpy()[:, covered], rtol=1e-14, atol=0)
    assert (ref[:, ~covered] == 0).all()


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("hw", G.BINARIZE_HW)
def test_mask_binarize_is_sigmoid_threshold(hw, dtype):
    v = G.binarize_rows(hw, dtype)
    m01, inv, und = R.mask_binarize(v)
    t = (torch.from_numpy(v).sigmoid() > 0.5).double()
    assert np.array_equal(m01, t.numpy())
    assert np.allclose(inv, (1.0 / (t.sum(-1) + 1e-8)).numpy(), rtol=1e-15)
    assert m01[4].sum() == 0 and inv[4] == 1e8 and m01[5].all()
    assert und.mean() <= 0.005


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("src,dst", G.ATTN_MASK)
def test_attn_mask_is_torchs_and_decided(src, dst, dtype):
    v = G.attn_rows(src, dst, dtype)
    n = dst[0] * dst[1]
    out, und, fragile = R.attn_mask(v, *dst, n + 8)
    up = F.interpolate(torch.from_numpy(v)[None], size=dst, mode="bilinear", align_corners=False)[0]      # float64 torch: decided elements only
    m = (up.sigmoid().flatten(1) < 0.5)
    m[torch.where(m.sum(-1) == m.shape[-1])] = False
    sure = ~und
    assert np.array_equal(out[:, :n][sure], m.numpy().astype(np.uint8)[sure]) and (out[:, n:] == 1).all()
    share = und.mean()
    print(f"attn_mask {src} -> {dst} {np.dtype(dtype).name}: undecided share {100 * share:.4f} %")
    assert share <= 0.005 and not fragile.any()
    assert (out[6, :n] == 0).all() and (out[7, :n] == 0).sum() == 1 and 0.05 < out[:6, :n].mean() < 0.95


@pytest.mark.parametrize("scale", G.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", G.SOFTMAX_COLS)
def test_softmax_rows_is_torchs(cols, scale):
    x, _ = G.softmax_input(cols)
    v = x[:, :cols].astype(np.float64)
    ref = R.softmax_rows(v, scale)
    got = torch.softmax(torch.from_numpy(v) * scale, -1).numpy()
    assert np.abs(ref - got).max() <= 1e-15 and np.isfinite(ref).all()
    assert ref[G.SOFTMAX_SPIKE_ROW].argmax() == cols // 3 and (scale != 1.0 or ref[G.SOFTMAX_SPIKE_ROW].max() > 0.99)


@pytest.mark.parametrize("C", G.L2_C)
def test_l2_normalize_is_torchs(C):
    x = G.rng(8).standard_normal((9, C)) * 3.0
    x[2] = 0.0
    ref, _ = R.l2_normalize(x)
    assert np.abs(ref - F.normalize(torch.from_numpy(x), dim=-1).numpy()).max() <= 1e-15 and (ref[2] == 0).all()


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("scales", G.CLASSIFY_SCALES)
@pytest.mark.parametrize("K", G.CLASSIFY_K)
def test_classify_rows_is_the_reference_formula(K, scales, binary):
    c = G.classify_case(K)
    ref = R.classify_rows(c["L1"], c["L2"], c["seg"], c["ovl"], *scales, G.ALPHA, G.BETA, c["binary"] if binary else None)
    got = G.classify_torch(c, *scales, binary, torch.float64)
    # float64's own conditioning: 1 - pn carries 2^-53 absolutely, behind log(. + 1e-8): 2^-53 / 1e-8 = 1.1e-8
    assert np.abs(ref - got).max() <= 2.0 ** -53 / 1e-8 + 1e-12, np.abs(ref - got).max()
    assert np.abs(np.exp(ref).sum(-1) - (1.0 + (K + 1) * 1e-8)).max() <= 1e-12
    if not binary:
        assert (ref[4].argmax() == K), "row 4: the null text dominates"
    assert ref[5, :K].argmax() == K // 2, "row 5: one class dominates"


def test_msda_prepare_weights_are_torchs_softmax():
    B, M, Lq, off, aw, _ = G.msda_case()
    hs, ws = zip(*G.MSDA_LEVELS)
    loc, w, _ = R.msda_prepare(off, aw, hs, ws, M)
    assert np.abs(w.reshape(B, Lq, M, 12) - torch.softmax(torch.from_numpy(aw).double(), -1).numpy()).max() <= 1e-15
    # zero offsets: every sampled level gets the centre of the query's own cell; first / last cell of every level
    z, _, _ = R.msda_prepare(np.zeros_like(off), aw, hs, ws, M)
    start = 0
    for h_, w_ in G.MSDA_LEVELS:
        assert np.allclose(z[0, start, 0, :, :, :], [0.5 / w_, 0.5 / h_]) and np.allclose(z[0, start + h_ * w_ - 1, 0], [1 - 0.5 / w_, 1 - 0.5 / h_])
        start += h_ * w_
    assert np.allclose(loc - z, off / np.array([[w_, h_] for h_, w_ in G.MSDA_LEVELS])[None, None, None, :, None, :])
