"""GPU: the small kernels between the GEMM stages (csrc/decoder_ops.hip, csrc/misc.hip, the head of csrc/classify_ops.hip, mask_binarize of
csrc/elementwise.hip), each through its hook of include/odise_hip_tools.h against the float64 restatement of tests/glue_reference.py, which
tests/test_glue_reference_cpu.py holds to torch's own operators at these shapes.  The shapes are the smallest that reach each kernel's edges:
windows flush with every border, sizes that are no multiple of the vector width or of the block, every instantiation and its ragged end.

Tolerances (all derived; the restatement returns `cond` = sum |weight * tap| of every element, the operation's own fp32 conditioning):
  fp32 outputs   |got - ref| <= 8 * 2^-24 * cond
  fp16 outputs   |got - ref| <= 2^-10 * |ref| + 8 * 2^-24 * cond     (one fp16 step: an fp32 value just off a rounding boundary may land on
                 either neighbour; the inputs keep every non-zero reference value whose cond is below 1/8 inside the fp16 normal range,
                 where that holds)
  softmax_rows, classify_rows   through exp2f / expf / logf, whose error is not derived but MEASURED: the reference's formula in float32 torch
                 on the same inputs, its distance to the float64 restatement, times 4 (another valid evaluation order, 1-2 ulp functions).
                 classify_rows: per case.  softmax_rows: per row (the spike row's distance would hide every other row's), which is stricter.
  thresholded outputs   exact wherever the float64 logit is farther than 1e-3 from zero; the undecided share is capped at 0.5 % per case.
Every test prints the device's worst error next to its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_cases as G
import glue_reference as R
from odise_amd import _lib

pytestmark = pytest.mark.gpu
U, STEP16 = G.U, G.STEP16
F16, F32 = _lib.F16, _lib.F32


def call(ctx, name, *args):
    _lib.check(getattr(ctx.lib, "odise_hip_" + name)(ctx.h, *args), name)


def report(what, err, bound):
    ratio = err / np.maximum(bound, 1e-300)
    i = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
    print(f"[glue] {what}: worst err {float(err[i]):.3e} at bound {float(bound[i]):.3e} (ratio {float(ratio[i]):.3f}); max err {float(err.max()):.3e}")
    return float(ratio[i])


def check32(got, ref, cond, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert report(what, np.abs(got - ref), 8 * U * cond + 1e-300) <= 1.0, what


def check16(got, ref, cond, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    assert report(what, np.abs(got - ref), STEP16 * np.abs(ref) + 8 * U * cond + 1e-300) <= 1.0, what


def nhwc(x):
    return np.ascontiguousarray(np.moveaxis(x, 1, -1))


# ---- crops -----------------------------------------------------------------------------------------------------------------------------------------
def test_crop_extract_exact(ctx):
    """K = 6 windows of 16 x 16 in 2 x 3 x 40 x 56, four of them flush with two borders each: the windows themselves, to the bit."""
    img = G.crop_image()
    B, Cc, H, W = img.shape
    K, S = len(G.CROP_BOXES), G.CROP_S
    out = ctx.empty((B * K, Cc, S, S), np.float32)
    call(ctx, "crop_extract", ctx.to_device(img), out, B, Cc, H, W, S, K, ctx.to_device(np.array(G.CROP_BOXES, np.int32)))
    assert np.array_equal(out.numpy().astype(np.float64), R.crop_extract(img, G.CROP_BOXES, S))


@pytest.mark.parametrize("s", G.BICUBIC_S)
def test_crop_resize_bicubic(ctx, s):
    """Windows of s = 12 / 15 / 16 into 16 x 16 (s = 16: weights 0, 1, 0, 0).  The image holds 50.0 everywhere outside the windows, so a
    clamped edge tap taken from the image instead of the window is an error of that size at all four edges of every window."""
    img = G.bicubic_image(s)
    B, Cc, H, W = img.shape
    K, S = len(G.BICUBIC_BOXES), G.CROP_S
    out = ctx.empty((B * K, Cc, S, S), np.float32)
    call(ctx, "crop_resize_bicubic", ctx.to_device(img), out, B, Cc, H, W, s, S, K, ctx.to_device(np.array(G.BICUBIC_BOXES, np.int32)))
    ref, cond = R.crop_resize_bicubic(img, G.BICUBIC_BOXES, s, S)
    check32(out.numpy(), ref, cond, f"crop_resize_bicubic {s} -> {S}")


# ---- CLIP preprocess / MaskCLIP resize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", G.PREPROCESS)
def test_clip_preprocess(ctx, hw):
    """Short side on either axis, the identity path, and 112 x 122: resized width 61, crop margin 5, which center_crop halves to 2 (Python's
    round) - a kernel cropping from column 3 is a whole column off (tests/test_glue_reference_cpu.py shows that shift far outside the bound)."""
    img = G.image01(G.rng(3), 2, *hw)
    S = G.CLIP_S
    out = ctx.empty((2, S, S, 8), np.float16)
    call(ctx, "clip_preprocess", ctx.to_device(img), out, 2, hw[0], hw[1], S)
    got = out.numpy()
    assert (got[..., 3:] == 0).all(), "channels 3..7 must be exactly zero"
    ref, cond = R.clip_preprocess(img, S)
    check16(got[..., :3], ref, cond, f"clip_preprocess {hw}")


@pytest.mark.parametrize("hw", G.BILINEAR_NORM)
def test_resize_bilinear_norm(ctx, hw):
    img = G.image01(G.rng(4), 2, *hw)
    S = G.CLIP_S
    out = ctx.empty((2, S, S, 8), np.float16)
    call(ctx, "resize_bilinear_norm", ctx.to_device(img), out, 2, hw[0], hw[1], S)
    got = out.numpy()
    assert (got[..., 3:] == 0).all()
    ref, cond = R.resize_bilinear_norm(img, S)
    check16(got[..., :3], ref, cond, f"resize_bilinear_norm {hw}")


# ---- backbone projection / stitching --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("src,dst", G.NEAREST)
def test_upsample_nearest_exact(ctx, src, dst, Cc):
    x = G.f16(nhwc(G.field(G.rng(5), (2, Cc), *src)))
    out = ctx.empty((2, dst[0], dst[1], Cc), np.float16)
    call(ctx, "upsample_nearest", ctx.to_device(x), out, 2, src[0], src[1], dst[0], dst[1], Cc)
    assert np.array_equal(out.numpy(), R.upsample_nearest(x, *dst))


@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("name", list(G.STITCH))
def test_stitch_both_outputs(ctx, name, Cc):
    """8 x 8 windows: four on 12 x 12 (overlap counts 1, 2, 4), nine on 16 x 16 (1, 2, 4) and on 12 x 12 (1, 2, 3, 4, 6, 9), four on 16 x 16 leaving
    an L of pixels uncovered (count 0 -> 0).  The fp16 NHWC and fp32 NCHW outputs against the reference and against each other."""
    boxes, size = G.stitch_boxes(name)
    K = len(boxes)
    feat = G.f16(G.field(G.rng(7), (2, K), 8, 8 * Cc).reshape(2, K, 8, 8, Cc))
    o16, o32 = ctx.empty((2, size, size, Cc), np.float16), ctx.empty((2, Cc, size, size), np.float32)
    call(ctx, "stitch", ctx.to_device(feat), o16, o32, 2, K, ctx.to_device(np.array(boxes, np.int32)), 8, 8, size, size, Cc)
    ref, cond, cnt = R.stitch(feat, boxes, size, size)
    g16, g32 = o16.numpy(), np.moveaxis(o32.numpy(), 1, -1)
    check32(g32, ref, cond, f"stitch {name} C={Cc} fp32 NCHW")
    check16(g16, ref, cond, f"stitch {name} C={Cc} fp16 NHWC")
    assert np.array_equal(g16, g32.astype(np.float16)), "the two outputs must be the same sums, one rounded to fp16"
    assert (g16[:, cnt == 0] == 0).all() and (g32[:, cnt == 0] == 0).all()
    # each output alone (the other pointer NULL)
    a16, a32 = ctx.empty((2, size, size, Cc), np.float16), ctx.empty((2, Cc, size, size), np.float32)
    call(ctx, "stitch", ctx.to_device(feat), a16, None, 2, K, ctx.to_device(np.array(boxes, np.int32)), 8, 8, size, size, Cc)
    call(ctx, "stitch", ctx.to_device(feat), None, a32, 2, K, ctx.to_device(np.array(boxes, np.int32)), 8, 8, size, size, Cc)
    assert np.array_equal(a16.numpy(), g16) and np.array_equal(a32.numpy(), o32.numpy())


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("with_vec", [False, True])
def test_add_vec_table(ctx, with_vec, with_table):
    g = G.rng(8)
    N, P, Cc = 3, 5, 24
    x = G.f16(g.standard_normal((N, P, Cc)) * 2.0 + np.arange(P)[None, :, None])
    vec = (g.standard_normal(Cc) * 0.5).astype(np.float32) if with_vec else None
    table = (g.standard_normal((P, Cc)) + np.arange(Cc)[None] * 0.1).astype(np.float32) if with_table else None
    out = ctx.empty((N, P, Cc), np.float16)
    call(ctx, "add_vec_table", ctx.to_device(x), ctx.to_device(vec) if with_vec else None, ctx.to_device(table) if with_table else None, out, N, P, Cc)
    ref, cond = R.add_vec_table(x, vec, table)
    check16(out.numpy(), ref, cond, f"add_vec_table vec={with_vec} table={with_table}")
    if not with_vec and not with_table:
        assert np.array_equal(out.numpy(), x)


def test_broadcast_rows_exact(ctx):
    x = G.f16(G.rng(9).standard_normal((5, 24)) + np.arange(24)[None])
    out = ctx.empty((3, 5, 24), np.float16)
    call(ctx, "broadcast_rows", ctx.to_device(x), out, 5 * 24, 3)
    assert np.array_equal(out.numpy(), np.broadcast_to(x, (3, 5, 24)))


@pytest.mark.parametrize("with_a", [False, True])
@pytest.mark.parametrize("Cc", [8, 24])
@pytest.mark.parametrize("src,dst", G.BILINEAR_ADD)
def test_bilinear_add(ctx, src, dst, Cc, with_a):
    g = G.rng(6)
    b = G.f16(nhwc(G.field(g, (2, Cc), *src)))
    a = G.f16(nhwc(G.field(g, (2, Cc), *dst))) if with_a else None
    out = ctx.empty((2, dst[0], dst[1], Cc), np.float16)
    call(ctx, "bilinear_add", ctx.to_device(a) if with_a else None, ctx.to_device(b), out, 2, src[0], src[1], dst[0], dst[1], Cc)
    ref, cond = R.bilinear_add(a, b, *dst)
    check16(out.numpy(), ref, cond, f"bilinear_add {src} -> {dst} C={Cc} a={with_a}")
    if src == dst and not with_a:
        assert np.array_equal(out.numpy(), b), "the identity size must return the map"


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("hw", G.BINARIZE_HW)
def test_mask_binarize(ctx, hw, dtype):
    """HW = 8 / 64 / 2056 (more than one pass of the 256-thread block over the row, the last one ragged); a row of all-negative logits (count
    0 -> inv = 1e8) and one of all-positive ones.  m01 exact on decided elements; inv is 1 / (the device's own count + 1e-8) to fp32 rounding."""
    v = G.binarize_rows(hw, dtype)
    rows = v.shape[0]
    m01, inv = ctx.empty((rows, hw), np.float16), ctx.empty((rows,), np.float32)
    call(ctx, "mask_binarize_f16" if dtype == np.float16 else "mask_binarize_f32", ctx.to_device(v.astype(dtype)), m01, inv, rows, hw)
    ref, ref_inv, und = R.mask_binarize(v)
    got = m01.numpy().astype(np.float64)
    share = und.mean()
    print(f"[glue] mask_binarize {np.dtype(dtype).name} HW={hw}: undecided share {100 * share:.4f} %")
    assert share <= 0.005
    assert np.isin(got, (0.0, 1.0)).all() and np.array_equal(got[~und], ref[~und])
    cnt = got.sum(-1)
    assert (np.abs(cnt - ref.sum(-1)) <= und.sum(-1)).all()
    want = 1.0 / (cnt + 1e-8)
    check32(inv.numpy(), want, want, f"mask_binarize {np.dtype(dtype).name} HW={hw} inv")
    assert cnt[4] == 0 and cnt[5] == hw


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("src,dst", G.ATTN_MASK)
def test_attn_mask(ctx, src, dst, dtype):
    """The shortcut (equal sizes), two reductions and an enlargement; ldm above oh * ow (the padding columns must be 1); row 6 masked everywhere
    (all logits well below zero: it must come back all zero, padding still 1); row 7 with a single visible key."""
    v = G.attn_rows(src, dst, dtype)
    rows, n = v.shape[0], dst[0] * dst[1]
    ldm = (n + 7) // 8 * 8 + 8
    out = ctx.to_device(np.full((rows, ldm), 7, np.uint8))
    call(ctx, "attn_mask", ctx.to_device(v.astype(dtype)), F16 if dtype == np.float16 else F32, out, rows, src[0], src[1], dst[0], dst[1], ldm)
    ref, und, fragile = R.attn_mask(v, *dst, ldm)
    got = out.numpy()
    share = und.mean()
    mism = int((got[:, :n] != ref[:, :n])[~und].sum())
    print(f"[glue] attn_mask {np.dtype(dtype).name} {src} -> {dst}: undecided share {100 * share:.4f} %, mismatches on decided elements {mism}, "
          f"masked {100 * ref[:6, :n].mean():.1f} %")
    assert share <= 0.005 and not fragile.any()
    assert np.isin(got, (0, 1)).all() and mism == 0
    assert (got[:, n:] == 1).all(), "padding columns must be 1"
    assert (got[6, :n] == 0).all() and (got[7, :n] == 0).sum() == 1


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", G.SOFTMAX_SCALES)
@pytest.mark.parametrize("cols", G.SOFTMAX_COLS)
def test_softmax_rows(ctx, cols, scale):
    """cols = 8 .. 8192: the three instantiations (2048 / 4096 / 8192 columns) and their ragged ends; ld above cols with NaN in the input's
    padding and a sentinel in the output's, which must stay; row 3 carries a +60 spike; in place (y == x) as the VAE attention calls it."""
    x, ld = G.softmax_input(cols)
    rows = x.shape[0]
    sentinel = np.float16(7.0)
    y = ctx.to_device(np.full((rows, ld), sentinel, np.float16))
    call(ctx, "softmax_rows", ctx.to_device(x), y, rows, cols, ld, scale)
    got = y.numpy()
    assert (got[:, cols:] == sentinel).all(), "the padding of the output must be left untouched"
    inplace = ctx.to_device(x)
    call(ctx, "softmax_rows", inplace, inplace, rows, cols, ld, scale)
    gi = inplace.numpy()
    assert np.array_equal(gi[:, :cols], got[:, :cols]) and np.isnan(gi[:, cols:]).all()
    v = x[:, :cols].astype(np.float64)
    ref = R.softmax_rows(v, scale)
    measured = np.abs(G.softmax_f32(x[:, :cols], scale) - ref).max(-1)                 # per row
    err = np.abs(got[:, :cols].astype(np.float64) - ref).max(-1)
    print(f"[glue] softmax_rows cols={cols} scale={scale}: fp32-torch distance per row {np.array2string(measured, precision=3)}, "
          f"device error per row {np.array2string(err, precision=3)}, worst ratio to 4 x measured {(err / (4 * measured)).max():.3f}")
    assert np.isfinite(got[:, :cols]).all() and (err <= 4 * measured).all()


@pytest.mark.parametrize("extra,TP", [(0, 17), (5, 22), (0, 24), (5, 24)])
def test_clip_assemble(ctx, extra, TP):
    g = G.rng(10)
    B, T, Cw = 2, 17, 64
    patches = G.f16(g.standard_normal((B, T - 1, Cw)) + np.arange(T - 1)[None, :, None] * 0.25)
    cls = g.standard_normal(Cw).astype(np.float32)
    pos = (0.3 * g.standard_normal((T, Cw)) + np.arange(T)[:, None] * 0.1).astype(np.float32)
    out = ctx.to_device(np.full((B, TP, Cw), 7, np.float16))
    call(ctx, "clip_assemble", ctx.to_device(patches), ctx.to_device(cls), ctx.to_device(pos), out, B, T, extra, TP, Cw)
    ref, cond = R.clip_assemble(patches, cls, pos, extra, TP)
    got = out.numpy()
    check16(got, ref, cond, f"clip_assemble extra={extra} TP={TP}")
    assert (got[:, T + extra:] == 0).all(), "the tail rows must be zero"


def test_cond_inputs(ctx):
    g = G.rng(11)
    B, T, Cw = 2, 7, 40
    uncond, pos = g.standard_normal((T, Cw)).astype(np.float32), (0.5 * g.standard_normal((T, Cw))).astype(np.float32)
    gate = np.tanh(g.standard_normal(Cw)).astype(np.float32)
    proj = (g.standard_normal((B, Cw)) * 2.0).astype(np.float32)
    A1, A2 = (v.astype(np.float32) for v in R.cond_fold(uncond, gate, pos))
    out = ctx.empty((B, T, Cw), np.float32)
    call(ctx, "cond_inputs", ctx.to_device(proj), ctx.to_device(A1), ctx.to_device(A2), out, B, T, Cw)
    ref, cond = R.cond_inputs(uncond, gate, pos, proj)
    check32(out.numpy(), ref, cond, "cond_inputs")


@pytest.mark.parametrize("want_latent", [False, True])
def test_latent_heads(ctx, want_latent):
    g = G.rng(12)
    B, P = 2, 24
    h = G.f16(g.standard_normal((B, P, 8)) * 3.0 + np.arange(P)[None, :, None] * 0.2)
    noise = g.standard_normal((4, P)).astype(np.float32)
    wq, bq = (0.4 * g.standard_normal((4, 8))).astype(np.float32), g.standard_normal(4).astype(np.float32)
    wp, bp = (0.5 * g.standard_normal((4, 4))).astype(np.float32), g.standard_normal(4).astype(np.float32)
    scale, qa, qb = 0.18215, float(np.sqrt(0.9)), float(np.sqrt(0.1))
    xt, zd = ctx.to_device(np.full((B, P, 8), 7, np.float16)), ctx.to_device(np.full((B, P, 8), 7, np.float16))
    lat = ctx.empty((B, 4, P), np.float32) if want_latent else None
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    keep = [np.ascontiguousarray(a, np.float32) for a in (wq, bq, wp, bp)]
    call(ctx, "latent_heads", ctx.to_device(h), ctx.to_device(noise), xt, zd, lat, B, P, *(fp(a) for a in keep), scale, qa, qb)
    ref = R.latent_heads(h, noise, wq, bq, wp, bp, scale, qa, qb)
    gx, gz = xt.numpy(), zd.numpy()
    assert (gx[..., 4:] == 0).all() and (gz[..., 4:] == 0).all(), "pad channels 4..7 must be exactly zero"
    check16(gx[..., :4], *ref["xt"], "latent_heads xt")
    check16(gz[..., :4], *ref["zdec"], "latent_heads zdec")
    if want_latent:
        check32(lat.numpy(), *ref["latent"], "latent_heads latent")


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
@pytest.mark.parametrize("Cc", G.L2_C)
@pytest.mark.parametrize("rows", G.L2_ROWS)
def test_l2_normalize(ctx, rows, Cc, dtype):
    """rows = 1, 4, 5, 9 around the four-rows-per-block edge; C = 32 (half a wavefront), 100 (ragged), 768; an all-zero row -> zeros."""
    g = G.rng(13)
    x = ((0.5 + np.abs(g.standard_normal((rows, Cc))) * 3.0) * np.where(g.random((rows, Cc)) < 0.5, -1.0, 1.0)).astype(dtype)   # no element near zero
    if rows > 1:
        x[rows // 2] = 0
    out = ctx.to_device(np.full((rows, Cc), 7, np.float16))
    call(ctx, "l2_normalize", ctx.to_device(x), F16 if dtype == np.float16 else F32, out, rows, Cc)
    ref, cond = R.l2_normalize(x.astype(np.float64))
    got = out.numpy()
    check16(got, ref, cond, f"l2_normalize rows={rows} C={Cc} {np.dtype(dtype).name}")
    assert rows == 1 or (got[rows // 2] == 0).all()


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("scales", G.CLASSIFY_SCALES)
@pytest.mark.parametrize("K", G.CLASSIFY_K)
def test_classify_rows(ctx, K, scales, binary):
    """K = 1, 5, 300 (more than the 256 threads); synonym groups of 1..4; ovl mixed; logit scales 100 and 14 on either bank; row 4: the null text
    dominates, row 5: one class dominates by 40; the learned binary head given and NULL."""
    c = G.classify_case(K)
    rows = c["L1"].shape[0]
    out = ctx.empty((rows, K + 1), np.float32)
    call(ctx, "classify_rows", ctx.to_device(c["L1"]), ctx.to_device(c["L2"]), ctx.to_device(c["seg"]), ctx.to_device(c["ovl"]),
         ctx.to_device(c["binary"]) if binary else None, out, rows, K, c["Ktot"], scales[0], scales[1], G.ALPHA, G.BETA)
    ref = R.classify_rows(c["L1"], c["L2"], c["seg"], c["ovl"], *scales, G.ALPHA, G.BETA, c["binary"] if binary else None)
    measured = float(np.abs(G.classify_torch(c, *scales, binary, torch.float32) - ref).max())
    got = out.numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    total = float(np.abs(np.exp(got).sum(-1) - 1.0).max())
    print(f"[glue] classify_rows K={K} scales={scales} binary={binary}: fp32-torch distance {measured:.3e}, device error {err:.3e} "
          f"(ratio to 4 x measured {err / (4 * measured):.3f}); |sum exp - 1| {total:.3e}")
    assert np.isfinite(got).all() and err <= 4 * measured
    assert total <= 4 * measured + (K + 1) * 1e-8
    assert got[5, :K].argmax() == K // 2 and (binary or got[4].argmax() == K)


# ---- MSDeformAttn's prologue ----------------------------------------------------------------------------------------------------------------------
def test_msda_prepare_through_the_two_kernel_hook(ctx):
    """msda_prepare_kernel<3, 4> through odise_hip_msda_fused_forward(fused = 0): levels 4 x 6, 8 x 12, 16 x 24, every cell a query (so the
    first and last cell of every level are there), M = 8.  loc to the fp32 bound of ref + off / size.  w: expf of (a - max) carries
    |a - max| * 2^-24 from the subtraction and <= 2 ulp of its own; the 12-term sum, the reciprocal and the product add 11 + 1 + 1 half-steps:
    |w - ref| <= (24 + |a - max|) * 2^-24 * ref, and the weights of a (row, head) sum to 1 within 16 * 2^-24."""
    B, M, Lq, off, aw, value = G.msda_case()
    hs, ws = zip(*G.MSDA_LEVELS)
    loc_s, w_s = ctx.empty((B, Lq, M, 3, 4, 2), np.float32), ctx.empty((B, Lq, M, 3, 4), np.float32)
    out = ctx.empty((B * Lq, M * 32), np.float16)
    call(ctx, "msda_fused_forward", ctx.to_device(value), ctx.to_device(off.reshape(B * Lq, -1)), ctx.to_device(aw.reshape(B * Lq, -1)),
         (C.c_int * 3)(*hs), (C.c_int * 3)(*ws), B, M, 0, out, loc_s, w_s)
    loc, w, cond = R.msda_prepare(off, aw, hs, ws, M)
    check32(loc_s.numpy(), loc, cond, "msda_prepare loc")
    gw = w_s.numpy().astype(np.float64)
    a = aw.astype(np.float64)
    spread = (a.max(-1, keepdims=True) - a).reshape(w.shape)
    assert report("msda_prepare w", np.abs(gw - w), (24 + spread) * U * w) <= 1.0
    tot = np.abs(gw.reshape(B, Lq, M, 12).sum(-1) - 1.0).max()
    print(f"[glue] msda_prepare: |sum w - 1| max {tot:.3e} (bound {16 * U:.3e})")
    assert tot <= 16 * U
    start = 0
    for h_, w_ in G.MSDA_LEVELS:                       # the reference points the first and last cell of every level sample around
        for q, (cx, cy) in ((start, (0.5 / w_, 0.5 / h_)), (start + h_ * w_ - 1, (1 - 0.5 / w_, 1 - 0.5 / h_))):
            d = loc_s.numpy()[0, q, 0].astype(np.float64) - off[0, q, 0] / np.array([[w2, h2] for h2, w2 in G.MSDA_LEVELS])[:, None, :]
            assert np.abs(d - [cx, cy]).max() <= 8 * U * (1 + np.abs(off[0, q, 0]).max()), (q, d)
        start += h_ * w_
