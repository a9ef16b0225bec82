"""Crafted problems for the GEMM / convolution library (csrc/gemm.hip), shared by tests/test_gemm_reference_cpu.py (preconditions, the reference
against torch) and tests/test_gpu_gemm_exact.py (the kernels against the reference, bit for bit).

Exactness: A and W (X and Wt) are integers in [-3, 3] stored as fp16, so every partial sum in any order and any split is an integer of magnitude
<= 9 K < 2^24 and the fp32 accumulators are exact whatever the kernel does.  alpha is 1 or 2^-3, scale_m in {1/2, 1, 2}, bias_n / bias_m /
rowgroup_add multiples of 1/4 in [-8, 8], the residual an fp16 multiple of 1/4 in [-64, 64], the activation none or ReLU: every intermediate is a
multiple of 2^-4 below 2^24 * 2^-4 (`worst_intermediate` states the bound per case), the fp32 result is exact and an fp16 output is its one RNE
rounding.  tests/gemm_reference.py computes the same in float64; the comparison is on bit patterns, no tolerance, no element excluded.

Memory: a problem owns flat host buffers in which every matrix sits at its own (offset, row pitch, batch stride).  Whatever the kernel has no
business reading - columns between K (or N) and the pitch, rows after the last one, the gaps between batches - is NaN; whatever it has no business
writing carries SENTINEL bits, and the test compares the WHOLE output buffer (guard rows and gaps included) with the expected image.  Every buffer
is large enough that such an access would stay inside the allocation."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import gemm_reference as R
from odise_amd import _lib

F16, F32 = _lib.F16, _lib.F32
NP_OUT = {F16: np.float16, F32: np.float32}
BITS = {F16: np.uint16, F32: np.uint32}
SENTINEL = {F16: 0xCAFE, F32: 0xCAFEF00D}
GUARD_ROWS = 64
STEP16 = 2.0 ** -10     # one fp16 step, relative

# csrc/gemm.hip kTileBM / kTileBN
TILE_BM = (128, 64, 64, 256, 256, 256, 512, 256, 256, 256)
TILE_BN = (128, 128, 64, 320, 256, 128, 128, 256, 128, 128)
DENSE_TILES = (0, 1, 2, 3, 4, 5, 6)
PLAIN_K = (8, 64, 72, 136, 192)          # one partial K-tile, whole tiles, ragged last tiles
PP_K = (64, 128, 192, 256, 576)          # 1, 2, 3, 4, 9 K-tiles: both parities of the ping-pong tail
# odise_hip_gemm_debug switches (csrc/gemm.hip SelectFlag << 4); PP2 / PP / BLOCK as in tests/test_gpu_ops.py
PP2, PP, BLOCK = 512 << 4, 1024 << 4, 32768 << 4
NOPP = 2 << 4                            # kFlagNoPingPong: the plain kernel also where K % 64 == 0


def tile_modes(tile):
    """[(debug flags, K list, kernel family the launch must take)] of one dense tile: tiles 3 / 4 have a plain and two ping-pong forms, 6 only
    the ping-pong ones, the others only the plain one; the 8-wave tiles also run with the block-wide epilogues."""
    if tile in (3, 4):
        return [(NOPP, PLAIN_K), (PP2, PP_K), (PP, PP_K), (BLOCK, tuple(sorted(set(PLAIN_K + PP_K))))]
    if tile == 6:
        return [(PP2, PP_K), (PP, PP_K), (BLOCK, PP_K)]
    if tile == 5:
        return [(0, PLAIN_K), (BLOCK, PLAIN_K)]
    return [(0, PLAIN_K)]


def dense_mn(tile):
    """Two row blocks, the second ragged and odd; a second column block of 8 and of 3 columns."""
    return TILE_BM[tile] + 9, (TILE_BN[tile] + 8, TILE_BN[tile] + 3)


def round_up(x, m):
    return (x + m - 1) // m * m


# ---- epilogues --------------------------------------------------------------------------------------------------------------------------------------
# name -> terms present.  rows_per_group is the layout's to choose (default 7: groups that straddle the row blocks).
EPILOGUES = {
    "none": dict(),
    "bias_res_relu": dict(alpha=0.125, bias_n=True, residual=True, act=R.ACT_RELU),
    "rows": dict(scale_m=True, bias_m=True, rowgroup=True),
    "all": dict(alpha=0.125, scale_m=True, bias_n=True, bias_m=True, rowgroup=True, residual=True, act=R.ACT_RELU),
    "bias_res": dict(bias_n=True, residual=True),
}


def worst_intermediate(K, epi):
    """(largest magnitude any intermediate of the epilogue can reach, the power of two all of them are multiples of)."""
    alpha = epi.get("alpha", 1.0)
    s = 2.0 if epi.get("scale_m") else 1.0
    worst = 9.0 * K * max(1.0, alpha * s) + 8.0 * sum(bool(epi.get(k)) for k in ("bias_n", "bias_m", "rowgroup")) + (64.0 if epi.get("residual") else 0.0)
    gran = min(1.0, alpha) * (0.5 if epi.get("scale_m") else 1.0)
    if any(epi.get(k) for k in ("bias_n", "bias_m", "rowgroup", "residual")):
        gran = min(gran, 0.25)
    return worst, gran


def _ints(rng, shape):
    return rng.integers(-3, 4, size=shape).astype(np.float16)


def _quarters(rng, shape, lim):
    return rng.integers(-4 * lim, 4 * lim + 1, size=shape) / 4.0


def _place(buf, mat, ld, stride, off):
    """mat [B, R, Cc] into the flat buffer at off + b * stride + r * ld + c."""
    B, Rr, Cc = mat.shape
    idx = off + np.arange(B, dtype=np.int64)[:, None, None] * stride + np.arange(Rr, dtype=np.int64)[None, :, None] * ld + np.arange(Cc, dtype=np.int64)[None, None, :]
    assert B == 1 or stride >= Rr * ld or stride == 0, "batches would overlap"
    assert idx.max() < buf.size
    buf[idx] = mat


def _span(B, Rr, ld, stride, off):
    return round_up(off + (B - 1) * stride + (Rr + GUARD_ROWS) * ld + 64, 64)


def _as3(x):
    return x if x.ndim == 3 else x[None]


# ---- dense problems ---------------------------------------------------------------------------------------------------------------------------------
def gemm_problem(M, N, K, *, dtype=F16, epi="none", batch=1, a_batched=True, w_batched=True, lda=None, ldw=None, ldc=None, ldr=None, ldg=0,
                 strideC=None, offA=0, offC=0, offR=0, interleaved=False, rows_per_group=7, alpha=None, geglu=False, act=None, seed=0):
    """One odise_gemm_desc recipe with its host buffers, the exact pre-activation x (float64) and, for the exact epilogues, the expected image of
    the whole output buffer.  Offsets, pitches and strides are in elements."""
    e = dict(EPILOGUES[epi])
    if alpha is not None:
        e["alpha"] = alpha
    if act is not None:
        e["act"] = act
    rng = np.random.default_rng([M, N, K, batch, seed])
    A = _ints(rng, (batch if (batch > 1 and a_batched) else 1, M, K))
    W = _ints(rng, (batch if (batch > 1 and w_batched) else 1, N, K))
    No = N // 2 if geglu else N
    p = SimpleNamespace(M=M, N=N, K=K, No=No, batch=batch, dtype=dtype, epi=e, geglu=geglu, rows_per_group=rows_per_group)
    if interleaved:      # A and W are the two halves of the rows of one [rows, 2 K] buffer (the CLIP towers' q | k)
        assert batch == 1
        lda = ldw = 2 * K
        ab = np.full(_span(1, max(M, N), 2 * K, 0, 0), np.nan, np.float16)
        _place(ab, A, lda, 0, 0)
        _place(ab, W, ldw, 0, K)
        p.bufA, p.bufW, p.offA, p.offW = ab, None, 0, K
        p.strideA = p.strideW = 0
    else:
        lda, ldw = lda or K, ldw or K
        p.strideA = (M * lda + 8) if A.shape[0] > 1 else 0       # + 8: a NaN gap between the batches
        p.strideW = (N * ldw + 8) if W.shape[0] > 1 else 0
        p.bufA = np.full(_span(A.shape[0], M, lda, p.strideA, offA), np.nan, np.float16)
        p.bufW = np.full(_span(W.shape[0], N, ldw, p.strideW, 0), np.nan, np.float16)
        _place(p.bufA, A, lda, p.strideA, offA)
        _place(p.bufW, W, ldw, p.strideW, 0)
        p.offA, p.offW = offA, 0
    p.lda, p.ldw = lda, ldw
    p.ldc = ldc or No
    p.strideC = strideC if strideC is not None else M * p.ldc
    p.offC = offC
    # epilogue terms
    p.alpha = float(e.get("alpha", 1.0))
    p.scale_m = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=M) if e.get("scale_m") else None
    p.bias_n = _quarters(rng, N, 8).astype(np.float32) if e.get("bias_n") else None
    p.bias_m = _quarters(rng, M, 8).astype(np.float32) if e.get("bias_m") else None
    p.ldg = ldg
    p.rowgroup = None
    if e.get("rowgroup"):
        groups = (M + rows_per_group - 1) // rows_per_group
        p.rowgroup = _quarters(rng, (groups, N), 8).astype(np.float32)
        p.bufG = np.full((groups + 1) * (ldg or N) + 64, np.nan, np.float32)
        _place(p.bufG, p.rowgroup[None], ldg or N, 0, 0)
    p.residual = None
    p.ldr, p.strideR, p.offR = ldr or No, 0, offR
    if e.get("residual"):
        p.residual = _quarters(rng, (batch, M, No), 64).astype(np.float16)
        p.strideR = M * p.ldr + 8 if batch > 1 else 0
        p.bufR = np.full(_span(batch, M, p.ldr, p.strideR, offR), np.nan, np.float16)
        _place(p.bufR, p.residual, p.ldr, p.strideR, offR)
    p.act = e.get("act", R.ACT_NONE)
    # reference
    p.acc = _as3(R.matmul_nt(A if A.shape[0] > 1 else A[0], W if W.shape[0] > 1 else W[0]))
    if p.acc.shape[0] != batch:
        p.acc = np.broadcast_to(p.acc, (batch, M, N))
    p.x = R.pre_activation(p.acc, alpha=p.alpha, scale_m=p.scale_m, bias_n=p.bias_n, bias_m=p.bias_m, rowgroup_add=p.rowgroup, rows_per_group=rows_per_group)
    p.total_c = _span(batch, M, p.ldc, p.strideC, offC)
    p.expected = None
    if not geglu and p.act in (R.ACT_NONE, R.ACT_RELU):
        p.out = R.finish(p.x, p.act, p.residual, NP_OUT[dtype])
        img = np.full(p.total_c, SENTINEL[dtype], BITS[dtype])
        _place(img, p.out.view(BITS[dtype]), p.ldc, p.strideC, offC)
        p.expected = img
    return p


def out_region(p, flat_bits):
    """[batch, M, No] of the output buffer, as the output type."""
    idx = p.offC + np.arange(p.batch, dtype=np.int64)[:, None, None] * p.strideC + np.arange(p.M, dtype=np.int64)[None, :, None] * p.ldc + np.arange(p.No, dtype=np.int64)[None, None, :]
    return flat_bits[idx].view(NP_OUT[p.dtype])


# Layouts: name -> [keyword sets of gemm_problem] for one (M, N, K); each entry is one launch recipe named after the call site it mirrors.
def layout_variants(layout, M, N, K):
    if layout == "natural":
        return [dict(dtype=F16, epi=e) for e in ("none", "bias_res_relu", "all")] + [dict(dtype=F32, epi=e) for e in ("none", "rows")]
    if layout == "padded_out":      # V^T rows padded to ldvt, batches of C * ldvt
        out = []
        for ldc in (N + 8, round_up(N, 8) + 8):
            for dt, e in ((F16, "bias_res_relu"), (F32, "bias_res"), (F16, "none")):
                out.append(dict(dtype=dt, epi=e, batch=2, ldc=ldc, strideC=M * ldc + 16, ldr=ldc))
        return out
    if layout == "interleaved_qk":  # extractor.cpp: q and k read out of one [rows, 2 C] buffer
        return [dict(dtype=F16, epi="none", interleaved=True), dict(dtype=F32, epi="rows", interleaved=True)]
    if layout == "gathered_rows":   # extractor.cpp: CLS rows gathered with lda = TP * Wd, the residual likewise
        return [dict(dtype=dt, epi=e, lda=5 * K, ldr=5 * N, offA=16, offR=8) for dt, e in ((F16, "bias_res_relu"), (F32, "bias_res"), (F16, "all"))]
    if layout == "odd_ldc_f32":     # maskgen.cpp / classify.cpp: fp32 logits with ldc = Ktot + 1 and ldc = 2
        if N % 2 == 0:
            return []
        return [dict(dtype=F32, epi=e) for e in ("none", "all")]
    if layout == "odd_base_f16":    # an output that starts one element into its buffer: only the scalar epilogue is legal
        return [dict(dtype=F16, epi=e, offC=1, offR=1) for e in ("none", "bias_res_relu")]
    if layout == "batched":         # batch 3: the shared-A V^T trick and both operands batched, a padded strideC
        return [dict(dtype=F16, epi="none", batch=3, a_batched=False, strideC=M * N + 16),
                dict(dtype=F16, epi="bias_res_relu", batch=3, strideC=M * N + 24),
                dict(dtype=F32, epi="rows", batch=3, a_batched=False)]
    if layout == "rowgroup_ld":     # the time-embedding broadcast read out of a wider table
        return [dict(dtype=dt, epi=e, rows_per_group=g, ldg=N + 4) for g in (1, 7) for dt, e in ((F16, "all"), (F32, "rows"))]
    raise KeyError(layout)


LAYOUTS = ("natural", "padded_out", "interleaved_qk", "gathered_rows", "odd_ldc_f32", "odd_base_f16", "batched", "rowgroup_ld")
SMALL_F32 = [(1, 2), (100, 2)]          # odd_ldc_f32's second form: (M, N) with ldc = N = 2 (maskgen.cpp's two-logit head)
SPLIT_CASES = [(576, 2), (576, 3), (576, 4), (136, 2)]   # 9 K-tiles as 5 + 4, 3 + 3 + 3, ceil -> 3 splits; the last split owning the 8-column partial tile
SPLIT_LAYOUTS = ("natural", "padded_out", "gathered_rows", "odd_ldc_f32", "odd_base_f16", "rowgroup_ld")   # gathered_rows: ldr != ldc in the reduce kernel


def split_variants(layout, M, N, K):
    """The split-K launches: the reduce kernel owns the epilogue and there is no batch."""
    if layout == "padded_out":
        ldc = N + 8
        return [dict(dtype=dt, epi=e, ldc=ldc, strideC=M * ldc + 16, ldr=ldc) for dt, e in ((F16, "bias_res_relu"), (F32, "bias_res"))]
    return [v for v in layout_variants(layout, M, N, K) if v.get("batch", 1) == 1]


STATS_CASE = dict(M=265, N=256, K=128, alpha=0.125)     # the producer statistics of odise_hip_gemm_ln: tile 4, N % 64 == 0


# ---- device side ------------------------------------------------------------------------------------------------------------------------------------
def _dev(ctx, host, off=0):
    """(owner, view at element offset `off`) of a flat host buffer on the device."""
    d = ctx.to_device(host)
    n = host.size - off
    return d, d.view((n,), offset_bytes=off * host.dtype.itemsize)


def upload(ctx, p):
    """Device buffers of a problem and its filled odise_gemm_desc (kept alive by the returned namespace)."""
    u = SimpleNamespace(keep=[])
    d = _lib.GemmDesc()
    d.M, d.N, d.K = p.M, p.N, p.K
    ownA, vA = _dev(ctx, p.bufA, p.offA)
    u.keep.append(ownA)
    if p.bufW is None:
        vW = ownA.view((p.bufA.size - p.offW,), offset_bytes=p.offW * 2)
    else:
        ownW, vW = _dev(ctx, p.bufW, p.offW)
        u.keep.append(ownW)
    d.A, d.lda, d.W, d.ldw = vA.ptr, p.lda, vW.ptr, p.ldw
    u.out = ctx.empty((p.total_c,), BITS[p.dtype])
    u.sentinel = np.full(p.total_c, SENTINEL[p.dtype], BITS[p.dtype])
    vC = u.out.view((p.total_c - p.offC,), offset_bytes=p.offC * u.out.dtype.itemsize)
    d.C, d.ldc, d.c_dtype = vC.ptr, p.ldc, p.dtype
    for name, host in (("bias_n", p.bias_n), ("bias_m", p.bias_m), ("scale_m", p.scale_m)):
        if host is not None:
            u.keep.append(ctx.to_device(host))
            setattr(d, name, u.keep[-1].ptr)
    if p.residual is not None:
        ownR, vR = _dev(ctx, p.bufR, p.offR)
        u.keep.append(ownR)
        d.residual = vR.ptr
    d.ldr = p.ldr
    if p.rowgroup is not None:
        u.keep.append(ctx.to_device(p.bufG))
        d.rowgroup_add = u.keep[-1].ptr
    d.rows_per_group, d.ldg = p.rows_per_group, p.ldg
    d.act, d.geglu, d.alpha = p.act, int(p.geglu), p.alpha
    d.batch = p.batch
    d.strideA, d.strideW, d.strideC, d.strideR = p.strideA, p.strideW, p.strideC, p.strideR
    u.desc = d
    return u


def run_gemm(ctx, p, u, tile, split=1):
    """One forced launch into the sentinel-filled output buffer; returns the whole buffer's bits.  Asserts that the forced tile and split ran."""
    u.out.copy_from(u.sentinel)
    _lib.check(ctx.lib.odise_hip_gemm_forced(ctx.h, C.byref(u.desc), int(tile), int(split)), "gemm_forced")
    ran = ctx.lib.odise_hip_last_tile()
    nk = (p.K + 63) // 64
    want = tile | (min(split, nk) if p.batch == 1 else 1) << 8
    assert ran == want, f"forced tile {tile} split {split}: the library ran tile {ran & 255} split {ran >> 8}"
    return u.out.numpy()


def describe(p, kw):
    return (f"M={p.M} N={p.N} K={p.K} " + " ".join(f"{k}={v}" for k, v in sorted(kw.items())))


def first_mismatch(got, exp, p):
    bad = np.flatnonzero(got != exp)
    if bad.size == 0:
        return ""
    i = int(bad[0])
    rel = i - p.offC
    b = rel // p.strideC if p.batch > 1 and p.strideC else 0
    r, c = divmod(rel - b * (p.strideC if p.batch > 1 else 0), p.ldc)
    return f"{bad.size} of {got.size} buffer elements differ; first at flat {i} (batch {b} row {r} col {c}): got bits {int(got[i]):#x}, expected {int(exp[i]):#x}"


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------------------
CONV_N, CONV_HW, CONV_SRC_HW = 2, (17, 33), (9, 17)      # ragged 16 x 16 patches both ways; the upsampled runs gather from 9 x 17
HALO_TILES, HALO_CIN, HALO_COUT = (7, 8, 9), (64, 192), (72, 128, 264)
IGEMM_TILES, IGEMM_CIN, IGEMM_COUT = (0, 2, 4, 5, 6), (24, 64, 72), (72, 136)
# name -> (k, stride, pad_tl, out_hw)
IGEMM_GEOMS = {"3x3": (3, 1, (1, 1), CONV_HW), "3x3s2": (3, 2, (0, 0), (9, 17)), "1x1": (1, 1, (0, 0), CONV_HW)}
CONV_EPILOGUES = [(F16, dict(bias=True, residual=True, per_image=True)), (F16, dict(bias=True, act=R.ACT_RELU)), (F32, dict(bias=True, residual=True, per_image=True)),
                  (F32, dict())]
PAD_X = 4096         # NaN elements before and after the input map


def conv_problem(Cin, Cout, *, k=3, stride=1, pad_tl=(1, 1), out_hw=None, ups=False, dtype=F16, epi=None, hw=None, seed=0):
    e = dict(epi or {})
    N = CONV_N
    H, W = hw or (CONV_SRC_HW if ups else CONV_HW)
    OH, OW = out_hw or ((2 * H, 2 * W) if ups else (H, W))
    rng = np.random.default_rng([Cin, Cout, k, stride, int(ups), seed])
    X = _ints(rng, (N, H, W, Cin))
    Wt = _ints(rng, (Cout, k, k, Cin))
    p = SimpleNamespace(N=N, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad_tl=pad_tl, OH=OH, OW=OW, ups=ups, dtype=dtype, epi=e, X=X, Wt=Wt)
    p.K = k * k * Cin
    p.M = N * OH * OW
    p.bufX = np.full(2 * PAD_X + X.size, np.nan, np.float16)
    p.bufX[PAD_X:PAD_X + X.size] = X.reshape(-1)
    p.bufW = np.full((Cout + GUARD_ROWS) * p.K, np.nan, np.float16)
    p.bufW[:Wt.size] = Wt.reshape(-1)
    p.bias = _quarters(rng, Cout, 8).astype(np.float32) if e.get("bias") else None
    p.per_image, p.ldp = None, Cout + 4
    if e.get("per_image"):
        p.per_image = _quarters(rng, (N, Cout), 8).astype(np.float32)
        p.bufP = np.full((N + 1) * p.ldp, np.nan, np.float32)
        _place(p.bufP, p.per_image[None], p.ldp, 0, 0)
    p.residual = _quarters(rng, (N, OH, OW, Cout), 64).astype(np.float16) if e.get("residual") else None
    p.act = e.get("act", R.ACT_NONE)
    p.acc = R.conv2d_nhwc(X, Wt, stride=stride, pad_tl=pad_tl, out_hw=(OH, OW), upsample2x=ups)
    x = p.acc.reshape(N, OH * OW, Cout)
    if p.bias is not None:
        x = x + p.bias.astype(np.float64)
    if p.per_image is not None:
        x = x + p.per_image.astype(np.float64)[:, None, :]
    p.x = x
    res = p.residual.reshape(N, OH * OW, Cout) if p.residual is not None else None
    p.out = R.finish(x, p.act, res, NP_OUT[dtype]).reshape(p.M, Cout)
    p.expected = np.full((p.M + GUARD_ROWS) * Cout, SENTINEL[dtype], BITS[dtype])
    p.expected[:p.M * Cout] = p.out.view(BITS[dtype]).reshape(-1)
    return p


def conv_worst_intermediate(p):
    return worst_intermediate(p.K, dict(bias_n=p.bias is not None, rowgroup=p.per_image is not None, residual=p.residual is not None))


def upload_conv(ctx, p):
    u = SimpleNamespace(keep=[])
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cin = p.N, p.H, p.W, p.Cin
    d.Cout, d.KH, d.KW, d.stride = p.Cout, p.k, p.k, p.stride
    d.pad_t, d.pad_l, d.OH, d.OW = p.pad_tl[0], p.pad_tl[1], p.OH, p.OW
    d.upsample2x = int(p.ups)
    ownX, vX = _dev(ctx, p.bufX, PAD_X)
    u.keep += [ownX, ctx.to_device(p.bufW)]
    d.X, d.Wt = vX.ptr, u.keep[-1].ptr
    u.out = ctx.empty((p.expected.size,), BITS[p.dtype])
    u.sentinel = np.full(p.expected.size, SENTINEL[p.dtype], BITS[p.dtype])
    d.Y, d.y_dtype = u.out.ptr, p.dtype
    if p.bias is not None:
        u.keep.append(ctx.to_device(p.bias))
        d.bias = u.keep[-1].ptr
    if p.residual is not None:
        u.keep.append(ctx.to_device(p.residual))
        d.residual = u.keep[-1].ptr
    if p.per_image is not None:
        u.keep.append(ctx.to_device(p.bufP))
        d.per_image_add, d.per_image_add_ld = u.keep[-1].ptr, p.ldp
    d.act = p.act
    u.desc = d
    return u


def run_conv(ctx, p, u, tile, split=1):
    u.out.copy_from(u.sentinel)
    _lib.check(ctx.lib.odise_hip_conv2d_forced(ctx.h, C.byref(u.desc), int(tile), int(split)), "conv2d_forced")
    ran = ctx.lib.odise_hip_last_tile()
    assert (ran & 255) == tile and (ran >> 8) == split, f"forced tile {tile} split {split}: the library ran tile {ran & 255} split {ran >> 8}"
    return u.out.numpy()


# ---- inexact activations on exact pre-activations -----------------------------------------------------------------------------------------------------
ACTIVATIONS = {"silu": R.ACT_SILU, "gelu": R.ACT_GELU, "quickgelu": R.ACT_QUICKGELU}
ACT_TILES = (0, 2, 4, 5, 6)
ACT_K_ALPHA = ((64, 2.0 ** -3), (576, 2.0 ** -5))      # pre-activations spread over roughly [-8, 8]


def act_reference(p):
    """(float64 reference, float32 restatement of csrc/common.h) of an activation / GEGLU problem, on the exact pre-activations."""
    x32 = p.x.astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), p.x)
    if p.geglu:
        return R.geglu(p.x), R.geglu_f32(x32).astype(np.float64)
    return R.activate(p.x, p.act), R.activate_f32(x32, p.act).astype(np.float64)
