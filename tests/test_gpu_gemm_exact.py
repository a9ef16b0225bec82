"""GPU: the GEMM / convolution library (csrc/gemm.hip) against the exact reference of tests/gemm_reference.py on the crafted problems of
tests/gemm_cases.py - every kernel family (the plain tiles, both ping-pong generations, the halo convolutions, the split-K reduction) under
every epilogue form (scalar, 8-column fast, math-first fp16, wave-private and block-wide), forced through odise_hip_gemm_forced /
odise_hip_conv2d_forced with every stride field of the descriptors set the way the model's call sites set them.

Inputs are small integers and dyadic epilogue terms (tests/test_gemm_reference_cpu.py shows that fp32 holds every intermediate exactly), so a
kernel that takes every k-step of every K-tile exactly once, whose split-K partition is a partition and whose padding contributes nothing, must
produce the reference's bits: `np.array_equal` on the WHOLE output buffer - the sentinel-filled pitch padding, guard rows and batch gaps included -
with no tolerance and no element excluded.  Whatever the kernel must not read is NaN.

The inexact activations (SiLU, GELU, QuickGELU, GEGLU) run on the same exact pre-activations and are held to
    |got - ref| <= 2^-10 |ref| + 4 x (distance of the float32 restatement of csrc/common.h from float64 on the same grid),
the rule of tests/test_gpu_glue_ops.py for operations through the device's fast exp / reciprocal; both numbers are printed."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as G
import gemm_reference as R
from odise_amd import _lib

pytestmark = pytest.mark.gpu
F16, F32 = G.F16, G.F32


def _check_exact(got, p, what):
    assert np.array_equal(got, p.expected), f"{what}: {G.first_mismatch(got, p.expected, p)}"


def _dense_sweep(ctx, tile, problems, modes):
    """problems: iterable of (K, keyword set, problem); every problem runs once under every mode whose K list holds its K."""
    launches = 0
    try:
        for K, kw, p in problems:
            u = G.upload(ctx, p)
            for flags, ks in modes:
                if K not in ks:
                    continue
                ctx.lib.odise_hip_gemm_debug(flags)
                got = G.run_gemm(ctx, p, u, tile)
                _check_exact(got, p, f"tile {tile} flags {flags >> 4} {G.describe(p, kw)}")
                launches += 1
    finally:
        ctx.lib.odise_hip_gemm_debug(0)
    return launches


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("tile", G.DENSE_TILES)
def test_dense_tiles_at_real_strides(ctx, tile, layout):
    """Two row blocks (the second ragged and odd) x two column blocks (8 and 3 columns into the second), every K of the tile's kernel forms, every
    launch recipe of the layout; tiles 3 / 4 as the plain kernel and as both ping-pong generations, the 8-wave tiles also with the block-wide
    epilogues.  (padded_out on tiles 4 - 6 is where the wave-private epilogue was found to leave the ragged last 8-column chunk unwritten: an
    aligned pitch with N % 8 != 0 - V^T rows padded to ldvt - passes every `fast` predicate, and that form only stored whole chunks.)"""
    M, Ns = G.dense_mn(tile)
    modes = G.tile_modes(tile)
    ks = sorted({k for _, kl in modes for k in kl})

    def problems():
        for N in Ns:
            for K in ks:
                for kw in G.layout_variants(layout, M, N, K):
                    yield K, kw, G.gemm_problem(M, N, K, **kw)
        if layout == "odd_ldc_f32":
            for m, n in G.SMALL_F32:
                for K in ks:
                    for e in ("none", "all"):
                        kw = dict(dtype=F32, epi=e)
                        yield K, kw, G.gemm_problem(m, n, K, **kw)

    n = _dense_sweep(ctx, tile, problems(), modes)
    print(f"[gemm] tile {tile} {layout}: {n} launches bit-equal to the reference, guards untouched")
    assert n >= len(ks)


@pytest.mark.parametrize("layout", G.SPLIT_LAYOUTS)
@pytest.mark.parametrize("tile", G.DENSE_TILES)
def test_split_k_partitions_and_reduce_epilogue(ctx, tile, layout):
    """9 K-tiles as 5 + 4, 3 + 3 + 3 and a requested 4 that becomes 3; 3 K-tiles as 2 + 1 where the last split owns only the 8-column partial
    tile.  The reduce kernel owns the epilogue: its vector and scalar forms at every pitch."""
    M, Ns = G.dense_mn(tile)
    pp_form = tile in (3, 4, 6)
    n = 0
    try:
        for N in Ns:
            for K, split in G.SPLIT_CASES:
                if tile == 6 and K % 64:
                    continue        # the 512 x 128 tile only exists as a ping-pong kernel (K % 64 == 0)
                for kw in G.split_variants(layout, M, N, K):
                    p = G.gemm_problem(M, N, K, **kw)
                    u = G.upload(ctx, p)
                    for flags in ((G.PP2, G.PP) if pp_form and K % 64 == 0 else (0,)):
                        ctx.lib.odise_hip_gemm_debug(flags)
                        got = G.run_gemm(ctx, p, u, tile, split)
                        _check_exact(got, p, f"tile {tile} split {split} flags {flags >> 4} {G.describe(p, kw)}")
                        n += 1
    finally:
        ctx.lib.odise_hip_gemm_debug(0)
    print(f"[gemm] tile {tile} {layout}: {n} split-K launches bit-equal to the reference")
    assert n > 0


def test_producer_statistics_are_exact(ctx):
    """odise_hip_gemm_ln's stats_out on the 256 x 256 tile: per-64-column (sum, sum of squares) of the rounded outputs are integers of granules
    below 2^24 here, so they equal the reference's."""
    c = G.STATS_CASE
    p = G.gemm_problem(c["M"], c["N"], c["K"], dtype=F16, alpha=c["alpha"])
    u = G.upload(ctx, p)
    parts = c["N"] // 64
    poison = np.full((c["M"] + G.GUARD_ROWS, parts, 2), np.nan, np.float32)
    stats = ctx.to_device(poison)
    u.out.copy_from(u.sentinel)
    _lib.check(ctx.lib.odise_hip_gemm_ln(ctx.h, C.byref(u.desc), None, 0, 0.0, 0.0, None, None, None, None, stats), "gemm_ln")
    assert (ctx.lib.odise_hip_last_tile() & 255) == 4
    _check_exact(u.out.numpy(), p, "producer output")
    got = stats.numpy()
    ref = R.row_stats(p.out[0]).astype(np.float32)
    assert np.array_equal(got[:c["M"]], ref), f"{int((got[:c['M']] != ref).sum())} of {ref.size} partial statistics differ"
    assert np.isnan(got[c["M"]:]).all(), "statistics rows past M were written"


# ---- convolutions -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ups", [False, True])
@pytest.mark.parametrize("Cout", G.HALO_COUT)
@pytest.mark.parametrize("Cin", G.HALO_CIN)
def test_halo_convolutions(ctx, Cin, Cout, ups):
    """Tiles 7 / 8 / 9 on 2 x 17 x 33 (ragged 16 x 16 patches both ways; with the fused upsample gathered from 9 x 17), one and three 64-channel
    chunks, the three chunks also split 2 + 1; every epilogue.  Tiles 8 and 9 are also compared with each other."""
    n = 0
    for dtype, epi in G.CONV_EPILOGUES:
        p = G.conv_problem(Cin, Cout, ups=ups, dtype=dtype, epi=epi)
        u = G.upload_conv(ctx, p)
        for split in (1, 2) if Cin == 192 else (1,):
            outs = {}
            for tile in G.HALO_TILES:
                outs[tile] = G.run_conv(ctx, p, u, tile, split)
                assert np.array_equal(outs[tile], p.expected), \
                    f"halo tile {tile} split {split} {Cin}->{Cout} ups {ups} {epi}: {int((outs[tile] != p.expected).sum())} of {p.expected.size} buffer elements differ"
                n += 1
            assert np.array_equal(outs[8], outs[9])
    print(f"[gemm] halo {Cin}->{Cout} ups={ups}: {n} launches bit-equal to the reference")


@pytest.mark.parametrize("Cin", G.IGEMM_CIN)
@pytest.mark.parametrize("geom", list(G.IGEMM_GEOMS))
def test_implicit_gemm_convolutions(ctx, geom, Cin):
    """3x3, 3x3 stride 2 with no top / left padding and an explicit output size, 1x1; Cin = 24 / 72 make a 64-deep K-tile straddle taps
    (tap-major), Cin = 64 walks chunk-major; tiles 0, 2, 4, 5 and (where Cin % 64 == 0, its only form) 6."""
    k, stride, pad_tl, out_hw = G.IGEMM_GEOMS[geom]
    n = 0
    for Cout in G.IGEMM_COUT:
        for dtype, epi in G.CONV_EPILOGUES:
            p = G.conv_problem(Cin, Cout, k=k, stride=stride, pad_tl=pad_tl, out_hw=out_hw, dtype=dtype, epi=epi)
            u = G.upload_conv(ctx, p)
            for tile in G.IGEMM_TILES:
                if tile == 6 and Cin % 64:
                    continue
                got = G.run_conv(ctx, p, u, tile)
                assert np.array_equal(got, p.expected), \
                    f"tile {tile} conv {geom} {Cin}->{Cout} {epi}: {int((got != p.expected).sum())} of {p.expected.size} buffer elements differ"
                n += 1
    print(f"[gemm] conv {geom} Cin={Cin}: {n} launches bit-equal to the reference")


# ---- inexact activations ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.ACTIVATIONS) + ["geglu"])
@pytest.mark.parametrize("tile", G.ACT_TILES)
def test_activations_on_exact_pre_activations(ctx, tile, name):
    """SiLU / GELU / QuickGELU / GEGLU of exact pre-activations spread over roughly [-8, 8] (wider at the tails), fp16 and fp32 out, through the
    vector epilogues, the scalar one (an output one element into its buffer) and the reduce kernel's; GEGLU with N % 16 != 0 and ldc = N / 2 + 4.
    The pitch padding and guard rows must keep their sentinel."""
    M, Ns = G.dense_mn(tile)
    geglu = name == "geglu"
    worst = 0.0
    try:
        for K, alpha in G.ACT_K_ALPHA:
            for N in ((Ns[0], 24) if geglu else (Ns[0],)):
                for dtype in (F16, F32):
                    for extra in (dict(), dict(offC=1)):
                        if extra and dtype == F32:
                            continue
                        kw = dict(dtype=dtype, alpha=alpha, geglu=geglu, act=G.ACTIVATIONS.get(name), **extra)
                        if geglu:
                            kw["ldc"] = N // 2 + 4
                        p = G.gemm_problem(M, N, K, **kw)
                        ref, f32 = G.act_reference(p)
                        measured = float(np.abs(f32 - ref).max())
                        bound = G.STEP16 * np.abs(ref) + 4 * measured
                        u = G.upload(ctx, p)
                        image = np.full(p.total_c, G.SENTINEL[dtype], G.BITS[dtype])
                        for flags, split in ((0, 1), (G.BLOCK, 1), (0, 2)):
                            if (flags and tile < 3) or (split > 1 and K < 128):
                                continue
                            ctx.lib.odise_hip_gemm_debug(flags)
                            bits = G.run_gemm(ctx, p, u, tile, split)
                            got = G.out_region(p, bits).astype(np.float64)
                            rest = bits.copy()
                            G._place(rest, image[:1].repeat(got.size).reshape(got.shape), p.ldc, p.strideC, p.offC)
                            assert np.array_equal(rest, image), "the activation epilogue wrote outside its [M, N] region"
                            err = np.abs(got - ref)
                            ratio = float((err / bound).max())
                            worst = max(worst, ratio)
                            print(f"[gemm] {name} tile {tile} K={K} N={N} {'f32' if dtype == F32 else 'f16'} offC={p.offC} flags {flags >> 4} split {split}: "
                                  f"float32 restatement within {measured:.3e} of float64, device error {err.max():.3e}, worst ratio to the bound {ratio:.3f}")
                            assert np.isfinite(got).all() and ratio <= 1.0
    finally:
        ctx.lib.odise_hip_gemm_debug(0)
    assert worst > 0.0
