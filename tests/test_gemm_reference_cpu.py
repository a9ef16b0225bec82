"""CPU: what tests/test_gpu_gemm_exact.py relies on, shown without a GPU.

1. The exactness precondition of every case of tests/gemm_cases.py: the largest magnitude any intermediate can reach, in units of the power of two
   all intermediates are multiples of, stays below 2^24 - so fp32 holds every one of them exactly, whatever the order of the sums.
2. The convolution reference (tests/gemm_reference.py conv2d_nhwc) against torch.nn.functional.conv2d in float64 at the geometries of the cases:
   stride 2 with top / left padding 0 and an explicit output size, the fused nearest-2x upsample, 1x1, 3x3.  Integer data: equal, not close.
3. The float32 restatement of csrc/common.h's mul_sigmoid / gelu_erf against the float64 formulas on the grids the activation tests use: the
   measured distance that, times 4, is the part of those tests' bound the fp16 step does not explain."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_cases as G
import gemm_reference as R

LIMIT = 2.0 ** 24


def _dense_problem_keys():
    for tile in G.DENSE_TILES:
        M, Ns = G.dense_mn(tile)
        ks = sorted({k for _, kl in G.tile_modes(tile) for k in kl})
        for N in Ns:
            for K in ks:
                for layout in G.LAYOUTS:
                    for kw in G.layout_variants(layout, M, N, K):
                        yield M, N, K, kw
            for K, _ in G.SPLIT_CASES:
                for layout in G.SPLIT_LAYOUTS:
                    for kw in G.split_variants(layout, M, N, K):
                        yield M, N, K, kw


def test_every_dense_case_is_exact_in_fp32():
    """Analytic worst case per (K, epilogue): 9 K alpha scale + the additive terms, over the granularity."""
    seen = set()
    worst_ratio = 0.0
    for M, N, K, kw in _dense_problem_keys():
        key = (K, kw["epi"])
        if key in seen:
            continue
        seen.add(key)
        worst, gran = G.worst_intermediate(K, G.EPILOGUES[kw["epi"]])
        worst_ratio = max(worst_ratio, worst / gran / LIMIT)
        assert worst / gran < LIMIT, (key, worst, gran)
        assert worst < 65504.0, "an fp16 output would overflow"
    print(f"[gemm] {len(seen)} (K, epilogue) classes; the largest intermediate reaches {worst_ratio:.4f} of 2^24 granules")
    assert len(seen) >= 30


@pytest.mark.parametrize("layout", G.LAYOUTS)
def test_generated_problems_keep_their_promises(layout):
    """One tile's worth of real problems per layout: operands are integers in [-3, 3], the terms dyadic, the measured intermediates inside the
    analytic bound, the poison is NaN exactly where no matrix lives, and the expected image carries the sentinel everywhere else."""
    M, Ns = G.dense_mn(2)
    for N in Ns:
        for K in (8, 136, 576):
            for kw in G.layout_variants(layout, M, N, K):
                p = G.gemm_problem(M, N, K, **kw)
                worst, gran = G.worst_intermediate(K, p.epi)
                assert np.abs(p.acc).max() <= 9 * K and np.array_equal(p.acc, np.rint(p.acc))
                y = R.activate(p.x, p.act) + (p.residual.astype(np.float64) if p.residual is not None else 0.0)
                for v in (p.acc * p.alpha, p.x, y):
                    assert np.abs(v).max() <= worst and np.array_equal(v / gran, np.rint(v / gran)), G.describe(p, kw)
                a = p.bufA[np.isfinite(p.bufA)]
                assert np.abs(a).max() <= 3 and np.array_equal(a, np.rint(a))
                n_a = p.batch * M * K if p.strideA else M * K
                n_w = p.batch * N * K if p.strideW else N * K
                finite = np.isfinite(p.bufA).sum() + (np.isfinite(p.bufW).sum() if p.bufW is not None else 0)
                assert finite == n_a + n_w, "NaN everywhere but in the operands"
                assert (p.expected != G.SENTINEL[p.dtype]).sum() <= p.batch * M * N
                assert (p.expected == G.SENTINEL[p.dtype]).sum() >= p.expected.size - p.batch * M * N
                got = G.out_region(p, p.expected)
                assert np.array_equal(got.view(G.BITS[p.dtype]), p.out.view(G.BITS[p.dtype]))
                if p.dtype == G.F32:
                    assert np.array_equal(p.out.astype(np.float64), y), "an fp32 output is the exact value"
                else:
                    assert (np.abs(p.out.astype(np.float64) - y) <= G.STEP16 / 2 * np.abs(y)).all()


def test_producer_statistics_case_is_exact():
    c = G.STATS_CASE
    p = G.gemm_problem(c["M"], c["N"], c["K"], dtype=G.F16, alpha=c["alpha"])
    assert np.abs(p.x).max() <= 64.0, "outputs above 64 would leave the range where the sums of squares stay below 2^24 granules"
    assert np.array_equal(p.out.astype(np.float64), p.x), "multiples of 1/8 below 64 are fp16 values"
    st = R.row_stats(p.out[0])
    assert np.abs(st[..., 0]).max() * 8 < LIMIT and st[..., 1].max() * 64 < LIMIT
    assert np.array_equal(st.astype(np.float32).astype(np.float64), st)


def _torch_conv(p):
    x = torch.from_numpy(p.X.astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(p.Wt.astype(np.float64)).permute(0, 3, 1, 2)
    if p.ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    H, W = x.shape[-2:]
    pb = max((p.OH - 1) * p.stride + p.k - p.pad_tl[0] - H, 0)
    pr = max((p.OW - 1) * p.stride + p.k - p.pad_tl[1] - W, 0)
    x = F.pad(x, (p.pad_tl[1], pr, p.pad_tl[0], pb))
    y = F.conv2d(x, w, stride=p.stride)[:, :, :p.OH, :p.OW]
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("geom", list(G.IGEMM_GEOMS) + ["3x3up"])
@pytest.mark.parametrize("Cin", [24, 64])
def test_conv_reference_against_torch_float64(geom, Cin):
    if geom == "3x3up":
        p = G.conv_problem(Cin, 72, ups=True)
    else:
        k, stride, pad_tl, out_hw = G.IGEMM_GEOMS[geom]
        p = G.conv_problem(Cin, 72, k=k, stride=stride, pad_tl=pad_tl, out_hw=out_hw)
    ref = _torch_conv(p)
    assert ref.shape == p.acc.shape == (p.N, p.OH, p.OW, p.Cout)
    assert np.array_equal(ref, p.acc), f"{geom}: conv2d_nhwc differs from torch on integer data"
    assert np.abs(p.acc).max() > 20, "a degenerate case would prove nothing"


def test_every_conv_case_is_exact_in_fp32():
    n = 0
    for Cin in set(G.HALO_CIN + G.IGEMM_CIN):
        for k in (1, 3):
            for dt, e in G.CONV_EPILOGUES:
                p = G.conv_problem(Cin, 72, k=k, pad_tl=(k // 2, k // 2), dtype=dt, epi=e, hw=(5, 6))
                worst, gran = G.conv_worst_intermediate(p)
                assert worst / gran < LIMIT and worst < 65504.0
                assert np.abs(p.x).max() <= worst and np.array_equal(p.x / gran, np.rint(p.x / gran))
                n += 1
    assert n == 4 * 2 * len(G.CONV_EPILOGUES)


@pytest.mark.parametrize("name", list(G.ACTIVATIONS) + ["geglu"])
def test_float32_restatement_of_the_activations(name):
    """The numpy float32 port of mul_sigmoid / gelu_erf (csrc/common.h) on the exact pre-activations of the GPU test's grids: finite, and its
    distance to the float64 formula is printed - the GPU test multiplies exactly this number by 4."""
    for K, alpha in G.ACT_K_ALPHA:
        M, Ns = G.dense_mn(2)
        N = Ns[0]
        p = G.gemm_problem(M, N, K, alpha=alpha, geglu=name == "geglu", act=G.ACTIVATIONS.get(name))
        ref, f32 = G.act_reference(p)
        d = np.abs(f32 - ref)
        print(f"[gemm] {name} K={K} alpha={alpha}: pre-activations in [{p.x.min():.3f}, {p.x.max():.3f}], float32 restatement within {d.max():.3e} of float64 "
              f"(relative to max |ref| {d.max() / np.abs(ref).max():.3e})")
        assert np.isfinite(f32).all() and p.x.min() < -4 and p.x.max() > 4
        # gelu_erf is Abramowitz & Stegun 7.1.26, |erf error| <= 1.5e-7: the restatement must be that close, or the port is wrong
        assert d.max() <= 2e-6 * max(1.0, np.abs(ref).max())
