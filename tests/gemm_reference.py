"""Exact numpy restatement of odise_hip_gemm / odise_hip_conv2d (include/odise_hip.h) for the crafted inputs of tests/gemm_cases.py.

Operands are small integers and every epilogue term is dyadic, so the float64 arithmetic below is exact (the products are summed by BLAS in
float64: integers far below 2^53 in any order), and so is the device's fp32 arithmetic in whatever order it sums (tests/test_gemm_reference_cpu.py
asserts the precondition per case).  The result is rounded ONCE to the output type, which is what the device does with its exact fp32 value.

    x = alpha * scale_m[m] * sum_k A[m, k] W[n, k] + bias_n[n] + bias_m[m] + rowgroup_add[m // rows_per_group, n]
    C = act(x) + residual            |   geglu: C[m, j] = x[m, 2 j] * gelu(x[m, 2 j + 1])

`pre_activation` returns x; the inexact activations (SiLU, GELU, QuickGELU, GEGLU) are applied to it in float64 by `activate` / `geglu`, and in
float32 the way csrc/common.h spells them by `mul_sigmoid_f32` / `gelu_erf_f32` (the measured part of those tests' tolerance)."""
import math

import numpy as np

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GELU, ACT_QUICKGELU = 0, 1, 2, 3, 4

_erf = np.vectorize(math.erf, otypes=[np.float64])


def matmul_nt(A, W):
    """[..., M, K] x [..., N, K]^T in float64 (exact for the integer operands of the cases); a 2-D operand is shared by the batch."""
    return np.matmul(np.asarray(A, np.float64), np.swapaxes(np.asarray(W, np.float64), -1, -2))


def pre_activation(acc, *, alpha=1.0, scale_m=None, bias_n=None, bias_m=None, rowgroup_add=None, rows_per_group=1):
    """The epilogue up to the activation, float64, on acc [..., M, N]."""
    x = np.asarray(acc, np.float64) * float(alpha)
    M = x.shape[-2]
    if scale_m is not None:
        x = x * np.asarray(scale_m, np.float64)[:, None]
    if bias_n is not None:
        x = x + np.asarray(bias_n, np.float64)[None, :]
    if bias_m is not None:
        x = x + np.asarray(bias_m, np.float64)[:, None]
    if rowgroup_add is not None:
        x = x + np.asarray(rowgroup_add, np.float64)[np.arange(M) // int(rows_per_group)]
    return x


def activate(x, act):
    x = np.asarray(x, np.float64)
    if act == ACT_NONE:
        return x
    if act == ACT_RELU:
        return np.maximum(x, 0.0)
    if act == ACT_SILU:
        return x / (1.0 + np.exp(-x))
    if act == ACT_QUICKGELU:
        return x / (1.0 + np.exp(-1.702 * x))
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    raise ValueError(act)


def geglu(x):
    """Interleaved (a, gate) columns -> a * gelu(gate), half as many columns."""
    return x[..., 0::2] * activate(x[..., 1::2], ACT_GELU)


def finish(x, act, residual, dtype):
    """act (exact ones only: none / ReLU) + residual, rounded once to the output type."""
    assert act in (ACT_NONE, ACT_RELU)
    y = activate(x, act)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y.astype(dtype)


def row_stats(c16, part=64):
    """The producer statistics of odise_hip_gemm_ln: [M][N / part][2] (sum, sum of squares) of the rounded outputs, per `part` columns."""
    M, N = c16.shape
    b = np.asarray(c16, np.float64).reshape(M, N // part, part)
    return np.stack([b.sum(-1), (b * b).sum(-1)], -1)


def conv2d_nhwc(X, Wt, *, stride=1, pad_tl=(1, 1), out_hw, upsample2x=False):
    """X [N, H, W, Cin], Wt [Cout, KH, KW, Cin] -> float64 [N, OH, OW, Cout]; zero padding wherever a tap leaves the (upsampled) input, at
    the top / left by pad_tl and at the bottom / right by whatever out_hw asks for."""
    X = np.asarray(X, np.float64)
    Wt = np.asarray(Wt, np.float64)
    if upsample2x:
        X = X.repeat(2, axis=1).repeat(2, axis=2)
    N, H, W, Cin = X.shape
    Cout, KH, KW, _ = Wt.shape
    OH, OW = out_hw
    pt, pl = pad_tl
    Hp, Wp = max((OH - 1) * stride + KH, pt + H), max((OW - 1) * stride + KW, pl + W)
    Xp = np.zeros((N, Hp, Wp, Cin))
    Xp[:, pt:pt + H, pl:pl + W] = X
    out = np.zeros((N, OH, OW, Cout))
    for ky in range(KH):
        for kx in range(KW):
            win = Xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]
            out += win @ Wt[:, ky, kx].T
    return out


# ---- csrc/common.h in float32 numpy: the same operations in the same order, with numpy's exp and a true division where the device has
# ---- its fast exp / reciprocal
def mul_sigmoid_f32(x, kx):
    x, kx = np.asarray(x, np.float32), np.asarray(kx, np.float32)
    return x * (np.float32(1.0) / (np.float32(1.0) + np.exp(-kx)))


def gelu_erf_f32(v):
    f = np.float32
    v = np.asarray(v, f)
    x = v * f(0.70710678118654752)
    a = np.abs(x)
    t = f(1.0) / (f(1.0) + f(0.3275911) * a)
    p = t * (f(0.254829592) + t * (f(-0.284496736) + t * (f(1.421413741) + t * (f(-1.453152027) + t * f(1.061405429)))))
    r = f(1.0) - p * np.exp(-a * a)
    return f(0.5) * v * (f(1.0) + np.copysign(r, x))


def activate_f32(x, act):
    x = np.asarray(x, np.float32)
    if act == ACT_SILU:
        return mul_sigmoid_f32(x, x)
    if act == ACT_QUICKGELU:
        return mul_sigmoid_f32(x, np.float32(1.702) * x)
    if act == ACT_GELU:
        return gelu_erf_f32(x)
    raise ValueError(act)


def geglu_f32(x):
    x = np.asarray(x, np.float32)
    return x[..., 0::2] * gelu_erf_f32(x[..., 1::2])
