"""Float64 numpy restatement of GroupNorm (+ residual, activation, accum) and LayerNorm (+ positional table), written from the operations'
definitions (nn.GroupNorm / nn.LayerNorm: biased variance about the mean, two passes), not from csrc/norm.hip; tests/test_norm_reference_cpu.py
holds it to F.group_norm and F.layer_norm in float64.

Both functions return `(ref, cond, stat)` in the convention of tests/glue_reference.py:
  cond   the operation's own fp32 conditioning per element: the sum of the absolute values of the terms entering the last fp32 expression,
         |x * scale| + |shift| + |residual| (scale = gamma * rstd, shift = beta - mean * scale), carried through the activation's slope,
         plus |accum|.  LayerNorm never forms `shift`: its last expression is (x - mean) * rstd * gamma + beta, so beta and mean * scale
         enter on their own, |x * scale| + |mean * scale| + |beta|.  (With |shift| an output where beta cancels the normalised term -
         x = 0, beta = mean * scale to 1e-5 - would be held to 8 * 2^-24 of its own 1e-5 although fp32 rounds beta and the product at 0.3:
         the device's 9e-8 there, at C = 4096, is what any fp32 evaluation gives.)
  stat   the sensitivity of the output to a relative error d in the sums behind the statistics, to first order.
         One pass (GroupNorm: var = E[x^2] - mean^2 from a sum and a sum of squares): an error d of the sum of squares moves var by
         d * E[x^2], hence rstd by rstd * d * E[x^2] / (2 * (var + eps)) and the normalised term y_pre - beta by that fraction of itself; an
         error d of the sum moves the mean by at most d * E|x| and the output by |gamma| * rstd times that:
             stat = |y_pre - beta| * (E[x^2] / (var + eps)) / 2 + |gamma| * rstd * E|x|
         Two passes (LayerNorm: var from the squared deviations): the sum of squared deviations is var itself, so E[x^2] becomes var.
         Like cond it is carried through the activation's slope.
The tests allow n_chain * 2^-24 * stat, n_chain being the longest fp32 summation chain behind a partial sum (gn_chain, ln_chain, conv_chain).

The device is handed eps as a float, so eps is rounded to fp32 and widened here."""
from collections import namedtuple

import numpy as np

from post_reference import f16_round  # noqa: F401  (re-exported for the tests)

NONE, SILU, RELU = 0, 1, 2
U = 2.0 ** -24          # half an fp32 step, relative
STEP16 = 2.0 ** -10     # one fp16 step, relative


def _f64(a):
    return None if a is None else np.asarray(a, np.float64)


def silu(t):
    t = np.asarray(t, np.float64)
    return t / (1.0 + np.exp(-t))


def _activate(t, cond_pre, act):
    """(act(t), |act'(t)|).  ReLU's slope is taken as 1 wherever the fp32 pre-activation may still be positive (t above minus its own bound)."""
    if act == NONE:
        return t, np.ones_like(t)
    if act == RELU:
        return np.maximum(t, 0.0), (t > -8 * U * cond_pre).astype(np.float64)
    if act == SILU:
        s = 1.0 / (1.0 + np.exp(-t))
        return t * s, np.abs(s * (1.0 + t * (1.0 - s)))
    raise ValueError(f"activation {act}")


def group_norm(x, gamma, beta, groups, eps, act, residual=None, accum=None):
    """x [N, HW, C], gamma / beta [C] or None -> act(GN(x) + residual) + accum, cond, stat (all [N, HW, C])."""
    x = _f64(x)
    N, HW, C = x.shape
    assert C % groups == 0
    cpg = C // groups
    eps = np.float64(np.float32(eps))
    g = np.ones(C) if gamma is None else _f64(gamma)
    b = np.zeros(C) if beta is None else _f64(beta)
    xg = x.reshape(N, HW, groups, cpg)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    ex2 = (xg ** 2).mean(axis=(1, 3), keepdims=True)
    eabs = np.abs(xg).mean(axis=(1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    full = lambda v: np.broadcast_to(v, xg.shape).reshape(N, HW, C)   # noqa: E731
    mean, rstd, ratio, eabs = full(mean), full(rstd), full(ex2 / (var + eps)), full(eabs)
    norm = (x - mean) * rstd * g                         # y_pre - beta
    scale = g * rstd
    shift = b - mean * scale
    r = np.zeros_like(x) if residual is None else _f64(residual)
    a = np.zeros_like(x) if accum is None else _f64(accum)
    t = norm + b + r
    cond_pre = np.abs(x * scale) + np.abs(shift) + np.abs(r)
    stat_pre = np.abs(norm) * ratio / 2.0 + np.abs(g) * rstd * eabs
    out, slope = _activate(t, cond_pre, act)
    return out + a, slope * cond_pre + np.abs(a), slope * stat_pre


def layer_norm(x, gamma, beta, eps, table=None, P=None):
    """x [rows, C] -> (y, cond, stat); with a table [P, C] -> ((y, y2), (cond, cond2), stat) where y2 = f16_round(y) + table[row % P]: the
    second output is formed from the ROUNDED first one (csrc/norm.hip, layer_norm_kernel)."""
    x = _f64(x)
    rows, C = x.shape
    eps = np.float64(np.float32(eps))
    g = np.ones(C) if gamma is None else _f64(gamma)
    b = np.zeros(C) if beta is None else _f64(beta)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    norm = (x - mean) * rstd * g
    scale = g * rstd
    y = norm + b
    cond = np.abs(x * scale) + np.abs(mean * scale) + np.abs(b)       # see the module docstring: shift's two terms, not |shift|
    stat = np.abs(norm) * (var / (var + eps)) / 2.0 + np.abs(g) * rstd * np.abs(x).mean(-1, keepdims=True)
    if table is None:
        return y, cond, stat
    t = _f64(table)[np.arange(rows) % P]
    y16 = f16_round(y)
    return (y, y16 + t), (cond, np.abs(y16) + np.abs(t)), stat


# ---- summation chains ------------------------------------------------------------------------------------------------------------------------------
GN_FOLD_IN_APPLY_MAX_CHUNKS = 64    # csrc/norm.hip: up to here gn_apply_kernel folds the chunk partials, beyond it gn_finalize_kernel does
LN_MANY_ROWS, LN_ROWS8 = 2048, 32768
LN_MAX_C = (256, 512, 1024, 2048, 4096)     # kLnChoices

GnChain = namedtuple("GnChain", "n_chain nchunks pix_per_chunk pixel_lanes")


def _ceil_div(a, b):
    return -(-a // b)


def gn_chain(N, HW, C, groups, cu_count, chunk_factor=2):
    """The chunk geometry of odise_hip_group_norm_ex restated: cu_count * chunk_factor / N chunks per image, at least four pixels per pixel
    lane, at most 256.  n_chain: a lane adds its share of a chunk's pixels (sum and sum of squares, fp32), then one thread per group adds the
    pixel lanes' sums of its cpg channels; the fold over chunks is fp64 and does not count."""
    V = C // 8
    VW = min(V, 256)
    PL = 256 // VW
    want = max(1, cu_count * chunk_factor // N)
    maxc = max(1, HW // (4 * PL))
    nchunks = min(want, maxc, 256)
    ppc = _ceil_div(HW, nchunks)
    nchunks = _ceil_div(HW, ppc)
    return GnChain(_ceil_div(ppc, PL) + PL * (C // groups), nchunks, ppc, PL)


def ln_chain(C):
    """A lane adds its vectors' elements, then six butterfly steps."""
    return C // 8 + 6


def conv_chain(H, W, blocks):
    """Rows behind one per-channel partial of a convolution's statistics epilogue, from the row blocks per image it reports: 16 x 16 output
    patches when the count is that of the patch grid, H * W / blocks rows otherwise (the larger when both readings fit)."""
    n = _ceil_div(H * W, blocks)
    if blocks == _ceil_div(H, 16) * _ceil_div(W, 16):
        n = max(n, min(H, 16) * min(W, 16))
    return n


def ln_branch(rows, C, table=False):
    """(index into kLnChoices, row range 0 / 1 / 2) the launcher takes - for the coverage assertions."""
    ci = 0 if table else next(i for i, m in enumerate(LN_MAX_C) if C <= m)
    return ci, (0 if rows < LN_MANY_ROWS else 1 if rows < LN_ROWS8 else 2)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------------------
def step16(ref):
    """One fp16 step at |ref|: 2^-10 |ref| in the normal range, the subnormal spacing 2^-24 below 2^-14."""
    return np.maximum(STEP16 * np.abs(ref), 2.0 ** -24)


def bound16(ref, cond, stat=None, n_chain=0, extra=0.0):
    """|got - ref| <= one fp16 step of |ref| + 8 * 2^-24 cond + n_chain * 2^-24 stat (+ extra: the measured term of an activation through
    expf).  The step is 2^-10 |ref| for every fp16 normal number; a pre-activation that beta cancels to below 2^-14 is rounded to the
    subnormal grid, whose step no longer shrinks with |ref|."""
    s = 0.0 if stat is None else n_chain * U * stat
    return step16(ref) + 8 * U * cond + s + extra


CAP_STEPS, CAP_SHARE = 8, 0.01


def stat_share_over_cap(ref, stat, n_chain):
    """Share of elements whose statistics term exceeds CAP_STEPS fp16 steps of |ref|."""
    return float((n_chain * U * stat > CAP_STEPS * STEP16 * np.abs(ref)).mean())
