"""Cases and inputs of tests/test_gpu_norm_ref.py and tests/test_norm_reference_cpu.py: GroupNorm and LayerNorm (csrc/norm.hip) against the
float64 restatement of tests/norm_reference.py.  Every input comes from the integer mix of tests/norm_cases.py (no RNG): the same bytes on
the CPU and on the device.

Input classes
  A         multiples of 1/4 with |x| <= 2 (norm_cases.quarters): at most 2^17 elements per group, so every fp32 partial sum (< 2^20 quarter
            steps) and sum of squares (< 2^23 sixteenth steps) is exact, whatever the chunking.  No statistics term in the bound.
  B         offset + quarters, exact in fp16 up to 48 + 2 (steps of 1/32 from 32): the mean is offset / 1.22 deviations (39 at 48), which is
            what makes E[x^2] - mean^2 cancel.  The offset of a case is the largest of OFFSETS at which the statistics term of the bound stays
            under the cap (norm_reference.stat_share_over_cap <= CAP_SHARE) for the case's own summation chain: a longer chain, or outputs
            that beta, the residual or accum bring close to zero, take a smaller offset - never a larger cap.  It is found from the float64
            reference alone (gn_offset, ln_offset), for GroupNorm at the chunk geometry of the device the test runs on.
  B0        class B with gamma = beta = NULL.
  massive   class A with one channel of one group per image at 60 + quarters (the VAE's / UNet's massive channels).
  const     class A with one whole group of image 0 (GroupNorm) or the first and last row (LayerNorm) equal to 3.25: variance exactly 0, the
            output is act(beta) (+ residual, accum).  Sums stay exact: no statistics term.
gamma in [0.25, 1.75] (eighths), beta in [-9/32, 11/32] (odd multiples of 1/32; gamma_beta below); residual and accum are class A tensors of other salts."""
import functools
from collections import namedtuple

import numpy as np

import norm_cases as NC
import norm_reference as R

NONE, SILU, RELU = R.NONE, R.SILU, R.RELU
ACTS = (NONE, SILU, RELU)
ACT_NAME = {NONE: "none", SILU: "silu", RELU: "relu"}
CONST = 3.25
MASSIVE = 60.0
NOMINAL_CUS = 256      # MI355X; the CPU test checks the cap at this geometry, the GPU test at the device's own
PAD = 64               # rows (LayerNorm) / pixels (GroupNorm) of NaN pattern behind every output
NAN_BITS = 0x7FA5      # an fp16 NaN no kernel writes

GnCase = namedtuple("GnCase", "name N HW C G kind offset act res acc eps")
LnCase = namedtuple("LnCase", "name rows C kind offset affine")
ConvCase = namedtuple("ConvCase", "name N H W Cin Cout G bias_add tile eps act")


def _salt(*v):
    s = 17
    for k in v:
        s = (s * 1000003 + int(k)) & 0x3FFFFFFF
    return s


def gamma_beta(C):
    """norm_cases.gamma_beta with beta moved by 1/32 (odd multiples of 1/32 in [-9/32, 11/32]): gamma is in eighths, so a group of two values
    (normalised to +-1) or a constant one can no longer meet beta = -+gamma exactly - a pre-activation that cancels to ~1e-6 would be held to
    a relative bound no fp32 evaluation of beta - mean * scale can meet."""
    g, b = NC.gamma_beta(C)
    return g, (b + np.float32(1.0 / 32)).astype(np.float32)


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------
# (N, HW, C, G) -> what it reaches in csrc/norm.hip
GN_SHAPES = [
    (1, 5, 8, 1),           # C = 8: one vector, 256 pixel lanes, HW < pixel lanes, one group of eight channels
    (2, 1, 64, 32),         # HW = 1, two channels per group, two images
    (1, 100, 96, 32),       # cpg = 3 (odd), 21 pixel lanes (256 / 12: four idle threads), ragged four-vector sweep
    (1, 37, 24, 8),         # groups other than 32, odd HW, 85 pixel lanes
    (1, 64, 2056, 8),       # C > 2048: V = 257 > 256, the ragged v += VW sweep (VW < V), cpg = 257 (odd)
    (1, 16, 4096, 256),     # GN_MAX_C, 256 groups (nsub = 1 in the fold), cpg = 16
    (3, 257, 320, 32),      # three images, 6 pixel lanes (256 / 40: 16 idle threads), several chunks with a ragged last one
]
GN_REFUSED = (1, 64, 2056, 257)    # G > 256
FOLD_C, FOLD_G = 512, 32           # the 64 / 65 chunk pair: HW from fold_pair()


OFFSETS = (48, 16, 8, 4, 2, 1)


@functools.lru_cache(maxsize=None)
def gn_offset(c, cus=NOMINAL_CUS, factor=2):
    """Class B's offset for case `c` on a device of `cus` compute units: the largest of OFFSETS whose statistics term is under the cap."""
    n = R.gn_chain(c.N, c.HW, c.C, c.G, cus, factor).n_chain
    for o in OFFSETS:
        ref, _, stat = gn_reference(c, gn_input(c, offset=o))
        if R.stat_share_over_cap(ref, stat, n) <= R.CAP_SHARE:
            return o
    raise AssertionError(f"{c.name}: no offset keeps the statistics term under the cap")


def _gn(N, HW, C, G, kind, act=NONE, res=False, acc=False, eps=1e-5, offset=None):
    name = f"gn_{N}x{HW}x{C}_g{G}_{kind}{offset or ''}_{ACT_NAME[act]}" + ("_res" if res else "") + ("_acc" if acc else "") + \
           ("" if eps == 1e-5 else "_eps1e-6")
    return GnCase(name, N, HW, C, G, kind, offset, act, res, acc, eps)


def gn_cases():
    out = []
    for i, s in enumerate(GN_SHAPES):
        out.append(_gn(*s, "A", act=ACTS[i % 3]))
        out.append(_gn(*s, "B", act=ACTS[(i + 1) % 3], eps=1e-6 if i % 2 else 1e-5))
        out.append(_gn(*s, "const", act=ACTS[(i + 2) % 3]))
    for s in [(1, 100, 96, 32), (3, 257, 320, 32), (1, 64, 2056, 8)]:
        out.append(_gn(*s, "massive", act=SILU, eps=1e-6))
    for s in [(1, 16, 4096, 256), (2, 1, 64, 32), (1, 37, 24, 8)]:      # gamma = beta = NULL: no beta to cancel the normalised term, the offset stays large
        out.append(_gn(*s, "B0", act=NONE))
    # every activation at every residual / accum setting: class A at the odd shape, class B at the multi-chunk one
    for s, kind in [((1, 37, 24, 8), "A"), ((3, 257, 320, 32), "B")]:
        for act in ACTS:
            for res in (False, True):
                for acc in (False, True):
                    c = _gn(*s, kind, act=act, res=res, acc=acc)
                    if c not in out:
                        out.append(c)
    return out


def gn_input(c, cus=NOMINAL_CUS, factor=2, offset=None):
    """(x, gamma, beta, residual or None, accum or None) as the device gets them (fp16 / fp32).  A class B case without an offset of its own
    takes gn_offset's for the device's geometry."""
    if c.kind in ("B", "B0") and offset is None:
        offset = c.offset if c.offset else gn_offset(c, cus, factor)
    shape = (c.N, c.HW, c.C)
    x = NC.quarters(shape, salt=_salt(c.N, c.HW, c.C, c.G)).astype(np.float32)
    cpg = c.C // c.G
    if c.kind in ("B", "B0"):
        x = x + np.float32(offset)
    elif c.kind == "massive":
        for n in range(c.N):
            ch = ((c.G // 2 + n) % c.G) * cpg + (n % cpg)
            x[n, :, ch] += np.float32(MASSIVE)
    elif c.kind == "const":
        g0 = c.G // 3
        x[0, :, g0 * cpg:(g0 + 1) * cpg] = CONST
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(np.float32), x), "the input must be exact in fp16"
    gamma, beta = gamma_beta(c.C) if c.kind != "B0" else (None, None)
    res = NC.quarters(shape, salt=_salt(c.N, c.HW, c.C, 1) + (1 << 20)) if c.res else None
    acc = NC.quarters(shape, salt=_salt(c.N, c.HW, c.C, 2) + (1 << 21)) if c.acc else None
    return x16, gamma, beta, res, acc


def gn_const_mask(c):
    """Elements of a "const" case whose group is constant."""
    m = np.zeros((c.N, c.HW, c.C), bool)
    cpg = c.C // c.G
    g0 = c.G // 3
    m[0, :, g0 * cpg:(g0 + 1) * cpg] = True
    return m


def gn_reference(c, inputs=None):
    x, gamma, beta, res, acc = inputs if inputs is not None else gn_input(c)
    return R.group_norm(x, gamma, beta, c.G, c.eps, c.act, res, acc)


def gn_stat_chain(c, cus, factor=2):
    """n_chain of the statistics term: 0 where every partial is exact."""
    return R.gn_chain(c.N, c.HW, c.C, c.G, cus, factor).n_chain if c.kind in ("B", "B0", "massive") else 0


def fold_pair(cus, N=1, C=FOLD_C, G=FOLD_G):
    """(HW reaching 64 chunks, HW reaching 65 chunks, chunk factor): the smallest sizes either side of GN_FOLD_IN_APPLY_MAX_CHUNKS on a device
    of `cus` compute units; the factor is 2 (the library's) unless the device is too small to ask for 65 chunks with it."""
    factor = 2
    while cus * factor // N < R.GN_FOLD_IN_APPLY_MAX_CHUNKS + 1:
        factor *= 2
    hw = {}
    for HW in range(1, 1 << 14):
        n = R.gn_chain(N, HW, C, G, cus, factor).nchunks
        if n in (64, 65) and n not in hw:
            hw[n] = HW
        if len(hw) == 2:
            return hw[64], hw[65], factor
    raise AssertionError("no HW reaches 64 and 65 chunks")


def fold_cases(cus):
    hw64, hw65, factor = fold_pair(cus)
    out = []
    for HW in (hw64, hw65):
        out.append(_gn(1, HW, FOLD_C, FOLD_G, "A", act=SILU))
        out.append(_gn(1, HW, FOLD_C, FOLD_G, "B", act=NONE))
    return out, factor


# ---- convolution with the statistics epilogue -----------------------------------------------------------------------------------------------------
CONV_CASES = [
    ConvCase("conv_gn_1x20x12x64x96_cpg3", 1, 20, 12, 64, 96, 32, 0.0, 8, 1e-5, SILU),       # cpg = 3: the odd branch of gn_finalize_cols_kernel
    ConvCase("conv_gn_1x40x24x128x128_bias8", 1, 40, 24, 128, 128, 32, 8.0, 8, 1e-6, NONE),  # cpg = 4: the float4 branch; mean of 8 on every channel
]


def conv_input(c):
    x = NC.quarters((c.N, c.H, c.W, c.Cin), salt=_salt(c.H, c.W, c.Cin))
    w = NC.weights((c.Cout, 3, 3, c.Cin), salt=_salt(c.Cout, c.Cin))
    gamma, beta = gamma_beta(c.Cout)
    bias = ((NC._ramp(c.Cout, 7919, 1, 9) - 4) / 8.0 + c.bias_add).astype(np.float32)
    return x, w, gamma, beta, bias


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------------
# C -> row counts.  32767 / 32771 (either side of LN_ROWS8) at C = 320 and C = 256 only; every other C at small row counts and one >= 2048
LN_ROWS = {
    8: (1, 3, 2051),
    256: (1, 3, 2047, 2048, 32767, 32771),
    264: (1, 3, 2048),
    320: (3, 2047, 32767, 32771),
    512: (3, 2047, 2051),
    520: (1, 3, 2048),
    1024: (3, 2047, 2051),
    1032: (1, 3, 2048),
    2048: (3, 2047, 2051),
    2056: (1, 3, 2048),
    4096: (1, 3, 2047, 2051),
}
LN_TABLE = [(33, 128, 1), (5, 8, 9), (2051, 256, 7)]      # (rows, C, P)


LN_PROXY_ROWS = 512


@functools.lru_cache(maxsize=None)
def ln_offset(rows, C, affine):
    """Class B's offset for a LayerNorm case: the largest of OFFSETS whose statistics term is under the cap.  Two passes: the variance does
    not cancel; what the chain costs is the mean's error, |gamma| * rstd * E|x| per unit of d, against outputs that come close to zero where
    x is close to the row's mean or beta cancels the normalised term.  Chosen on the first LN_PROXY_ROWS rows (the rows are alike) at 0.8 of
    the cap's share; the CPU test asserts the cap itself on the whole case."""
    n = R.ln_chain(C)
    for o in OFFSETS:
        c = LnCase("", min(rows, LN_PROXY_ROWS), C, "B", o, affine)
        x, gamma, beta = ln_input(c)
        ref, _, stat = R.layer_norm(x, gamma, beta, 1e-5)
        if R.stat_share_over_cap(ref, stat, n) <= 0.8 * R.CAP_SHARE:
            return o
    raise AssertionError(f"ln {rows}x{C}: no offset keeps the statistics term under the cap")


def _ln(rows, C, kind, affine=True):
    offset = ln_offset(rows, C, affine) if kind == "B" else 0
    name = f"ln_{rows}x{C}_{kind}{offset if kind == 'B' else ''}" + ("" if affine else "_noaffine")
    return LnCase(name, rows, C, kind, offset, affine)


def ln_cases():
    out = []
    for C, rows_list in LN_ROWS.items():
        for i, rows in enumerate(rows_list):
            big = rows > 30000
            out.append(_ln(rows, C, "A", affine=not (i == 1)))         # the second row count of every C without gamma / beta
            if not big or C == 320:
                out.append(_ln(rows, C, "B", affine=not (i == 2)))
            if rows <= 3 or rows == 2051:
                out.append(_ln(rows, C, "const"))
    return out


def ln_input(c):
    x = NC.quarters((c.rows, c.C), salt=_salt(c.rows, c.C, 7)).astype(np.float32)
    x[:, :max(1, c.C // 8)] += np.float32(1.0)     # the row mean moves 1/8 off the quarter grid, so no x sits on it: an output of (nearly) 0 has no fp16 step to be held to
    if c.kind == "B":
        x = x + np.float32(c.offset)
    elif c.kind == "const":
        x[0] = CONST
        x[-1] = CONST
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(np.float32), x)
    gamma, beta = gamma_beta(c.C) if c.affine else (None, None)
    return x16, gamma, beta


def ln_reference(c, inputs=None):
    x, gamma, beta = inputs if inputs is not None else ln_input(c)
    return R.layer_norm(x, gamma, beta, 1e-5)


def ln_stat_chain(c):
    return R.ln_chain(c.C) if c.kind == "B" else 0


def ln_table_input(rows, C, P, kind):
    c = _ln(rows, C, kind)
    x, gamma, beta = ln_input(c)
    return c, x, gamma, beta, NC.table(P, C)


def nan_pattern(shape):
    return np.full(shape, NAN_BITS, np.uint16).view(np.float16)
