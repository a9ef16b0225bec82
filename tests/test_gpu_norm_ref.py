"""GPU: the GroupNorm and LayerNorm kernels of csrc/norm.hip, and the GroupNorm that reads a convolution's statistics epilogue, against the
float64 restatement of tests/norm_reference.py (held to torch's own operators by tests/test_norm_reference_cpu.py) on the crafted inputs of
tests/norm_ref_cases.py.

Bound (norm_reference.bound16):   |got - ref| <= one fp16 step of |ref| (2^-10 |ref|) + 8 * 2^-24 * cond + n_chain * 2^-24 * stat
  cond     the operation's own fp32 conditioning, stat the output's sensitivity to a relative error of the sums behind the statistics (both from
           the restatement); n_chain the longest fp32 summation chain behind a partial sum: from gn_chain (the launcher's chunk geometry at this
           device's CU count), C / 8 + 6 for LayerNorm, the rows per statistics block for the convolution path.  The last term is zero for class A
           and constant inputs, whose sums are exact; and it is capped: on at most 1 % of a case's elements may it exceed 8 fp16 steps of |ref|
           (asserted here at the device's geometry; the inputs take a smaller offset where it would, never a larger cap).
  SiLU     goes through expf: its term is measured, never from the kernel - the distance of float32 torch silu to the float64 restatement on the same
           pre-activation (the case's maximum), times 4 - and added.
Every output is allocated with 64 rows (pixels) of a NaN pattern behind it, which must be untouched; the pattern also fills the output itself,
so an element the kernel skips is not finite.  Every check prints the worst error next to its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

import norm_ref_cases as K
import norm_reference as R
from odise_amd import _lib

pytestmark = pytest.mark.gpu

GN = K.gn_cases()
LN = K.ln_cases()
EPS_LN = 1e-5


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------
def report(what, err, bound):
    ratio = err / np.maximum(bound, 1e-300)
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"[norm] {what}: worst err {float(err[i]):.3e} at bound {float(bound[i]):.3e} (ratio {float(ratio[i]):.3f}); max err {float(err.max()):.3e}")
    return float(ratio[i])


def check16(got, ref, cond, what, stat=None, n_chain=0, extra=0.0):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} outputs not finite (not written, or a NaN computed)"
    assert report(what, np.abs(got - ref), R.bound16(ref, cond, stat, n_chain, extra)) <= 1.0, what


def capped(ref, stat, n_chain, what):
    if n_chain:
        share = R.stat_share_over_cap(ref, stat, n_chain)
        print(f"[norm] {what}: n_chain {n_chain}, statistics term over {R.CAP_STEPS} fp16 steps on {100 * share:.3f} % of the elements")
        assert share <= R.CAP_SHARE, what


def silu_term(c, inputs):
    """4 x the distance of float32 torch silu to the float64 restatement on the case's pre-activation (0 for the other activations)."""
    if c.act != K.SILU:
        return 0.0
    x, gamma, beta, res, _ = inputs
    t, _, _ = R.group_norm(x, gamma, beta, c.G, c.eps, K.NONE, res, None)
    measured = float(np.abs(torch.nn.functional.silu(torch.from_numpy(t.astype(np.float32))).numpy().astype(np.float64) - R.silu(t)).max())
    print(f"[norm] {c.name}: fp32-torch silu distance {measured:.3e}")
    return 4 * measured


class Padded:
    """An fp16 output of `rows` x C with K.PAD more rows behind it, all of it the NaN pattern."""

    def __init__(self, ctx, rows, Cc):
        self.rows, self.C = rows, Cc
        self.buf = ctx.to_device(K.nan_pattern((rows + K.PAD, Cc)))

    def result(self, shape, what):
        a = self.buf.numpy()
        tail = a[self.rows:].view(np.uint16)
        assert (tail == K.NAN_BITS).all(), f"{what}: {int((tail != K.NAN_BITS).sum())} elements written past the end of the output"
        return a[:self.rows].reshape(shape)


def dev(ctx, a):
    return None if a is None else ctx.to_device(a)


def run_gn(ctx, c, inputs):
    x, gamma, beta, res, acc = inputs
    out = Padded(ctx, c.N * c.HW, c.C)
    rc = ctx.lib.odise_hip_group_norm_ex(ctx.h, dev(ctx, x), out.buf, dev(ctx, gamma), dev(ctx, beta), c.N, c.HW, c.C, c.G, C.c_float(c.eps), c.act,
                                         dev(ctx, res), dev(ctx, acc))
    _lib.check(rc, "group_norm_ex")
    ctx.sync()
    return out.result((c.N, c.HW, c.C), c.name)


def check_gn(ctx, c, cus, factor=2):
    inputs = K.gn_input(c, cus, factor)
    ref, cond, stat = K.gn_reference(c, inputs)
    n_chain = K.gn_stat_chain(c, cus, factor)
    what = c.name + (f" (offset {K.gn_offset(c, cus, factor)})" if c.kind in ("B", "B0") else "")
    capped(ref, stat, n_chain, what)
    got = run_gn(ctx, c, inputs)
    check16(got, ref, cond, what, stat, n_chain, silu_term(c, inputs))
    return got, ref, inputs


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GN, ids=[c.name for c in GN])
def test_group_norm(ctx, c):
    got, ref, inputs = check_gn(ctx, c, ctx.device_info()[1])
    if c.kind == "const" and not c.res and not c.acc:
        m = K.gn_const_mask(c)
        beta = np.broadcast_to(inputs[2].astype(np.float64), ref.shape)
        want = {K.NONE: beta, K.RELU: np.maximum(beta, 0), K.SILU: R.silu(beta)}[c.act]
        assert np.abs(ref - want)[m].max() <= 1e-12      # ... and `got` was held to ref above: a constant group comes out as act(beta)


def test_group_norm_folds_in_apply_up_to_64_chunks_and_in_finalize_beyond(ctx):
    """HW either side of GN_FOLD_IN_APPLY_MAX_CHUNKS for this device's CU count: 64 chunks (gn_apply_kernel folds the partials) and 65
    (gn_finalize_kernel runs).  A device too small to want 65 chunks gets a denser chunking for the duration of the test."""
    cus = ctx.device_info()[1]
    cases, factor = K.fold_cases(cus)
    reached = {R.gn_chain(c.N, c.HW, c.C, c.G, cus, factor).nchunks for c in cases}
    assert reached == {R.GN_FOLD_IN_APPLY_MAX_CHUNKS, R.GN_FOLD_IN_APPLY_MAX_CHUNKS + 1}, reached
    try:
        if factor != 2:
            ctx.lib.odise_hip_gn_tuning(factor)
        for c in cases:
            check_gn(ctx, c, cus, factor)
    finally:
        ctx.lib.odise_hip_gn_tuning(2)


def test_group_norm_refuses_more_than_256_groups(ctx):
    N, HW, Cc, G = K.GN_REFUSED
    x = ctx.to_device(K.NC.quarters((N, HW, Cc)))
    out = Padded(ctx, N * HW, Cc)
    rc = ctx.lib.odise_hip_group_norm_ex(ctx.h, x, out.buf, None, None, N, HW, Cc, G, C.c_float(1e-5), 0, None, None)
    assert rc == -1, rc      # ODISE_ERR_ARG
    ctx.sync()
    assert (out.buf.numpy().view(np.uint16) == K.NAN_BITS).all(), "a refused call launched something"


def test_group_norm_of_no_images_writes_nothing(ctx):
    x = ctx.to_device(K.NC.quarters((1, 16, 64)))
    out = Padded(ctx, 16, 64)
    rc = ctx.lib.odise_hip_group_norm_ex(ctx.h, x, out.buf, None, None, 0, 16, 64, 32, C.c_float(1e-5), 1, None, None)
    assert rc == 0, rc
    ctx.sync()
    assert (out.buf.numpy().view(np.uint16) == K.NAN_BITS).all()


# ---- the statistics epilogue of the convolutions -> gn_finalize_cols_kernel -----------------------------------------------------------------------
@pytest.mark.parametrize("c", K.CONV_CASES, ids=[c.name for c in K.CONV_CASES])
def test_group_norm_from_conv_statistics(ctx, c):
    """The reference is the GroupNorm of the fp16 tensor the convolution actually wrote; n_chain = the rows behind one per-channel partial of
    the epilogue.  The conv's outputs are not exact sums: the statistics term applies."""
    x, w, gamma, beta, bias = K.conv_input(c)
    y, yn, blocks = ctx.conv2d_gn(ctx.to_device(x), ctx.to_device(w), ctx.to_device(gamma), ctx.to_device(beta), bias=ctx.to_device(bias), groups=c.G,
                                  eps=c.eps, act=c.act, force_tile=c.tile, force_split=1)
    assert blocks > 0, f"{c.name}: the convolution left no statistics (gn_finalize_cols_kernel did not run)"
    y16 = y.numpy().reshape(c.N, c.H * c.W, c.Cout)
    assert np.isfinite(y16).all()
    g = y16.astype(np.float64).reshape(c.N, c.H * c.W, c.G, -1)
    ratio = np.abs(g.mean((1, 3))) / g.std((1, 3))
    print(f"[norm] {c.name}: {blocks} row blocks, mean / deviation of the groups {ratio.min():.2f} .. {ratio.max():.2f}")
    n_chain = R.conv_chain(c.H, c.W, blocks)
    ref, cond, stat = R.group_norm(y16, gamma, beta, c.G, c.eps, c.act)
    what = f"{c.name} ({blocks} row blocks, n_chain {n_chain})"
    capped(ref, stat, n_chain, what)
    gc = K.GnCase(c.name, c.N, c.H * c.W, c.Cout, c.G, "conv", 0, c.act, False, False, c.eps)
    check16(yn.numpy().reshape(ref.shape), ref, cond, what, stat, n_chain, silu_term(gc, (y16, gamma, beta, None, None)))


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LN, ids=[c.name for c in LN])
def test_layer_norm(ctx, c):
    inputs = K.ln_input(c)
    x, gamma, beta = inputs
    ref, cond, stat = K.ln_reference(c, inputs)
    n_chain = K.ln_stat_chain(c)
    capped(ref, stat, n_chain, c.name)
    out = Padded(ctx, c.rows, c.C)
    _lib.check(ctx.lib.odise_hip_layer_norm(ctx.h, dev(ctx, x), out.buf, dev(ctx, gamma), dev(ctx, beta), c.rows, c.C, C.c_float(EPS_LN)), "layer_norm")
    ctx.sync()
    check16(out.result((c.rows, c.C), c.name), ref, cond, c.name, stat, n_chain)


@pytest.mark.parametrize("kind", ["A", "B", "const"])
@pytest.mark.parametrize("rows,Cc,P", K.LN_TABLE)
def test_layer_norm_with_table(ctx, rows, Cc, P, kind):
    """y against the restatement; y2 against it too (its bound: y's own, one fp16 step of y2 and the fp32 sum's conditioning), and - the rule
    csrc/norm.hip documents - y2 is formed from the ROUNDED y: it is the device's own y + table, rounded once (half an fp16 step, the fp32 sum's
    rounding may tip it: 2 * 2^-24 * cond)."""
    c, x, gamma, beta, table = K.ln_table_input(rows, Cc, P, kind)
    (ref, ref2), (cond, cond2), stat = R.layer_norm(x, gamma, beta, EPS_LN, table, P)
    n_chain = K.ln_stat_chain(c)
    what = f"layer_norm_table {c.name} P={P}"
    capped(ref, stat, n_chain, what)
    o1, o2 = Padded(ctx, rows, Cc), Padded(ctx, rows, Cc)
    _lib.check(ctx.lib.odise_hip_layer_norm_table(ctx.h, dev(ctx, x), o1.buf, dev(ctx, gamma), dev(ctx, beta), rows, Cc, C.c_float(EPS_LN), o2.buf,
                                                  dev(ctx, table), P), "layer_norm_table")
    ctx.sync()
    y, y2 = o1.result((rows, Cc), what + " y"), o2.result((rows, Cc), what + " y2")
    check16(y, ref, cond, what + " y", stat, n_chain)
    by = R.bound16(ref, cond, stat, n_chain)
    got2 = y2.astype(np.float64)
    assert np.isfinite(got2).all()
    assert report(what + " y2", np.abs(got2 - ref2), by + R.step16(ref2) + 8 * R.U * cond2) <= 1.0
    t = table.astype(np.float64)[np.arange(rows) % P]
    own = y.astype(np.float64) + t
    assert report(what + " y2 from the rounded y", np.abs(got2 - own), R.step16(own) / 2 + 2 * R.U * (np.abs(y.astype(np.float64)) + np.abs(t))) <= 1.0


def test_layer_norm_of_no_rows_writes_nothing(ctx):
    x = ctx.to_device(K.NC.quarters((4, 64)))
    tab = ctx.to_device(K.NC.table(2, 64))
    o1, o2 = Padded(ctx, 4, 64), Padded(ctx, 4, 64)
    assert ctx.lib.odise_hip_layer_norm(ctx.h, x, o1.buf, None, None, 0, 64, C.c_float(EPS_LN)) == 0
    assert ctx.lib.odise_hip_layer_norm_table(ctx.h, x, o1.buf, None, None, 0, 64, C.c_float(EPS_LN), o2.buf, tab, 2) == 0
    ctx.sync()
    assert (o1.buf.numpy().view(np.uint16) == K.NAN_BITS).all() and (o2.buf.numpy().view(np.uint16) == K.NAN_BITS).all()
