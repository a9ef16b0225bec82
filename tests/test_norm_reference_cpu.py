"""CPU: tests/norm_reference.py (float64 numpy) against F.group_norm and F.layer_norm in float64 at every case of tests/norm_ref_cases.py, so
the restatement is shown to BE the operation before any kernel is held to it; and the properties of the crafted inputs that
tests/test_gpu_norm_ref.py relies on, asserted from the reference alone: class A's exact sums (by integer arithmetic), class B's ratio of mean to
deviation, the constant groups' output, the cap on the statistics term of the bound, and how few outputs fall below the fp16 normal range."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC
import norm_ref_cases as K
import norm_reference as R

GN = K.gn_cases() + K.fold_cases(K.NOMINAL_CUS)[0]
LN = K.ln_cases()
TIGHT = 1e-12


def same(got, ref, what):
    err = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f"{what}: max |torch - restatement| / max(1, |ref|) = {err:.3e}")
    assert got.shape == ref.shape and err <= TIGHT, what


def torch_act(t, act):
    return {K.NONE: lambda v: v, K.SILU: F.silu, K.RELU: F.relu}[act](t)


def subnormal_share(ref, cond, what):
    """Outputs below the fp16 normal range whose 8 * 2^-24 * cond is under half a subnormal step: only there does the bound's first term rest on
    the subnormal spacing (norm_reference.step16) and not on 2^-10 |ref|.  They must stay rare."""
    share = float(((cond < 1.0 / 16) & (ref != 0) & (np.abs(ref) < 2.0 ** -14)).mean())
    print(f"{what}: {100 * share:.4f} % of the outputs are held to the subnormal step")
    assert share <= 0.001, what


@pytest.mark.parametrize("c", GN, ids=[c.name for c in GN])
def test_group_norm_restatement_is_torchs(c):
    inputs = K.gn_input(c)
    x, gamma, beta, res, acc = inputs
    ref, cond, stat = K.gn_reference(c, inputs)
    w, b = (None, None) if gamma is None else (torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)))
    t = F.group_norm(torch.from_numpy(x.astype(np.float64)).permute(0, 2, 1), c.G, w, b, eps=float(np.float32(c.eps))).permute(0, 2, 1)
    if res is not None:
        t = t + torch.from_numpy(res.astype(np.float64))
    t = torch_act(t, c.act)
    if acc is not None:
        t = t + torch.from_numpy(acc.astype(np.float64))
    same(t.numpy(), ref, c.name)
    assert (cond >= np.abs(ref) * (1 - 1e-9)).all() if c.act == K.NONE else np.isfinite(cond).all()
    assert np.isfinite(stat).all() and (stat >= 0).all()
    subnormal_share(ref, cond, c.name)
    if c.kind == "const" and not c.res and not c.acc:
        m = K.gn_const_mask(c)
        want = torch_act(torch.from_numpy(np.broadcast_to(beta.astype(np.float64), ref.shape).copy()), c.act).numpy()
        assert np.abs(ref - want)[m].max() <= 1e-12, "a constant group's output is act(beta)"


@pytest.mark.parametrize("c", GN, ids=[c.name for c in GN])
def test_group_norm_statistics_term_is_capped(c):
    inputs = K.gn_input(c)
    ref, _, stat = K.gn_reference(c, inputs)
    n = K.gn_stat_chain(c, K.NOMINAL_CUS)
    share = R.stat_share_over_cap(ref, stat, n) if n else 0.0
    print(f"{c.name}: n_chain {n}, share of elements whose statistics term exceeds {R.CAP_STEPS} fp16 steps: {100 * share:.3f} %")
    assert share <= R.CAP_SHARE
    if c.kind in ("B", "B0"):
        o = K.gn_offset(c)
        x = inputs[0].astype(np.float64).reshape(c.N, c.HW, c.G, -1)
        ratio = np.abs(x.mean((1, 3))) / np.maximum(x.std((1, 3)), 1e-300)
        print(f"{c.name}: offset {o}, mean / deviation {ratio.min():.1f} .. {ratio.max():.1f}")
        if c.HW * (c.C // c.G) >= 64:      # enough values per group for the deviation to be that of the 17 quarter steps (1.2247)
            assert (ratio >= o / 1.2247 * 0.8).all()


def test_class_b_reaches_39_deviations_at_48():
    """The stated ratio of class B: at the offset 48 the mean is about 39 deviations; and some GroupNorm case does run at 48."""
    q = NC.quarters((4096,), salt=5).astype(np.float64)
    assert abs(q.std() - 1.2247) < 0.03 and abs((48 + q).mean() / q.std() - 39.2) < 1.5
    assert any(c.kind in ("B", "B0") and K.gn_offset(c) == 48 for c in GN), "no GroupNorm case keeps the offset 48 under the cap"
    assert any(c.kind == "B" and c.offset == 48 for c in LN), "no LayerNorm case keeps the offset 48 under the cap"
    assert any(c.kind == "B" and K.gn_offset(c) >= 16 and c.res for c in GN)


@pytest.mark.parametrize("c", [c for c in GN if c.kind in ("A", "const")], ids=[c.name for c in GN if c.kind in ("A", "const")])
def test_class_a_sums_are_exact_in_fp32(c):
    """Integer arithmetic: in quarter steps every |x| <= 13 (3.25), so any partial sum of a group is below 13 * elements and any partial sum of
    squares (sixteenth steps) below 169 * elements - both must stay below 2^24, where fp32 holds every integer; and the inputs ARE quarter steps."""
    x = K.gn_input(c)[0].astype(np.float64)
    q = np.rint(x * 4).astype(np.int64)
    assert np.array_equal(q / 4.0, x) and np.abs(q).max() <= 13
    per_group = c.HW * (c.C // c.G)
    g = q.reshape(c.N, c.HW, c.G, -1)
    assert int(np.abs(g).sum((1, 3)).max()) < 2 ** 24 and int((g * g).sum((1, 3)).max()) < 2 ** 24
    assert per_group <= 2 ** 17


def test_gn_chain_restates_the_launcher():
    """Spot values of the chunk geometry worked by hand from odise_hip_group_norm_ex (256 CUs, factor 2)."""
    assert R.gn_chain(1, 8192, 128, 32, 256) == (4 + 16 * 4, 128, 64, 16)            # want 512, maxc 128
    assert R.gn_chain(1, 5, 8, 1, 256) == (1 + 256 * 8, 1, 5, 256)
    assert R.gn_chain(16, 64, 640, 32, 256) == (5 + 3 * 20, 5, 13, 3)                # maxc 64 / 12 = 5 -> ppc 13 -> 5 chunks, ceil(13 / 3) pixels per lane
    assert R.gn_chain(1, 64, 2056, 8, 256) == (4 + 257, 16, 4, 1)
    hw64, hw65, factor = K.fold_pair(256)
    assert factor == 2 and R.gn_chain(1, hw64, K.FOLD_C, K.FOLD_G, 256).nchunks == 64 and R.gn_chain(1, hw65, K.FOLD_C, K.FOLD_G, 256).nchunks == 65
    hw64, hw65, factor = K.fold_pair(8)                                              # a small device needs a denser chunking for 65
    assert factor > 2 and R.gn_chain(1, hw65, K.FOLD_C, K.FOLD_G, 8, factor).nchunks == 65
    assert R.conv_chain(20, 12, 2) == 16 * 12 and R.conv_chain(40, 24, 6) == 256 and R.conv_chain(64, 32, 4) == 512


@pytest.mark.parametrize("c", LN, ids=[c.name for c in LN])
def test_layer_norm_restatement_is_torchs(c):
    inputs = K.ln_input(c)
    x, gamma, beta = inputs
    ref, cond, stat = K.ln_reference(c, inputs)
    w, b = (None, None) if gamma is None else (torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)))
    t = F.layer_norm(torch.from_numpy(x.astype(np.float64)), (c.C,), w, b, eps=float(np.float32(1e-5)))
    same(t.numpy(), ref, c.name)
    subnormal_share(ref, cond, c.name)
    n = K.ln_stat_chain(c)
    share = R.stat_share_over_cap(ref, stat, n) if n else 0.0
    print(f"{c.name}: n_chain {n}, share over the cap {100 * share:.3f} %")
    assert share <= R.CAP_SHARE
    if c.kind == "const":
        want = np.zeros(c.C) if beta is None else beta.astype(np.float64)
        assert np.abs(ref[0] - want).max() <= 1e-12 and np.abs(ref[-1] - want).max() <= 1e-12, "a constant row's output is beta"
    if c.kind == "B" and c.C >= 64:
        xf = x.astype(np.float64)
        assert (np.abs(xf.mean(-1)) / xf.std(-1) >= c.offset / 1.2247 * 0.8).all()


def test_layer_norm_cases_reach_every_launcher_branch():
    """Each kLnChoices entry below and from LN_MANY_ROWS, C just above each limit, the eight-rows kernel (C = 320 from LN_ROWS8) and C = 256 either
    side of LN_ROWS8; the 32 K-row cases stay at C = 320 and C = 256 (the other entries launch the same instantiation from 2048 rows)."""
    reached = {R.ln_branch(c.rows, c.C) for c in LN}
    assert {(i, r) for i in range(5) for r in (0, 1)} <= reached and {(0, 2), (1, 2)} <= reached
    assert all(c.C in (256, 320) for c in LN if c.rows > 30000)
    assert {R.ln_branch(r, C, table=True) for r, C, _ in K.LN_TABLE} == {(0, 0), (0, 1)}
    assert {c.C for c in LN} >= {8, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096}
    assert {c.rows for c in LN} == {1, 3, 2047, 2048, 2051, 32767, 32771}


@pytest.mark.parametrize("rows,C,P", K.LN_TABLE)
def test_layer_norm_table_output_is_formed_from_the_rounded_first(rows, C, P):
    c, x, gamma, beta, table = K.ln_table_input(rows, C, P, "A")
    (y, y2), (cond, cond2), stat = R.layer_norm(x, gamma, beta, 1e-5, table, P)
    t = F.layer_norm(torch.from_numpy(x.astype(np.float64)), (C,), torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)),
                     eps=float(np.float32(1e-5))).numpy()
    same(t, y, f"layer_norm table {rows}x{C}")
    want2 = t.astype(np.float32).astype(np.float16).astype(np.float64) + table.astype(np.float64)[np.arange(rows) % P]
    assert np.abs(want2 - y2).max() <= 2.0 ** -10 * np.abs(y).max() + 1e-12    # torch's y may round to the neighbouring fp16 value
    assert (np.abs(y2 - (y + table[np.arange(rows) % P])) <= 2.0 ** -11 * np.abs(y) + 2.0 ** -25).all(), "y2 is half an fp16 step of y from y + table"
    assert (cond2 >= np.abs(y2) * (1 - 1e-12)).all()
