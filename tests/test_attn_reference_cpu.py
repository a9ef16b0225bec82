"""CPU: tests/attn_reference.py attention_f64 against torch's own attention at every shape of tests/attn_cases.py, and the conditions that make
those cases mean something - so that tests/test_gpu_attention_ref.py cannot pass vacuously: the peaked rows are peaked on the intended key, the
hot keys reach every position they are meant to, the wide rows do drive P below the fp16 normal range, the bound is finite and small where a wrong
key would be an error of order 1, the table names every kernel instance and split count, and the strided layouts address what they mean.

On the shapes with 256 (head, image) pairs the comparisons against torch and the Gaussian / wide / flat conditions take the fixed quarter of the
pairs that the GPU test's reference takes (Case.pairs); the peaked family is checked on all."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attn_cases as A
from attn_reference import attention_f64

U32 = 2.0 ** -24


def _reduced(case, arrays, mask):
    """The case restricted to the heads of Case.pairs (those are the same heads in every image): (H', arrays')."""
    p = case.pairs("G")
    if p is None:
        return case.H, arrays
    heads = np.nonzero(p[0])[0]
    assert (p == p[0]).all()
    cols = (heads[:, None] * case.D + np.arange(case.D)[None, :]).reshape(-1)
    return len(heads), [x[:, :, cols] for x in arrays]


@pytest.mark.parametrize("cid", list(A.BY_ID))
def test_attention_f64_against_torch(cid):
    """torch.softmax(q k^T scale + mask) @ v in float64 to 1e-12, and F.scaled_dot_product_attention in float32 within float32's own rounding:
    |sdpa - ref| <= 2^-24 (2 D smax + Lk + 16) cond, with smax = max_k sum_d |q_d k_d| scale (a relative error of D 2^-24 on a score is that much on
    its probability, twice for the normalisation), Lk for the two sums over the keys and cond = sum_k p_k |v_k|.  Rows without a visible key are 0."""
    case = A.BY_ID[cid]
    mask = A.mask_rows(case) if case.masked else None
    for fam in ("G", "P0"):
        H, (Q, K, V) = _reduced(case, list(A.inputs(case, fam)), mask)
        ref, bound = attention_f64(Q, K, V, H, case.scale, mask)
        assert np.isfinite(ref).all() and np.isfinite(bound).all()
        B, Lq, Lk, D = case.B, case.Lq, case.Lk, case.D
        for b in range(B):
            q, k, v = (torch.from_numpy(x[b].astype(np.float64)).view(-1, H, D).transpose(0, 1) for x in (Q, K, V))   # [H, L, D]
            s = q @ k.transpose(-1, -2) * case.scale
            hidden = None
            if mask is not None:
                hidden = torch.from_numpy(mask[b] != 0)
                s = s.masked_fill(hidden[None], float("-inf"))
            p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
            t64 = (p @ v).transpose(0, 1).reshape(Lq, H * D).numpy()
            assert np.abs(t64 - ref[b]).max() <= 1e-12 * max(1.0, np.abs(ref[b]).max()), (cid, fam, b)
            cond = (p @ v.abs()).transpose(0, 1).reshape(Lq, H * D).numpy()
            smax = (q.abs() @ k.abs().transpose(-1, -2) * case.scale).amax(-1)                                          # [H, Lq]
            smax = np.repeat(smax.transpose(0, 1).numpy(), D, axis=1)                                                   # [Lq, H*D]
            live = np.ones(Lq, bool) if hidden is None else ~hidden.all(1).numpy()
            am = None if hidden is None else (~hidden)[None, live]
            sd = F.scaled_dot_product_attention(q[:, live].float()[None], k.float()[None], v.float()[None], attn_mask=am, scale=case.scale)[0]
            sd = sd.transpose(0, 1).reshape(int(live.sum()), H * D).double().numpy()
            tol = U32 * (2 * D * smax[live] + Lk + 16) * cond[live] + 1e-300
            worst = float((np.abs(sd - ref[b][live]) / tol).max())
            assert worst <= 1.0, (cid, fam, b, worst)
            if hidden is not None:
                dead = hidden.all(1).numpy()
                assert dead.any() and (ref[b][dead] == 0).all() and (bound[b][dead] == 0).all(), (cid, fam)


@pytest.mark.parametrize("cid", list(A.BY_ID))
def test_cases_are_not_vacuous(cid):
    case = A.BY_ID[cid]
    mask = A.mask_rows(case) if case.masked else None
    for fam, masked in sorted({(f, m) for f, m, _ in case.runs()}):
        Q, K, V = A.inputs(case, fam)
        for x in (Q, K, V):
            assert x.dtype == np.float16 and np.isfinite(x).all()
        m = mask if masked else None
        ref, bound, st = attention_f64(Q, K, V, case.H, case.scale, m, pairs=case.pairs(fam), stats=True)
        done = np.ones((case.B, case.H), bool) if case.pairs(fam) is None else case.pairs(fam)
        cols = np.repeat(done, case.D, axis=1)[:, None, :]                              # [B, 1, H*D]
        sel = np.broadcast_to(cols, ref.shape)
        assert np.isfinite(ref[sel]).all() and np.isfinite(bound[sel]).all() and (bound[sel] >= 0).all(), (cid, fam)
        # the bound is positive wherever anything can differ: a row that sees a key with a non-zero value in that channel.  (The other elements -
        # rows with no visible key, the flat family's all-zero value columns - have bound 0: the device must give 0 to the bit there.)
        seen = (np.ones((case.B, case.Lq, case.Lk)) if m is None else (m == 0).astype(np.float64)) @ np.abs(V.astype(np.float64))
        assert ((bound > 0) == (seen > 0))[sel].all(), (cid, fam)
        assert st["smax"][done].max() <= 40.0, (cid, fam, st["smax"].max())             # the range the fp32 allowance of the bound is stated for
        if fam.startswith("P"):
            want = A.expected_keys(case, fam, m)
            on = want >= 0
            if m is None:
                assert on.all()
            else:
                assert on.mean() >= 0.5                                                 # first-only, last-only, all and the split patterns hide both keys
            assert (st["top_k"][on] == want[on]).all(), (cid, fam)
            assert st["top_p"][on].min() >= 0.99, (cid, fam, st["top_p"][on].min())
            rows = np.broadcast_to(np.repeat(on.transpose(0, 2, 1), case.D, axis=2), bound.shape)      # [B, Lq, H*D]
            assert bound[rows].max() < 2e-2, (cid, fam, bound[rows].max())
        if fam in ("WA", "WD"):
            assert (st["n_small"][done] > 0).all(), (cid, fam)                          # every row has keys whose P is an fp16 subnormal or 0
            assert st["smax"][done].max() >= 39.0


def test_hot_keys_reach_every_position():
    """Over the peaked families of a case the +-1 keys sit on every candidate position: 0, 1, 31, 32, 63, 64, Lk-2, Lk-1 and both ends of every split."""
    for case in A.CASES:
        got = set()
        for fam in case.family_list():
            if fam.startswith("P"):
                sp = A.special_keys(case, int(fam[1:]))
                got |= set(sp[..., :2].reshape(-1).tolist())
        want = {k for k in (0, 1, 31, 32, 63, 64, case.Lk - 2, case.Lk - 1) if 0 <= k < case.Lk}
        if case.nsplit > 1:
            bounds = case.split_bounds()
            assert len(bounds) == case.nsplit and bounds[-1][1] == case.Lk - 1 and all(a <= b for a, b in bounds)
            want |= {k for ab in bounds for k in ab}
        assert want <= got, (case.id, sorted(want - got))
        if case.Lk >= 4:
            assert (A.special_keys(case, 0) >= 0).all()
            s = A.special_keys(case, 0).reshape(-1, 4)
            assert all(len(set(r)) == 4 for r in s.tolist())


def test_table_reaches_every_kernel_instance():
    reach = {(c.kernel, c.dpad) for c in A.CASES}
    assert {(A.TILED, d) for d in (32, 48, 64, 80, 96, 128, 160)} <= reach
    assert (A.KVRES, 64) in reach
    assert {(A.PIPELINED, d) for d in (48, 64, 80)} <= reach
    assert {c.nsplit for c in A.CASES} >= {1, 2, 3, 5}
    assert {c.D for c in A.CASES if c.group == "tiled-d"} == {8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 128, 160}
    # the pipelined cases walk every residue of the V^T triple buffer, and the one-key last split exists
    assert {(c.Lk // 64) % 3 for c in A.CASES if c.kernel == A.PIPELINED} == {0, 1, 2}
    assert any(c.nsplit > 1 and c.split_bounds()[-1][0] == c.split_bounds()[-1][1] for c in A.CASES)
    # the selection rules of csrc/attn.hip on 256 compute units, restated: what each case is meant to reach
    for c in A.CASES:
        pairs = c.B * c.H
        kvres = c.D == 64 and 256 <= c.Lk <= 608 and c.Lq >= 256 and pairs >= 256 and -(-pairs // 256) / (pairs / 256) <= 1.07
        blocks = (c.Lq // 128) * pairs
        sa = c.Lq % 128 == 0 and c.Lk % 128 == 0 and c.Lk >= 256 and 32 < c.D <= 80 and 256 <= blocks <= 8 * 256
        if kvres:
            want = (A.KVRES, 64, 1)
        elif sa:
            want = (A.PIPELINED, 48 if c.D <= 48 else 64 if c.D <= 64 else 80, 1)
        else:
            base, ntiles, ns = -(-c.Lq // 128) * pairs, -(-c.Lk // 64), 1
            if base < 256 and ntiles >= 8:
                n0 = min(-(-512 // base), ntiles // 4)
                if n0 > 1:
                    ns = -(-ntiles // -(-ntiles // n0))
            want = (A.TILED, A.dpad_of(c.D), ns)
        assert (c.kernel, c.dpad, c.nsplit) == want, (c.id, want)


@pytest.mark.parametrize("cid", [c.id for c in A.CASES if c.layouts])
def test_layouts_address_the_operands(cid):
    case = A.BY_ID[cid]
    Q, K, V = A.inputs(case, "P0")
    mask = A.mask_rows(case) if case.masked else None
    for layout in ("packed", "packed-maskpad") + case.layouts:
        bufs, kw = A.lay_out(case, layout, Q, K, V, mask)
        q, k, v, m = A.gather(case, bufs, kw)
        assert np.array_equal(q, Q) and np.array_equal(k, K) and np.array_equal(v, V), (cid, layout)
        assert (m is None) == (mask is None) and (m is None or np.array_equal(m, mask)), (cid, layout)
        idx = A.o_index(case, kw)
        assert idx.min() == A.O_GUARD and idx.max() == bufs["O"].size - A.O_GUARD - 1 and len(np.unique(idx)) == idx.size
        # what odise_hip_attention requires of a layout (and the model's call sites keep)
        assert all(kw[n] % 8 == 0 for n in ("ldq", "ldk", "ldvt", "strideQ", "strideK", "strideVt")) and kw["ldo"] % 4 == 0 and kw["strideO"] % 4 == 0
        assert kw["ldvt"] >= A.round_up(case.Lk, 8) and kw.get("offK", 0) % 8 == 0 and kw["offO"] % 4 == 0
        if m is not None:
            assert kw["ldmask"] % 4 == 0 and kw["ldmask"] >= A.round_up(case.Lk, 4) and kw["strideMask"] % 4 == 0 and kw.get("offMask", 0) % 4 == 0
