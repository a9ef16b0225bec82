"""Shapes, inputs, masks and memory layouts shared by tests/test_attn_reference_cpu.py (the float64 restatement against torch, and the
conditions that make these inputs mean something) and tests/test_gpu_attention_ref.py (the three kernels of csrc/attn.hip and the combine pass
against the restatement).

Gaussian inputs hide weight errors: the softmax is nearly flat and one wrong key moves an average of Lk rows by 1 / Lk.  So besides the Gaussian
baseline the scores here are RANK ONE per head - Q[q] = a_q u, K[k] = c_k u / D with u a fixed +-1 vector, score = a_q c_k at any D >= 8 - and the
families choose a_q / c_k so that a wrong weight is a large error:

  G    Gaussian Q, K, V (the baseline of tests/test_gpu_ops.py).
  P<r> peaked: a_q alternates sign, c_k is 0 except +1 / -1 at two "hot" keys and +0.5 / -0.5 at two runner-up keys elsewhere.  An even row
       puts >= 0.99 of its weight on the +1 key (on the +0.5 key if the mask hides the first), an odd row on the -1 / -0.5 keys: a key that is
       misindexed, dropped or wrongly masked is an error of order 1 against a bound of order 1e-3.  The hot keys rotate over (b, h) - and over
       the rotations r where there are fewer (b, h) than positions - through 0, 1, 31, 32, 63, 64, Lk-2, Lk-1 and the first and last key of
       every key split.
  F1   flat: Q = 0, V = 1: the output is 1 to the bound (l against the numerator).
  FL   flat with V = 1 on the last key only: 1 / (visible keys) where the last key is visible, else exactly 0.
  WA / WD  wide: c_k ramps so that score * scale * log2(e) spans ~0.6 .. 39.5 (four row scalings: 1, 7/8, 3/4, 5/8 of that) ascending over the keys
       - the running maximum rises and the accumulator is rescaled every tile - or descending - it never rises, and most of P is an fp16 subnormal
       or zero when it enters the second MFMA.

V is seeded normal except in F.  Masks (u8, non-zero = hidden) give each query row q one of twelve patterns by q % 12 (mask_rows)."""
import functools
import math
from dataclasses import dataclass

import numpy as np

TILED, KVRES, PIPELINED = 0, 1, 2
KERNEL_NAMES = {TILED: "tiled", KVRES: "kv-resident", PIPELINED: "pipelined"}
CANARY = np.uint16(0x5A5A)      # 203.25 as fp16: what O holds wherever the kernel must not write
O_GUARD = 64                    # canary elements before and after O
LOG2E = math.log2(math.e)
W_SPAN = 39.5                   # largest score * scale * log2(e) of the wide family (fp16 rounding of a_q and c_k / D keeps it below 40)
W_ROWS = (1.0, 0.875, 0.75, 0.625)


def dpad_of(D):
    return next(p for p in (32, 48, 64, 80, 96, 128, 160) if D <= p)


def round_up(x, m):
    return (x + m - 1) // m * m


def f16(x):
    return np.asarray(x, np.float32).astype(np.float16)


@dataclass(frozen=True)
class Case:
    group: str
    B: int
    H: int
    Lq: int
    Lk: int
    D: int
    kernel: int                  # the kernel, padded head dim and key split this shape is meant to reach on 256 compute units
    dpad: int
    nsplit: int = 1
    families: tuple = ("G", "P")
    masked: bool = False         # also run G, P0, F1, FL under mask_rows
    layouts: tuple = ()          # besides "packed": "qk", "side", "wide-o" (family P0, masked where the case is)
    quarter: bool = False        # reference of the G / W / F families on a fixed quarter of the (b, h) pairs (host time); P on all
    seed: int = 0

    @property
    def id(self):
        return f"{self.group}-B{self.B}H{self.H}Lq{self.Lq}Lk{self.Lk}D{self.D}"

    @property
    def scale(self):
        return float(self.D) ** -0.5

    @property
    def expect(self):
        return self.kernel | self.dpad << 8 | self.nsplit << 16

    def split_bounds(self):
        """[(first key, last key)] of every key split of launch_attn (64-key tiles dealt in runs of ceil(ntiles / nsplit))."""
        ntiles = (self.Lk + 63) // 64
        per = (ntiles + self.nsplit - 1) // self.nsplit
        return [(s * per * 64, min(self.Lk, (s + 1) * per * 64) - 1) for s in range(self.nsplit)]

    def hot_candidates(self):
        c = [0, 1, 31, 32, 63, 64, self.Lk - 2, self.Lk - 1]
        if self.nsplit > 1:
            for a, b in self.split_bounds():
                c += [a, b]
        out = []
        for k in c:
            if 0 <= k < self.Lk and k not in out:
                out.append(k)
        return out

    def rotations(self):
        """How many P families it takes to put a hot key on every candidate position: each (b, h) pair carries two."""
        return max(1, -(-len(self.hot_candidates()) // (2 * self.B * self.H)))

    def family_list(self):
        out = []
        for f in self.families:
            if f == "P":
                out += [f"P{r}" for r in range(self.rotations())]
            elif f == "W":
                out += ["WA", "WD"]
            elif f == "F":
                out += ["F1", "FL"]
            else:
                out.append(f)
        return out

    def runs(self):
        """[(family, masked, layout)] in the order the GPU test walks them; runs of one (family, masked) share a reference."""
        out = [(f, False, "packed") for f in self.family_list()]
        if self.masked:
            out += [(f, True, "packed") for f in ("G", "P0", "F1", "FL")]
            out.append(("P0", True, "packed-maskpad"))          # ldmask 4 wider, padding bytes all 1: bit-identical to the run before
        out += [("P0", self.masked, lay) for lay in self.layouts]
        return out

    def pairs(self, fam):
        """[B, H] bool: the (b, h) whose reference is computed for this family (None = all)."""
        if not self.quarter or fam.startswith("P"):
            return None
        i = np.arange(self.B * self.H).reshape(self.B, self.H)
        return i % 4 == 1


def _cases():
    c = []
    # tiled kernel, every instance and every D < DPAD
    for D in (8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 96, 128, 160):
        c.append(Case("tiled-d", 1, 2, 33, 65, D, TILED, dpad_of(D), seed=D))
    # tiled kernel, Lq / Lk straddling 32, 64, 128; Lk < 8
    edges = [(1, 1), (1, 8), (31, 7), (32, 9), (33, 63), (127, 64), (128, 65), (129, 77), (130, 127), (100, 129)]
    for i, (Lq, Lk) in enumerate(edges):
        c.append(Case("tiled-edge", 2, 2, Lq, Lk, 40, TILED, 48, families=("G", "P", "F"), masked=i >= 6,
                      layouts=("qk", "wide-o") if (Lq, Lk) in ((129, 77), (100, 129)) else (), seed=100 + i))
    # tiled kernel with the keys split over blocks + attn_combine_kernel
    #   513: 9 tiles, splits of 5 and 4, the last tile one key;  833: 14 tiles, splits of 5, 5 and 4, the last tile one key;
    #   1281: 21 tiles, splits 5, 5, 5, 5, 1: the last split is a single one-key tile
    for Lq, Lk, D, ns in ((100, 513, 32, 2), (100, 833, 32, 3), (100, 1281, 32, 5), (100, 833, 40, 3), (100, 513, 160, 2), (129, 833, 32, 3)):
        c.append(Case("tiled-split", 1, 2, Lq, Lk, D, TILED, dpad_of(D), ns, families=("G", "P", "W", "F"), masked=Lk in (833, 1281), seed=200 + Lk + D + Lq))
    # K / V^T-resident kernel: one block per (head, image), 256 pairs
    for Lq, Lk in ((256, 256), (257, 289), (300, 608), (256, 577)):
        c.append(Case("kvres", 2, 128, Lq, Lk, 64, KVRES, 64, families=("G", "P", "W", "F") if Lk == 577 else ("G", "P"), masked=Lk in (289, 577),
                      layouts=("qk", "side") if Lk == 577 else (), quarter=True, seed=300 + Lk))
    # one key fewer / more than the resident kernel takes: the tiled kernel
    for Lk in (255, 609):
        c.append(Case("kvres-not", 2, 128, 256, Lk, 64, TILED, 64, quarter=True, seed=400 + Lk))
    # pipelined self-attention: 4, 6 and 8 key tiles = every residue of the V^T buffer rotation, D = DPAD and D < DPAD of each instance
    for i, (D, Lk) in enumerate(((40, 256), (48, 384), (56, 512), (64, 256), (72, 384), (80, 512))):
        c.append(Case("pipelined", 2, 128, 128, Lk, D, PIPELINED, dpad_of(D), families=("G", "P", "WA") + (("F",) if i == 0 else ()),
                      layouts=("qk",) if i == 0 else (), quarter=True, seed=500 + i))
    c.append(Case("pipelined", 1, 128, 256, 384, 40, PIPELINED, 48, families=("G", "P", "WA"), quarter=True, seed=510))
    return c


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def head_signs(case):
    """[H, D] of +-1: the direction u of every head's rank-one scores."""
    g = np.random.default_rng(7000 + case.seed)
    return np.where(g.random((case.H, case.D)) < 0.5, -1.0, 1.0)


def special_keys(case, rot=0):
    """[B, H, 4] int: the keys holding c = +1, -1, +0.5, -0.5 of every (b, h) (-1: Lk has no room for it).  The +-1 keys walk the candidate
    positions; each runner-up sits half the keys away from its hot key (another 64-key tile wherever Lk > 128)."""
    cand = case.hot_candidates()
    n = len(cand)
    out = np.full((case.B, case.H, 4), -1, np.int64)
    for b in range(case.B):
        for h in range(case.H):
            j = 2 * (rot * case.B * case.H + b * case.H + h)
            used = []

            def take(k):
                for step in range(case.Lk):
                    kk = (k + step) % case.Lk
                    if kk not in used:
                        used.append(kk)
                        return kk
                return -1
            kmax = take(cand[j % n])
            kmin = take(cand[(j + 1) % n])
            rmax = take(kmax + case.Lk // 2)
            rmin = take(kmin + case.Lk // 2 + 1) if kmin >= 0 else -1
            out[b, h] = (kmax, kmin, rmax, rmin)
    return out


def peak_strength(case):
    """A * scale of the peaked family: exp(A scale / 2) >= 200 Lk, so that even the runner-up (c = 0.5) outweighs all flat keys 200 to 1."""
    return 2.0 * math.log(200.0 * case.Lk)


def _rank_one(case, a, c):
    """Q [B, Lq, H*D] = a[b, h, q] u_h, K [B, Lk, H*D] = c[b, h, k] u_h / D as fp16."""
    u = head_signs(case)
    Q = np.einsum("bhq,hd->bqhd", a, u).reshape(case.B, case.Lq, case.H * case.D)
    K = np.einsum("bhk,hd->bkhd", c, u / case.D).reshape(case.B, case.Lk, case.H * case.D)
    return f16(Q), f16(K)


@functools.lru_cache(maxsize=3)
def _normal(case, which):
    """The case's seeded normal Q / K / V [B, L, H*D] as fp16, read-only: one V for all families of a case, one K for G and F."""
    L = case.Lq if which == "Q" else case.Lk
    g = np.random.default_rng(case.seed * 16 + "QKV".index(which))
    x = f16(g.standard_normal((case.B, L, case.H * case.D), np.float32))
    x.setflags(write=False)
    return x


def inputs(case, fam):
    """(Q, K, V) fp16: [B, Lq, H*D], [B, Lk, H*D], [B, Lk, H*D]."""
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.D
    HD = H * D
    V = _normal(case, "V")
    if fam == "G":
        return _normal(case, "Q"), _normal(case, "K"), V
    if fam in ("F1", "FL"):
        V = np.zeros((B, Lk, HD), np.float16)
        V[:, Lk - 1 if fam == "FL" else slice(None)] = 1.0
        return np.zeros((B, Lq, HD), np.float16), _normal(case, "K"), V
    if fam.startswith("P"):
        sp = special_keys(case, int(fam[1:]))
        A = peak_strength(case) / case.scale
        a = np.broadcast_to(np.where(np.arange(Lq) % 2 == 0, A, -A), (B, H, Lq))
        c = np.zeros((B, H, Lk))
        bi, hi = np.meshgrid(np.arange(B), np.arange(H), indexing="ij")
        for j, val in ((3, -0.5), (2, 0.5), (1, -1.0), (0, 1.0)):
            ok = sp[..., j] >= 0
            c[bi[ok], hi[ok], sp[..., j][ok]] = val
        Q, K = _rank_one(case, a, c)
        return Q, K, V
    if fam in ("WA", "WD"):
        ramp = (1.0 + 63.0 * np.arange(Lk) / max(Lk - 1, 1)) / 64.0
        if fam == "WD":
            ramp = ramp[::-1]
        c = np.broadcast_to(W_SPAN / LOG2E * ramp, (B, H, Lk))
        a = np.broadcast_to(math.sqrt(D) * np.array(W_ROWS)[np.arange(Lq) % 4], (B, H, Lq))
        Q, K = _rank_one(case, a, c)
        return Q, K, V
    raise KeyError(fam)


# ---- masks -------------------------------------------------------------------------------------------------------------------------------------
MASK_PATTERNS = ("none", "stripe0", "stripe1", "stripe2", "only-first", "only-last", "lead-tiles", "middle-tile", "hot-key", "all", "one-split",
                 "last-split")


def mask_rows(case):
    """[B, Lq, Lk] u8, non-zero = hidden.  Row q takes pattern q % 12:
      0 none          1-3 every third key hidden, three phases (byte order inside the kernel's 4-byte mask reads)
      4 only key 0 visible          5 only key Lk-1 visible
      6 the leading tiles hidden (128 keys; 64 / 32 where Lk is no longer than that): the running maximum is -inf into the first visible tile
      7 the middle 64-key tile hidden
      8 the hot key of this row's sign of head (q // 12) % H hidden (rotation 0): the runner-up, elsewhere, must win
      9 everything hidden: the row is 0
      10 / 11 with a key split: split 1 hidden / only the last split visible (a split whose running maximum stays -inf into the combine pass);
              without one: none."""
    B, Lq, Lk = case.B, case.Lq, case.Lk
    m = np.zeros((B, Lq, Lk), np.uint8)
    k = np.arange(Lk)
    sp = special_keys(case, 0)
    lead = 128 if Lk > 128 else 64 if Lk > 64 else 32 if Lk > 32 else 0
    mid = ((Lk + 63) // 64) // 2 * 64
    bounds = case.split_bounds() if case.nsplit > 1 else None
    for q in range(Lq):
        pat = q % 12
        if pat in (1, 2, 3):
            m[:, q, (k + pat) % 3 == 0] = 1
        elif pat == 4:
            m[:, q, 1:] = 1
        elif pat == 5:
            m[:, q, :Lk - 1] = 1
        elif pat == 6:
            m[:, q, :lead] = 1
        elif pat == 7 and Lk > 64:
            m[:, q, mid:mid + 64] = 1
        elif pat == 8:
            for b in range(B):
                m[b, q, sp[b, (q // 12) % case.H, q % 2]] = 1
        elif pat == 9:
            m[:, q] = 1
        elif pat == 10 and bounds:
            m[:, q, bounds[1][0]:bounds[1][1] + 1] = 1
        elif pat == 11 and bounds:
            m[:, q, :bounds[-1][0]] = 1
    return m


def expected_keys(case, fam, mask=None):
    """[B, H, Lq] int: the key a peaked row must put >= 0.99 of its weight on - its hot key, the runner-up where the mask hides the hot key,
    -1 where it hides both (such a row is a plain average and only held to the bound) or where Lk has no such key."""
    sp = special_keys(case, int(fam[1:]))
    odd = np.arange(case.Lq) % 2
    hot = np.where(odd[None, None, :] == 0, sp[..., 0:1], sp[..., 1:2])          # [B, H, Lq]
    run = np.where(odd[None, None, :] == 0, sp[..., 2:3], sp[..., 3:4])
    if case.Lk == 1:
        hot = np.zeros_like(hot)        # one key: every row is on it
    if mask is None:
        return hot
    vis = np.asarray(mask) == 0                                                   # [B, Lq, Lk]
    b = np.arange(case.B)[:, None, None]
    q = np.arange(case.Lq)[None, None, :]
    hot_ok = (hot >= 0) & vis[b, q, np.maximum(hot, 0)]
    run_ok = (run >= 0) & vis[b, q, np.maximum(run, 0)]
    return np.where(hot_ok, hot, np.where(run_ok, run, -1))


# ---- memory layouts ----------------------------------------------------------------------------------------------------------------------------
def _o_buffer(B, Lq, HD, ldo, strideO):
    n = O_GUARD + (B - 1) * strideO + (Lq - 1) * ldo + HD + O_GUARD
    return np.full(n, CANARY, np.uint16).view(np.float16)


def lay_out(case, layout, Q, K, V, mask=None):
    """The operands as one of the model's call sites holds them.  Returns (bufs, kw): bufs = host arrays by name ("Q", "K", "Vt", "O", "mask";
    K may be the very array of Q) and kw = the keyword arguments of Context.attention beyond the buffers.  Every padding element is poisoned:
    NaN in Q / K / V^T, the canary in O, and the mask padding as the layout says.

      packed          Q [B, Lq, HD], K [B, Lk, HD], V^T [B, HD, round_up(Lk, 8)], mask [B, Lq, round_up(Lk, 4)] with padding bytes 0
      packed-maskpad  the same with ldmask 4 wider and every padding byte 1
      qk              Q and K interleaved in one [B, max(Lq, Lk), 2 HD] buffer, K = Q + HD (the UNet's and the mask decoder's self-attention)
      side            MaskCLIP's second pass: Q packed, K inside a [B, TP, 2 HD] q|k buffer, V^T of all images side by side in one
                      [HD, B * TP] matrix (strideVt = TP: the columns after image b's Lk + padding are image b+1's values), the mask rows
                      of image b behind T0 rows of another purpose (strideMask = (T0 + Lq) * ldm, ldm = round_up(Lk, 8) + 8)
      wide-o          packed operands, O rows 8 elements wider than H*D and images 24 elements further apart than Lq rows"""
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.D
    HD = H * D
    nan = np.float16(np.nan)
    kw = dict(B=B, Lq=Lq, Lk=Lk, D=D)
    bufs = {}
    ldo, strideO = HD, Lq * HD
    if layout == "wide-o":
        ldo, strideO = HD + 8, Lq * (HD + 8) + 24
    if layout in ("qk", "side"):
        rows = max(Lq, Lk) if layout == "qk" else round_up(Lk, 8) + 8
        qk = np.full((B, rows, 2 * HD), nan, np.float16)
        qk[:, :Lk, HD:] = K
        bufs["K"] = qk
        kw.update(ldk=2 * HD, strideK=rows * 2 * HD, offK=HD)
        if layout == "qk":
            qk[:, :Lq, :HD] = Q
            bufs["Q"] = qk
            kw.update(ldq=2 * HD, strideQ=rows * 2 * HD)
        else:
            bufs["Q"] = np.ascontiguousarray(Q)
            kw.update(ldq=HD, strideQ=Lq * HD)
    else:
        bufs["Q"], bufs["K"] = np.ascontiguousarray(Q), np.ascontiguousarray(K)
        kw.update(ldq=HD, strideQ=Lq * HD, ldk=HD, strideK=Lk * HD)
    if layout == "side":
        TP = round_up(Lk, 8) + 8
        vt = np.full((HD, B * TP), nan, np.float16)
        for b in range(B):
            vt[:, b * TP:b * TP + Lk] = V[b].T
        kw.update(ldvt=B * TP, strideVt=TP)
    else:
        ldvt = round_up(Lk, 8)
        vt = np.full((B, HD, ldvt), nan, np.float16)
        vt[:, :, :Lk] = np.transpose(V, (0, 2, 1))
        kw.update(ldvt=ldvt, strideVt=HD * ldvt)
    bufs["Vt"] = vt
    bufs["O"] = _o_buffer(B, Lq, HD, ldo, strideO)
    kw.update(ldo=ldo, strideO=strideO, offO=O_GUARD)
    if mask is not None:
        if layout == "side":
            T0, ldm = 5, round_up(Lk, 8) + 8
            mb = np.ones((B, T0 + Lq, ldm), np.uint8)
            mb[:, T0:, :Lk] = mask
            kw.update(ldmask=ldm, strideMask=(T0 + Lq) * ldm, offMask=T0 * ldm)
        else:
            wide = layout == "packed-maskpad"
            ldm = round_up(Lk, 4) + (4 if wide else 0)
            mb = np.full((B, Lq, ldm), 1 if wide else 0, np.uint8)
            mb[:, :, :Lk] = mask
            kw.update(ldmask=ldm, strideMask=Lq * ldm)
        bufs["mask"] = mb
    return bufs, kw


def o_index(case, kw):
    """[B, Lq, HD] flat indices of the output elements inside the O buffer."""
    HD = case.H * case.D
    return (kw["offO"] + np.arange(case.B)[:, None, None] * kw["strideO"] + np.arange(case.Lq)[None, :, None] * kw["ldo"]
            + np.arange(HD)[None, None, :])


def gather(case, bufs, kw):
    """What the descriptor's strides address, read back from the host buffers: (Q, K, V, mask) in their logical shapes.  The CPU test holds
    this to the arrays lay_out was given, so that a layout the GPU test uploads is the layout it means."""
    B, H, Lq, Lk, D = case.B, case.H, case.Lq, case.Lk, case.D
    HD = H * D
    b = np.arange(B)[:, None, None]

    def rows(buf, off, ld, stride, L):
        return buf.reshape(-1)[off + b * stride + np.arange(L)[None, :, None] * ld + np.arange(HD)[None, None, :]]
    Q = rows(bufs["Q"], kw.get("offQ", 0), kw["ldq"], kw["strideQ"], Lq)
    K = rows(bufs["K"], kw.get("offK", 0), kw["ldk"], kw["strideK"], Lk)
    Vt = bufs["Vt"].reshape(-1)[kw.get("offVt", 0) + b * kw["strideVt"] + np.arange(HD)[None, :, None] * kw["ldvt"] + np.arange(Lk)[None, None, :]]
    M = None
    if "mask" in bufs:
        M = bufs["mask"].reshape(-1)[kw.get("offMask", 0) + b * kw["strideMask"] + np.arange(Lq)[None, :, None] * kw["ldmask"] + np.arange(Lk)[None, None, :]]
    return Q, K, np.transpose(Vt, (0, 2, 1)), M
