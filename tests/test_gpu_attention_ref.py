"""GPU: odise_hip_attention (csrc/attn.hip: the tiled kernel with and without the key split + combine pass, the K / V^T-resident kernel, the
pipelined self-attention kernel) against the float64 restatement of tests/attn_reference.py on the crafted inputs, masks and memory layouts of
tests/attn_cases.py, which tests/test_attn_reference_cpu.py holds to torch and checks for vacuity.

Every run asserts
  * which kernel, padded head dim and key split ran (odise_hip_last_attention) - on a device with 256 compute units, for which the shapes are
    chosen; on another one what ran is printed and the numeric checks stay;
  * a finite output with |got - ref| <= bound elementwise, bound = 2^-11 |ref| + 2^-10 sum_k p_k |v_k| + 2^-24 sum_k |v_k| / L as derived in
    tests/attn_reference.py, nothing added (where the bound is 0 - a row that sees no key - the output is 0 to the bit);
  * the canary around and between the rows of O intact.
One test is one shape with its families, masks and layouts looped inside; a line per run gives the worst err / bound.  On the shapes with 256
(head, image) pairs the float64 reference of the Gaussian, wide and flat families is computed for a fixed quarter of the pairs (every fourth,
both images; host time) and the peaked family for all of them; the finiteness and canary checks cover the whole output either way.

Measured on an MI355X (256 compute units), worst err / bound over all runs, per kernel and family (G Gaussian, P peaked, WA / WD wide, FL flat with one
value; F1 is exact everywhere):
    tiled, no key split        G 0.44  P 0.33  WA 0.18  WD 0.19  FL 0.21
    tiled, split + combine     G 0.17  P 0.31  WA 0.18  WD 0.19  FL 0.22
    K / V^T-resident           G 0.25  P 0.33  WA 0.19  WD 0.19  FL 0.19
    pipelined                  G 0.25  P 0.29  WA 0.28           FL 0.00
Every case ran on the kernel, padded head dim and split count its row of tests/attn_cases.py names."""
import numpy as np
import pytest

import attn_cases as A
from attn_reference import attention_f64

pytestmark = pytest.mark.gpu


def describe(which):
    return f"{A.KERNEL_NAMES.get(which & 255, which & 255)} DPAD {which >> 8 & 255} nsplit {which >> 16}"


def upload(ctx, bufs):
    dev = {}
    for name in ("Q", "K", "Vt", "mask"):
        if name in bufs:
            dev[name] = dev["Q"] if name == "K" and bufs["K"] is bufs["Q"] else ctx.to_device(bufs[name])
    return dev


def launch(ctx, case, dev, bufs, kw):
    """One odise_hip_attention call into a fresh canary-filled O: (output [B, Lq, H*D] fp16, what ran)."""
    O = ctx.to_device(bufs["O"])
    ctx.attention(dev["Q"], dev["K"], dev["Vt"], case.H, case.scale, mask=dev.get("mask"), out=O, **kw)
    which = ctx.lib.odise_hip_last_attention()
    got = O.numpy()
    idx = A.o_index(case, kw)
    outside = np.ones(got.size, bool)
    outside[idx.reshape(-1)] = False
    assert (got.view(np.uint16)[outside] == A.CANARY).all(), "attention wrote outside O[b, :Lq, :H*D]"
    return got[idx], which


def held(case, fam, got, ref, bound, what):
    """Asserts finite and within the bound; returns the worst err / bound."""
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    pairs = case.pairs(fam)
    sel = np.ones(ref.shape, bool) if pairs is None else np.broadcast_to(np.repeat(pairs, case.D, axis=1)[:, None, :], ref.shape)
    err = np.abs(got.astype(np.float64) - ref)[sel]
    bnd = bound[sel]
    ratio = float((err / np.where(bnd > 0, bnd, 1.0))[bnd > 0].max()) if (bnd > 0).any() else 0.0
    print(f"[attn] {what}: worst err / bound {ratio:.3f} (max err {err.max():.3e})")
    assert (err[bnd == 0] == 0).all(), f"{what}: non-zero output where no visible key has a value"
    assert ratio <= 1.0, f"{what}: err / bound {ratio:.3f}"
    return ratio


@pytest.mark.parametrize("cid", list(A.BY_ID))
def test_attention_against_float64(ctx, cid):
    case = A.BY_ID[cid]
    cus = ctx.device_info()[1]
    mask = A.mask_rows(case) if case.masked else None
    assert ctx.get_option(ctx.OPT_ATTN_KV_RESIDENT) == 0

    def ran(which, want, what):
        if cus == 256:
            assert which == want, f"{what}: ran {describe(which)}, meant for {describe(want)}"
        elif which != want:
            print(f"[attn] {what}: {cus} compute units: ran {describe(which)} (on 256: {describe(want)})")

    tiled = A.TILED | A.dpad_of(case.D) << 8 | 1 << 16
    runs = case.runs()
    order = sorted(range(len(runs)), key=lambda i: ([r[:2] for r in runs].index(runs[i][:2]), i))       # runs of one reference side by side
    ref_of, packed_out = None, {}
    try:
        for fam, masked, layout in (runs[i] for i in order):
            what = f"{cid} {fam}{' masked' if masked else ''} {layout}"
            Q, K, V = A.inputs(case, fam)
            m = mask if masked else None
            if ref_of != (fam, masked):
                ref, bound = attention_f64(Q, K, V, case.H, case.scale, m, pairs=case.pairs(fam))
                ref_of = (fam, masked)
            bufs, kw = A.lay_out(case, layout, Q, K, V, m)
            dev = upload(ctx, bufs)
            got, which = launch(ctx, case, dev, bufs, kw)
            ran(which, case.expect, what)
            held(case, fam, got, ref, bound, f"{what} [{describe(which)}]")
            if layout == "packed":
                packed_out[fam, masked] = got
            if layout == "packed-maskpad":      # the padding bytes [Lk, ldmask) all 1 instead of all 0, one more word of them: not a bit may move
                assert np.array_equal(got.view(np.uint16), packed_out[fam, masked].view(np.uint16)), f"{what}: the mask padding reached the output"
            if case.kernel == A.KVRES:
                # never the resident kernel: the tiled one, or - 256 x 256 is whole 128-blocks - the pipelined one; then (6) the tiled one there too
                sa = case.Lq % 128 == 0 and case.Lk % 128 == 0 and not masked
                for opt, want in ((2, A.PIPELINED | 64 << 8 | 1 << 16 if sa else tiled),) + (((6, tiled),) if sa else ()):
                    ctx.set_option(ctx.OPT_ATTN_KV_RESIDENT, opt)
                    other, which = launch(ctx, case, dev, bufs, kw)
                    ran(which, want, f"{what} option {opt}")
                    held(case, fam, other, ref, bound, f"{what} option {opt} [{describe(which)}]")
                ctx.set_option(ctx.OPT_ATTN_KV_RESIDENT, 0)
            if case.kernel == A.PIPELINED:
                ctx.set_option(ctx.OPT_ATTN_KV_RESIDENT, 4)
                other, which = launch(ctx, case, dev, bufs, kw)
                ctx.set_option(ctx.OPT_ATTN_KV_RESIDENT, 0)
                ran(which, tiled, f"{what} option 4")
                assert np.array_equal(got.view(np.uint16), other.view(np.uint16)), f"{what}: pipelined and tiled attention differ"
            for d in set(dev.values()):
                d.free()
    finally:
        ctx.set_option(ctx.OPT_ATTN_KV_RESIDENT, 0)


# ---- entry validation --------------------------------------------------------------------------------------------------------------------------
BAD_LAYOUTS = {
    "strideQ": dict(strideQ=4), "strideK": dict(strideK=4), "strideVt": dict(strideVt=4), "strideO": dict(strideO=2), "strideMask": dict(strideMask=2),
    "Q": dict(offQ=4), "K": dict(offK=4), "Vt": dict(offVt=4), "O": dict(offO=2), "mask": dict(offMask=2),
}


@pytest.mark.parametrize("which", list(BAD_LAYOUTS))
def test_attention_rejects_rows_that_lose_their_alignment(ctx, which):
    """Batch strides that are no multiple of 8 (Q, K, V^T) / 4 (O, mask) elements and operands that do not start on 16 (Q, K, V^T) / 8 (O) / 4 (mask)
    bytes would put the kernels' 16-, 8- and 4-byte accesses across their natural alignment: ODISE_ERR_ARG, nothing launched, O untouched.  (Every
    leading dimension stays valid here, and every buffer has room for the shifted layout.)"""
    case = A.Case("bad", 2, 2, 8, 16, 8, A.TILED, 32, seed=900)
    Q, K, V = A.inputs(case, "G")
    bufs, kw = A.lay_out(case, "packed", Q, K, V, A.mask_rows(case))
    room = {n: np.concatenate([b.reshape(-1), np.zeros(64, b.dtype)]) for n, b in bufs.items() if n != "O"}
    room["O"] = np.concatenate([bufs["O"], bufs["O"][:A.O_GUARD]])
    dev = {n: ctx.to_device(b) for n, b in room.items()}
    for name, delta in BAD_LAYOUTS[which].items():
        kw[name] = kw.get(name, 0) + delta
    with pytest.raises(RuntimeError, match=r"attention failed \(code -1\)"):
        ctx.attention(dev["Q"], dev["K"], dev["Vt"], case.H, case.scale, mask=dev["mask"], out=dev["O"], **kw)
    ctx.sync()
    assert (dev["O"].numpy().view(np.uint16) == A.CANARY).all()
