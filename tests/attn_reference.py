"""Float64 restatement of odise_hip_attention (csrc/attn.hip) and the bound its fp16 / fp32 arithmetic is held to.

    O[b, q, h*D + d] = sum_k softmax_k(scale * Q[b, q, h] . K[b, k, h]) V[b, k, h*D + d]       over the keys the mask leaves visible

The inputs are the fp16-rounded arrays the device reads, taken to float64: the restatement has no input rounding of its own.  A row that sees no
key is 0 (the kernel's l = 0 -> inv = 0).

Bound.  The device differs from exact arithmetic in three places (l_run sums the unrounded fp32 p, so only the numerator carries the P error):
  * P is rounded to fp16 before V^T P^T: 2^-11 relative per key, or half a subnormal step (2^-25 <= 2^-24) where p < 2^-14;
  * the output is rounded to fp16: 2^-11 relative;
  * the fp32 terms - the score sum over D, scale * log2e, v_exp_f32, the accumulation over Lk - each a few 2^-24 relative for
    |score * scale * log2e| <= 40.
With p_k the exact softmax, v_k the value row and L = sum_k exp(s_k - max s) >= 1 (sums over the visible keys only):

    bound = 2^-11 |ref|  +  2^-10 sum_k p_k |v_k|  +  2^-24 sum_k |v_k| / L

Half of the middle term is the P rounding, the other half the allowance for the fp32 terms (about 30 times what they need).  Nothing else is
added anywhere: a row without a visible key, or whose visible values are all zero, has bound 0 and must be 0 to the bit."""
import numpy as np

SUBNORMAL_P = 2.0 ** -14      # below this an fp16 P is a subnormal


def attention_f64(Q, K, V, H, scale, mask=None, pairs=None, stats=False):
    """Q [B, Lq, H*D], K / V [B, Lk, H*D] (any float dtype, used as float64), mask [B, Lq, Lk] (non-zero = hidden) or None.
    Returns (out, bound) [B, Lq, H*D] float64; computed per (b, h) so that the working set stays at one Lq x Lk matrix.
    pairs: optional [B, H] bool - only these (b, h) are computed, the rest of out / bound is NaN (the caller compares the computed ones only).
    stats=True also returns a dict of [B, H, Lq] arrays: top_p / top_k (the largest probability of the row and its key; -1 for a row that sees
    no key), n_small (visible keys with p < 2^-14) and smax (the largest |score * scale * log2(e)| over the visible keys)."""
    Q, K, V = (np.asarray(x, np.float64) for x in (Q, K, V))
    B, Lq, HD = Q.shape
    Lk = K.shape[1]
    D = HD // H
    assert HD == H * D and K.shape == (B, Lk, HD) and V.shape == (B, Lk, HD)
    out = np.full((B, Lq, HD), np.nan)
    bound = np.full((B, Lq, HD), np.nan)
    st = None
    if stats:
        st = {"top_p": np.zeros((B, H, Lq)), "top_k": np.full((B, H, Lq), -1, np.int64), "n_small": np.zeros((B, H, Lq), np.int64),
              "smax": np.zeros((B, H, Lq))}
    for b in range(B):
        vis = None
        if mask is not None:
            vis = np.asarray(mask[b]) == 0                      # [Lq, Lk]
            anyvis = vis.any(axis=1)
        for h in range(H):
            if pairs is not None and not pairs[b, h]:
                continue
            c = slice(h * D, (h + 1) * D)
            q, k, v = Q[b, :, c], K[b, :, c], V[b, :, c]
            s = (q @ k.T) * scale
            if vis is not None:
                s = np.where(vis, s, -np.inf)
            m = s.max(axis=1, keepdims=True)
            m = np.where(np.isfinite(m), m, 0.0)                # a row without a visible key: exp(-inf - 0) = 0 everywhere
            e = np.exp(s - m)
            L = e.sum(axis=1, keepdims=True)
            inv = np.where(L > 0, 1.0 / np.where(L > 0, L, 1.0), 0.0)
            p = e * inv
            av = np.abs(v)
            ref = p @ v
            if vis is None:
                sum_av = av.sum(axis=0, keepdims=True)
            else:
                sum_av = vis.astype(np.float64) @ av
            out[b, :, c] = ref
            bound[b, :, c] = 2.0 ** -11 * np.abs(ref) + 2.0 ** -10 * (p @ av) + 2.0 ** -24 * sum_av * inv
            if stats:
                st["top_p"][b, h] = p.max(axis=1)
                tk = p.argmax(axis=1)
                st["top_k"][b, h] = tk if vis is None else np.where(anyvis, tk, -1)
                seen = np.ones_like(p, bool) if vis is None else vis
                st["n_small"][b, h] = ((p < SUBNORMAL_P) & seen).sum(axis=1)
                st["smax"][b, h] = np.where(seen, np.abs(s), 0.0).max(axis=1) * np.log2(np.e)
    return (out, bound, st) if stats else (out, bound)
