"""Inputs and shapes shared by tests/test_glue_reference_cpu.py (the float64 restatement against torch's own operators) and
tests/test_gpu_glue_ops.py (the kernels against the restatement), and the float32 torch evaluations of the two operations whose tolerance
is measured instead of derived (softmax_rows, classify_rows).

Every input has structure - a smooth coarse field plus noise, a ramp - so that a shifted, transposed or mis-strided result is a large error."""
import numpy as np
import torch

import glue_reference as R

U = 2.0 ** -24          # half an fp32 step, relative
STEP16 = 2.0 ** -10     # one fp16 step, relative


def rng(seed):
    return np.random.default_rng(seed)


def field(g, lead, h, w, std=4.0, noise=0.3, coarse=(4, 5)) -> np.ndarray:
    """[*lead, h, w] float64: a coarse normal field of standard deviation `std`, upsampled bicubically, plus white noise."""
    c = g.standard_normal(tuple(lead) + coarse) * std
    return R.bicubic(c, h, w)[0] + noise * g.standard_normal(tuple(lead) + (h, w))


def image01(g, N, H, W) -> np.ndarray:
    """[N, 3, H, W] fp32 in [0, 1]: a diagonal ramp (different per channel) plus a coarse field."""
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    ramp = np.stack([0.6 * y + 0.2 * x, 0.2 * y + 0.6 * x, 0.4 * (1 - y) + 0.4 * x])[None]
    return np.clip(ramp + 0.1 + field(g, (N, 3), H, W, std=0.08, noise=0.02), 0.0, 1.0).astype(np.float32)


def f16(x) -> np.ndarray:
    return np.asarray(x, np.float32).astype(np.float16)


# ---- shapes (tests/test_gpu_glue_ops.py documents why each is there) -----------------------------------------------------------------------------
CROP_IMG = (2, 3, 40, 56)
CROP_S = 16
CROP_BOXES = [(0, 0), (0, 40), (24, 0), (24, 40), (11, 23), (5, 33)]                 # K = 6, four flush with a border each way
BICUBIC_BOXES = [(0, 0), (0, 40), (24, 0), (24, 40), (12, 20)]                       # disjoint for every s <= 16
BICUBIC_S = [12, 15, 16]
OUTSIDE = 50.0                                                                        # what lies around a bicubic window
PREPROCESS = [(80, 120), (120, 80), (56, 56), (112, 122)]
BILINEAR_NORM = [(40, 72), (72, 40), (56, 56)]
CLIP_S = 56
NEAREST = [((5, 7), (16, 16)), ((16, 16), (16, 16)), ((12, 20), (32, 32))]
STITCH = {"k4_12": ((0, 4), (0, 4), 12), "k9_16": ((0, 4, 8), (0, 4, 8), 16), "k9_12": ((0, 2, 4), (0, 2, 4), 12), "k4_16_hole": ((0, 4), (0, 4), 16)}
BILINEAR_ADD = [((6, 10), (12, 20)), ((5, 7), (9, 13)), ((6, 10), (6, 10))]
BINARIZE_HW = [8, 64, 2056]
ATTN_MASK = [((24, 40), (24, 40)), ((24, 40), (12, 20)), ((24, 40), (6, 10)), ((12, 20), (24, 40))]
SOFTMAX_COLS = [8, 100, 2048, 2056, 4096, 4104, 8192]
SOFTMAX_SCALES = [1.0, 0.125]
L2_ROWS, L2_C = [1, 4, 5, 9], [32, 100, 768]
CLASSIFY_K = [1, 5, 300]
CLASSIFY_SCALES = [(100.0, 14.0), (14.0, 100.0)]
MSDA_LEVELS = ((4, 6), (8, 12), (16, 24))


def crop_image(seed=1) -> np.ndarray:
    return (image01(rng(seed), CROP_IMG[0], *CROP_IMG[2:]) * 4.0 - 1.0).astype(np.float32)


def bicubic_image(s, seed=2) -> np.ndarray:
    """OUTSIDE everywhere but in the s x s windows of BICUBIC_BOXES: a tap read past a window's edge shows as an error of its size."""
    g = rng(seed + s)
    img = np.full(CROP_IMG, OUTSIDE, np.float32)
    for y, x in BICUBIC_BOXES:
        img[:, :, y:y + s, x:x + s] = field(g, CROP_IMG[:2], s, s, std=1.0, noise=0.1, coarse=(3, 3))
    return img


def stitch_boxes(name):
    ys, xs, size = STITCH[name]
    return [(y, x) for y in ys for x in xs], size


def mask_rows(g, rows, h, w, dtype) -> np.ndarray:
    """[rows, h, w] logits of standard deviation ~4 in the kernel's input type (as float64)."""
    v = field(g, (rows,), h, w)
    return f16(v).astype(np.float64) if dtype == np.float16 else v.astype(np.float32).astype(np.float64)


def binarize_rows(hw, dtype, seed=5) -> np.ndarray:
    """[6, hw]: four field rows, one all-negative, one all-positive."""
    g = rng(seed + hw)
    v = mask_rows(g, 6, 1, hw, dtype).reshape(6, hw)
    v[4] = -np.abs(v[4]) - 0.5
    v[5] = np.abs(v[5]) + 0.5
    return v


def attn_rows(src, dst, dtype, seed=6) -> np.ndarray:
    """[8, H, W]: six field rows; row 6 masked everywhere (all logits well below zero); row 7 with a single visible key."""
    (H, W), (oh, ow) = src, dst
    g = rng(seed + H * 1000 + oh)
    v = mask_rows(g, 8, H, W, dtype)
    v[6] = -np.abs(v[6]) - 5.0
    for pos in ((0, 0), (1, 1)):
        for spike in (2.0, 4.0, 40.0, 100.0):
            row = np.full((H, W), -10.0)
            row[pos] = spike
            out, und, _ = R.attn_mask(row[None], oh, ow, oh * ow)
            if (out == 0).sum() == 1 and not und.any():
                v[7] = row
                return v
    raise AssertionError("no single-key row for this geometry")


def softmax_input(cols, seed=7):
    """x [5, ld] f16 with NaN in the padding columns cols..ld-1; row 3 carries a +60 spike.  -> (x, ld)"""
    g = rng(seed + cols)
    ld = (cols + 7) // 8 * 8 + 8
    x = np.full((5, ld), np.nan, np.float16)
    x[:, :cols] = f16(g.standard_normal((5, cols)) * 2.0 + np.sin(np.arange(cols) / 37.0) * 3.0)
    x[3, cols // 3] += np.float16(60.0)
    return x, ld


SOFTMAX_SPIKE_ROW = 3


def softmax_f32(x16, scale) -> np.ndarray:
    """The VAE attention's softmax as float32 torch evaluates it, rounded to the kernel's output type."""
    return torch.softmax(torch.from_numpy(np.asarray(x16, np.float32)) * np.float32(scale), -1).half().numpy().astype(np.float64)


def classify_case(K, seed=8):
    """-> dict(L1 [6, Ktot + 1], L2 [6, Ktot], seg, ovl, binary [6, 2]); rows 0..3 ordinary, row 4: the null text dominates, row 5: one class
    dominates by 40 (in scaled logits, whichever scale is applied)."""
    g = rng(seed + K)
    sizes = [1 + k % 4 for k in range(K)]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    Ktot = int(seg[-1])
    L1 = (0.25 + 0.02 * g.standard_normal((6, Ktot + 1))).astype(np.float32)
    L2 = (0.20 + 0.05 * g.standard_normal((6, Ktot))).astype(np.float32)
    L1[4, Ktot] = L1[4, :Ktot].max() + np.float32(0.35)                      # +35 / +4.9 over the best class
    k = K // 2
    L1[5, seg[k]] = L1[5, :Ktot].max() + np.float32(40.0 / 14.0)            # >= 40 at either scale
    ovl = (g.random(K) < 0.5).astype(np.int32)
    binary = (g.standard_normal((6, 2)) * 2.0).astype(np.float32)
    return {"L1": L1, "L2": L2, "seg": seg, "ovl": ovl, "binary": binary, "K": K, "Ktot": Ktot}


ALPHA, BETA = 0.4, 0.8


def classify_torch(c, ls1, ls2, binary, dtype) -> np.ndarray:
    """The reference's own formula (helper.py:96-100, odise.py:1507-1536, 307-323 / 559-565) in torch at `dtype`."""
    L1, L2 = torch.from_numpy(c["L1"]).to(dtype), torch.from_numpy(c["L2"]).to(dtype)
    seg, K = c["seg"], c["K"]
    f = lambda v: torch.tensor(np.float32(v).item(), dtype=dtype)
    logits = L1 * f(ls1)                                                                   # [rows, Ktot + 1], scaled
    pred = torch.stack([logits[:, seg[k]:seg[k + 1]].max(-1).values for k in range(K)] + [logits[:, -1]], -1)
    clip = torch.stack([(L2 * f(ls2))[:, seg[k]:seg[k + 1]].max(-1).values for k in range(K)], -1)
    p, q = pred[:, :-1].softmax(-1), clip.softmax(-1)
    ovl = torch.from_numpy(c["ovl"]).to(dtype)
    alpha, beta = f(ALPHA), f(BETA)
    base = (p ** (1 - alpha) * q ** alpha).log() * ovl
    novel = (p ** (1 - beta) * q ** beta).log() * (1 - ovl)
    # a probability that underflows makes log() -inf and -inf * 0 NaN in the OTHER branch: the reference adds the two, each category is in one
    open_logits = torch.where(ovl.bool(), base, novel)
    pn = pred.softmax(-1)[:, -1] if not binary else torch.from_numpy(c["binary"]).to(dtype).softmax(-1)[:, 1]
    probs = torch.cat([open_logits.softmax(-1) * (1 - pn)[:, None], pn[:, None]], -1)
    return torch.log(probs + 1e-8).double().numpy()


def msda_case(seed=9):
    g = rng(seed)
    B, M = 2, 8
    Lq = sum(h * w for h, w in MSDA_LEVELS)
    off = (g.standard_normal((B, Lq, M, 3, 4, 2)) * 3.0).astype(np.float32)
    aw = (g.standard_normal((B, Lq, M, 12)) * 2.0).astype(np.float32)
    value = f16(g.standard_normal((B, Lq, M, 32)))
    return B, M, Lq, off, aw, value
