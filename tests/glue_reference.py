"""Float64 numpy restatement of the small operations between the GEMM stages (the kernels of csrc/decoder_ops.hip, csrc/misc.hip, the head of
csrc/classify_ops.hip and mask_binarize of csrc/elementwise.hip), each written from the reference model's own call:

  crops                  feature_extractor.py:197-224 (slide windows; T.Resize(BICUBIC) of a window smaller than the network input)
  clip_preprocess        clip.py:94 (torchvision Resize of the short side + center_crop + Normalize)
  resize_bilinear_norm   clip.py:327-332 + Normalize
  upsample_nearest       feature_extractor.py:165-168 (F.interpolate's default mode)
  stitch                 feature_extractor.py:229-248
  add_vec_table          msdeformattn.py:71-75, odise.py:657-660
  bilinear_add           msdeformattn.py:347
  mask_binarize          MaskPooling's prologue, odise.py:948-953
  attn_mask              odise.py:760-774, 683
  clip_assemble          clip.py:179-190, 268-270
  cond_inputs            ldm.py:706-709
  latent_heads           ldm.py:459-467, 535-538, 577-598; gaussian_diffusion.py:275-292
  l2_normalize           F.normalize
  classify_rows          helper.py:79-109, odise.py:1506-1536, 300-323 (559-565 for the learned binary head)
  msda_prepare           ms_deform_attn.py:103-110

As in tests/post_reference.py the tap positions and weights of an interpolation are part of the operation's definition: torch computes them in
fp32 for fp32 tensors, so they are taken in fp32 here and widened; every interpolated value, exp, log and sum is float64.

Functions whose device counterpart rounds return `(ref, cond)`: cond is the sum of |weight * tap| (and |addend|) behind every element - the
operation's own fp32 conditioning, from which the tests derive their absolute tolerance.
"""
import numpy as np

from post_reference import f16_round, resize, taps  # noqa: F401  (f16_round is re-exported for the tests)

CLIP_MEAN = np.array([0.48145466, 0.4578275, 0.40821073], np.float32).astype(np.float64)
CLIP_STD = np.array([0.26862954, 0.26130258, 0.27577711], np.float32).astype(np.float64)
_F = np.float32


# ---- interpolation ---------------------------------------------------------------------------------------------------------------------------------
def cubic_taps(out_size: int, in_size: int):
    """(idx [out, 4], w [out, 4]) of F.interpolate(mode="bicubic", align_corners=False): source coordinate scale * (dst + 0.5) - 0.5 (not
    clamped), cubic convolution with A = -0.75, tap indices clamped to the input - all in fp32 as upsample_bicubic2d does for fp32 tensors."""
    A = _F(-0.75)
    o = np.arange(out_size, dtype=np.float32)
    scale = _F(in_size) / _F(out_size)
    s = scale * (o + _F(0.5)) - _F(0.5)
    fl = np.floor(s)
    t = (s - fl).astype(np.float32)

    def c1(x):
        return ((A + _F(2)) * x - (A + _F(3))) * x * x + _F(1)

    def c2(x):
        return ((A * x - _F(5) * A) * x + _F(8) * A) * x - _F(4) * A

    x2 = _F(1) - t
    w = np.stack([c2(t + _F(1)), c1(t), c1(x2), c2(x2 + _F(1))], -1)
    assert w.dtype == np.float32
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3), 0, in_size - 1)
    return idx, w.astype(np.float64)


def _separable(x, ty, tx):
    """sum_j wy[., j] sum_i wx[., i] x[..., iy[., j], ix[., i]] and the same over absolute values."""
    (iy, wy), (ix, wx) = ty, tx
    x = np.asarray(x, np.float64)

    def run(v, wy, wx):
        rows = sum(v[..., iy[:, j], :] * wy[:, j][:, None] for j in range(iy.shape[1]))
        return sum(rows[..., ix[:, i]] * wx[:, i] for i in range(ix.shape[1]))

    return run(x, wy, wx), run(np.abs(x), np.abs(wy), np.abs(wx))


def bicubic(x, oh: int, ow: int):
    """F.interpolate(x [..., H, W], (oh, ow), mode="bicubic", align_corners=False) -> (value, cond)."""
    return _separable(x, cubic_taps(oh, np.shape(x)[-2]), cubic_taps(ow, np.shape(x)[-1]))


def bilinear(x, oh: int, ow: int):
    """post_reference.resize and its conditioning (the weights are non-negative: the resize of |x|)."""
    return resize(x, oh, ow), resize(np.abs(np.asarray(x, np.float64)), oh, ow)


def nearest_index(out_size: int, in_size: int) -> np.ndarray:
    """F.interpolate's nearest mode: floor(dst * float32(in / out)), in fp32 (nearest_neighbor_compute_source_index)."""
    scale = _F(in_size) / _F(out_size)
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)


# ---- feature extractor -----------------------------------------------------------------------------------------------------------------------------
def crop_extract(img, boxes, S: int) -> np.ndarray:
    """img [B, C, H, W], boxes [K, 2] (y1, x1) -> [B * K, C, S, S]: the windows themselves."""
    img = np.asarray(img, np.float64)
    return np.stack([img[b, :, y:y + S, x:x + S] for b in range(img.shape[0]) for y, x in boxes])


def crop_resize_bicubic(img, boxes, s: int, S: int):
    """windows of s x s resized to S x S: the resize sees the CROPPED tensor, so its clamped taps stay inside the window."""
    return bicubic(crop_extract(img, boxes, s), S, S)


def clip_resize_geometry(H: int, W: int, S: int):
    """(nh, nw, top, left): torchvision's Resize of the short side to S (the long side truncated) and center_crop's int(round(margin / 2.0)) -
    Python's round, halves to even."""
    nh, nw = (S, int(S * W / H)) if H <= W else (int(S * H / W), S)
    return nh, nw, int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))


def _normalize_nhwc(v, cond):
    v = (np.moveaxis(v, 1, -1) - CLIP_MEAN) / CLIP_STD
    cond = (np.moveaxis(cond, 1, -1) + CLIP_MEAN) / CLIP_STD
    return v, cond


def clip_preprocess(img, S: int):
    """img [N, 3, H, W] in [0, 1] -> ([N, S, S, 3] normalised, cond)."""
    img = np.asarray(img, np.float64)
    H, W = img.shape[-2:]
    nh, nw, top, left = clip_resize_geometry(H, W, S)
    v, c = (img, np.abs(img)) if (nh, nw) == (H, W) else bicubic(img, nh, nw)
    return _normalize_nhwc(v[:, :, top:top + S, left:left + S], c[:, :, top:top + S, left:left + S])


def resize_bilinear_norm(img, S: int):
    """F.interpolate(img, (S, S), mode="bilinear", align_corners=False), normalised -> ([N, S, S, 3], cond)."""
    return _normalize_nhwc(*bilinear(img, S, S))


def upsample_nearest(x, oh: int, ow: int) -> np.ndarray:
    """x [N, H, W, C] -> [N, oh, ow, C]."""
    x = np.asarray(x)
    return x[:, nearest_index(oh, x.shape[1])][:, :, nearest_index(ow, x.shape[2])]


def stitch(feat, boxes, OH: int, OW: int):
    """feat [B, K, ch, cw, C], boxes [K, 2] in feature pixels -> (sum of the windows / count_mat [B, OH, OW, C], cond, count [OH, OW]);
    the kernel's convention for a pixel no window covers is 0."""
    feat = np.asarray(feat, np.float64)
    B, K, ch, cw, C = feat.shape
    acc, cond, cnt = np.zeros((B, OH, OW, C)), np.zeros((B, OH, OW, C)), np.zeros((OH, OW))
    for k, (y, x) in enumerate(boxes):
        acc[:, y:y + ch, x:x + cw] += feat[:, k]
        cond[:, y:y + ch, x:x + cw] += np.abs(feat[:, k])
        cnt[y:y + ch, x:x + cw] += 1
    div = np.where(cnt > 0, cnt, 1.0)[None, :, :, None]
    return acc / div, cond / div, cnt.astype(np.int64)


# ---- pixel decoder / transformer decoder ---------------------------------------------------------------------------------------------------------
def add_vec_table(x, vec=None, table=None):
    """x [N, P, C] + vec [C] + table [P, C]."""
    x = np.asarray(x, np.float64)
    v = 0.0 if vec is None else np.asarray(vec, np.float64)
    t = 0.0 if table is None else np.asarray(table, np.float64)
    return x + v + t, np.abs(x) + np.abs(v) + np.abs(t)


def bilinear_add(a, b, oh: int, ow: int):
    """a [N, oh, ow, C] (or None) + bilinear(b [N, H, W, C] -> oh x ow)."""
    v, c = bilinear(np.moveaxis(np.asarray(b, np.float64), -1, 1), oh, ow)
    v, c = np.moveaxis(v, 1, -1), np.moveaxis(c, 1, -1)
    if a is not None:
        v, c = v + np.asarray(a, np.float64), c + np.abs(np.asarray(a, np.float64))
    return v, c


UNDECIDED = 1e-3   # a thresholded element whose float64 logit is closer to zero than this may take either value


def mask_binarize(logits):
    """logits [rows, HW] -> (m01 = sigmoid > 0.5 <=> logit > 0, inv = 1 / (sum m01 + 1e-8), undecided [rows, HW])."""
    v = np.asarray(logits, np.float64)
    m = v > 0
    return m.astype(np.float64), 1.0 / (m.sum(-1) + 1e-8), np.abs(v) < UNDECIDED


def attn_mask(logits, oh: int, ow: int, ldm: int):
    """logits [rows, H, W] -> out [rows, ldm] u8: 1 where sigmoid(resized logit) < 0.5 <=> logit < 0, a row that masks every key cleared, the
    columns past oh * ow 1; undecided [rows, oh * ow]; fragile [rows]: the all-masked rule of the row hangs on an undecided element."""
    v = np.asarray(logits, np.float64)
    if v.shape[-2:] != (oh, ow):
        v = resize(v, oh, ow)
    v = v.reshape(v.shape[0], -1)
    m = v < 0
    und = np.abs(v) < UNDECIDED
    fragile = (m | und).all(-1) & und.any(-1)
    m = m & ~m.all(-1, keepdims=True)
    out = np.ones((v.shape[0], ldm), np.uint8)
    out[:, :oh * ow] = m
    return out, und, fragile


def msda_prepare(off, aw, hs, ws, M: int):
    """off [B, Lq, M, L, P, 2], aw [B, Lq, M, L * P] -> (loc [B, Lq, M, L, P, 2], w [B, Lq, M, L, P], cond of loc): the reference point of query
    q is the centre of its own cell at its own level (valid ratios 1), loc = ref + off / (W_l, H_l), w = softmax over levels * points."""
    off, aw = np.asarray(off, np.float64), np.asarray(aw, np.float64)
    L, P = off.shape[3], off.shape[4]
    ref = np.concatenate([np.stack(np.meshgrid((np.arange(w_) + 0.5) / w_, (np.arange(h_) + 0.5) / h_), -1).reshape(-1, 2)
                          for h_, w_ in zip(hs, ws)])                                      # [Lq, 2] (x, y), row-major cells
    norm = np.array([[w_, h_] for h_, w_ in zip(hs, ws)], np.float64)[None, None, None, :, None, :]
    r = ref[None, :, None, None, None, :]
    return r + off / norm, softmax_rows(aw).reshape(aw.shape[:3] + (L, P)), np.abs(r) + np.abs(off / norm)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------
def softmax_rows(x, scale=1.0) -> np.ndarray:
    z = np.asarray(x, np.float64) * np.float64(_F(scale))
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def l2_normalize(x):
    """F.normalize(x, dim=-1): x / max(||x||, 1e-12) -> (value, cond = |value|)."""
    x = np.asarray(x, np.float64)
    v = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-12)
    return v, np.abs(v)


def clip_assemble(patches, cls, pos, extra: int, TP: int):
    """patches [B, T - 1, Cw], cls [Cw], pos [T, Cw] -> [B, TP, Cw]: cat([cls, patches]) + pos, then `extra` copies of the class token row
    (cls + pos[0]), then zero rows."""
    p, c, e = np.asarray(patches, np.float64), np.asarray(cls, np.float64), np.asarray(pos, np.float64)
    B, T = p.shape[0], p.shape[1] + 1
    tok = np.concatenate([np.broadcast_to(c, (B, 1, c.size)), p], 1)
    out, cond = np.zeros((B, TP, c.size)), np.zeros((B, TP, c.size))
    out[:, :T], cond[:, :T] = tok + e, np.abs(tok) + np.abs(e)
    out[:, T:T + extra], cond[:, T:T + extra] = out[:, :1], cond[:, :1]
    return out, cond


def cond_fold(uncond, gate, pos):
    """The per-model constants the kernel is handed: uncond + gate * (proj + pos) = A1 + A2 * proj."""
    u, g, p = (np.asarray(v, np.float64) for v in (uncond, gate, pos))
    return u + g * p, np.broadcast_to(g, u.shape).copy()


def cond_inputs(uncond, gate, pos, proj):
    """uncond [T, Cw] + gate * (proj [B, 1, Cw] + pos [T, Cw]) with gate = tanh(alpha_cond) -> ([B, T, Cw], cond)."""
    u, g, p, x = (np.asarray(v, np.float64) for v in (uncond, gate, pos, proj))
    x = x[:, None, :]
    return u + g * (x + p), np.abs(u) + np.abs(g) * (np.abs(x) + np.abs(p))


def latent_heads(h, noise, wq, bq, wp, bp, scale, qa, qb):
    """h [B, P, 8] (the VAE encoder's conv_out), noise [4, P] -> dict of (value, cond): latent [B, 4, P] = scale * quant_conv(h)[mean],
    xt [B, P, 4] = qa * latent + qb * noise (q_sample with the shared noise), zdec [B, P, 4] = post_quant_conv(latent / scale)."""
    h, noise, wq, bq, wp, bp = (np.asarray(v, np.float64) for v in (h, noise, wq, bq, wp, bp))
    scale, qa, qb = (np.float64(_F(v)) for v in (scale, qa, qb))
    mean, mean_c = h @ wq.T + bq, np.abs(h) @ np.abs(wq).T + np.abs(bq)            # [B, P, 4]
    lat, lat_c = scale * mean, abs(scale) * mean_c
    xt, xt_c = qa * lat + qb * noise.T, abs(qa) * lat_c + abs(qb) * np.abs(noise.T)
    z, z_c = (lat / scale) @ wp.T + bp, mean_c @ np.abs(wp).T + np.abs(bp)
    return {"latent": (np.moveaxis(lat, 1, 2), np.moveaxis(lat_c, 1, 2)), "xt": (xt, xt_c), "zdec": (z, z_c)}


def classify_rows(L1, L2, seg, ovl, ls1, ls2, alpha, beta, binary=None) -> np.ndarray:
    """L1 [rows, Ktot + 1] cosines against the category text bank, null text last; L2 [rows, Ktot] against MaskCLIP's; seg [K + 1] offsets of
    the synonym groups; ovl [K] 1 = category seen in training -> [rows, K + 1] log-probabilities."""
    L1, L2 = np.asarray(L1, np.float64), np.asarray(L2, np.float64)
    ls1, ls2, alpha, beta = (np.float64(_F(v)) for v in (ls1, ls2, alpha, beta))
    K = len(seg) - 1
    a = np.stack([L1[:, seg[k]:seg[k + 1]].max(-1) for k in range(K)], -1) * ls1     # ensemble_logits_with_labels, "max"
    b = np.stack([L2[:, seg[k]:seg[k + 1]].max(-1) for k in range(K)], -1) * ls2
    p, q = softmax_rows(a), softmax_rows(b)
    w = np.where(np.asarray(ovl) != 0, alpha, beta)
    with np.errstate(divide="ignore"):
        open_logits = np.log(p ** (1.0 - w) * q ** w)                                  # base + novel: each category is in exactly one
    if binary is None:
        pn = softmax_rows(np.concatenate([a, L1[:, -1:] * ls1], -1))[:, -1]           # odise.py:312
    else:
        pn = softmax_rows(np.asarray(binary, np.float64))[:, 1]
    probs = np.concatenate([softmax_rows(open_logits) * (1.0 - pn)[:, None], pn[:, None]], -1)
    return np.log(probs + 1e-8)
