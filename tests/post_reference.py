"""Float64 numpy restatement of the post-processing stage (odise.py:326-331, maskformer_model.py:280-380), on fp16-rounded mask logits.

It follows oracle/odise_model.py (the fp32 torch restatement) operation by operation, with two things pinned that torch leaves open:
  * the instance head's selection is `np.lexsort((flat_index, -prob))[:topk]` - probability descending, flat index ascending among equal
    probabilities - which is the order the device kernel documents (torch.topk leaves ties unspecified);
  * arg-max means numpy's documented first maximum.
The bilinear tap positions (source index and weight of every output row / column) are part of the operation's definition, and torch
computes them in fp32 for fp32 tensors (`area_pixel_compute_source_index<float>`): they are taken in fp32 here too and widened; every
interpolated VALUE, the softmax, the sigmoid and all sums are float64.

Besides the outputs the functions return the margins the tests' tolerance rules need: the top-2 relative margin of score * sigmoid per
pixel, |logit| per pixel and query, the top-2 gap of the semantic scores, the distance of every class probability to the k-th one.
"""
import numpy as np

MAX_SEGMENTS = 100


def f16_round(x) -> np.ndarray:
    """fp32 -> fp16 (round to nearest even, as the device cast) -> float64."""
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def taps(out_size: int, in_size: int):
    """(i0, i1, t) of every output index: torch's align_corners=False source index, in fp32."""
    o = np.arange(out_size, dtype=np.float32)
    scale = np.float32(in_size) / np.float32(out_size)
    s = (o + np.float32(0.5)) * scale - np.float32(0.5)
    s = np.maximum(s, np.float32(0.0))
    i0 = np.minimum(s.astype(np.int64), in_size - 1)
    i1 = np.where(i0 < in_size - 1, i0 + 1, i0)
    t = (s - i0.astype(np.float32)).astype(np.float64)
    return i0, i1, t


def resize(x: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """F.interpolate(x [..., H, W], (oh, ow), mode="bilinear", align_corners=False) in float64."""
    x = np.asarray(x, np.float64)
    y0, y1, ty = taps(oh, x.shape[-2])
    x0, x1, tx = taps(ow, x.shape[-1])
    rows = x[..., y0, :] * (1.0 - ty)[:, None] + x[..., y1, :] * ty[:, None]
    return rows[..., x0] * (1.0 - tx) + rows[..., x1] * tx


def upsample(logits16, pad_hw, img_hw, out_hw) -> np.ndarray:
    """logits [Q, h4, w4] (already fp16-representable) -> [Q, oh, ow]: resize to the padded size, crop to the image, resize to the output."""
    m = resize(logits16, pad_hw[0], pad_hw[1])[:, :img_hw[0], :img_hw[1]]
    if tuple(out_hw) != tuple(img_hw):
        m = resize(m, out_hw[0], out_hw[1])
    return m


def softmax(mask_cls) -> np.ndarray:
    z = np.asarray(mask_cls, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def sigmoid(v) -> np.ndarray:
    return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def panoptic(mask_cls, mask, K, thing_ids, object_mask_threshold=0.0, overlap_threshold=0.8, max_segments=MAX_SEGMENTS) -> dict:
    """panoptic_inference (maskformer_model.py:286-342) of one image; `mask` [Q, oh, ow] upsampled logits.

    owner [oh, ow]: winning query of the pixel among the kept ones (-1: nothing kept); inside: its sigmoid >= 0.5; counts [3, Q]: mask_area,
    original_area, intersection (zero rows for dropped queries); qmap [Q]: segment id per query; seg: the panoptic map; info: segments_info;
    margin [oh, ow]: (top1 - top2) / top1 of score * sigmoid (inf with fewer than two kept queries).
    The record holds at most `max_segments` rows: a segment past the cap gets no id and consumes none (odise_post_desc)."""
    probs = softmax(mask_cls)
    Q = probs.shape[0]
    scores, labels = probs.max(-1), probs.argmax(-1)
    keep = (labels != K) & (scores > np.float64(np.float32(object_mask_threshold)))
    sig = sigmoid(mask)
    oh, ow = mask.shape[-2:]
    kept = np.flatnonzero(keep)
    out = {"keep": keep, "labels": labels, "scores": scores, "counts": np.zeros((3, Q), np.int64), "qmap": np.zeros(Q, np.int64),
           "seg": np.zeros((oh, ow), np.int32), "info": [], "owner": np.full((oh, ow), -1, np.int64), "inside": np.zeros((oh, ow), bool),
           "margin": np.full((oh, ow), np.inf), "margin_distinct": np.full((oh, ow), np.inf)}
    if kept.size == 0:
        return out
    pm = scores[kept, None, None] * sig[kept]
    first = pm.argmax(0)                                                   # first maximum
    owner = kept[first]
    inside = np.take_along_axis(sig[kept], first[None], 0)[0] >= 0.5
    if kept.size > 1:
        top2 = np.partition(pm, -2, axis=0)[-2:]
        out["margin"] = (top2[1] - top2[0]) / top2[1]
    # the same against the largest value BELOW the maximum: what decides a pixel whose maximum is shared by duplicated queries (bitwise equal on
    # the device too, the first index wins)
    below = np.where(pm < pm.max(0), pm, -np.inf).max(0)
    out["margin_distinct"] = np.where(np.isfinite(below), (pm.max(0) - below) / pm.max(0), np.inf)
    out["owner"], out["inside"] = owner, inside
    out["counts"][0] = np.bincount(owner.ravel(), minlength=Q)
    out["counts"][1, kept] = (sig[kept] >= 0.5).reshape(kept.size, -1).sum(1)
    out["counts"][2] = np.bincount(owner.ravel()[inside.ravel()], minlength=Q)
    thing = set(int(t) for t in thing_ids)
    current, stuff = 0, {}
    for q in kept:
        cls = int(labels[q])
        mask_area, original_area, inter = (int(v) for v in out["counts"][:, q])
        if mask_area > 0 and original_area > 0 and inter > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            if cls not in thing and cls in stuff:
                out["qmap"][q] = stuff[cls]
                continue
            if len(out["info"]) >= max_segments:
                continue
            if cls not in thing:
                stuff[cls] = current + 1
            current += 1
            out["qmap"][q] = current
            out["info"].append({"id": current, "isthing": cls in thing, "category_id": cls})
    out["seg"] = np.where(inside, out["qmap"][owner], 0).astype(np.int32)
    return out


def semantic(mask_cls, mask, K) -> np.ndarray:
    """semantic_inference (maskformer_model.py:280-284): [K, oh, ow]."""
    q, oh, ow = mask.shape
    return (softmax(mask_cls)[:, :K].T @ sigmoid(mask).reshape(q, -1)).reshape(K, oh, ow)        # einsum("qc,qhw->chw")


def semantic_bound(ref, Q) -> np.ndarray:
    """Error bound of the device's semantic score against `ref`: every term is non-negative, so the fp16 roundings of the probability and of
    the sigmoid are relative to the value (2^-11 each, and their product), the fp32 accumulation adds 2^-16 of it at most for Q <= 304 terms,
    and a probability below the fp16 normal range loses at most 2^-24 absolutely, times a sigmoid <= 1, per query."""
    return (2.0 ** -10 + 2.0 ** -16) * ref + Q * 2.0 ** -24


def semantic_decided(sem, Q, twin=None):
    """(first, decided) per pixel: the arg-max over classes, and whether the top-2 gap exceeds twice the device bound.  twin = (a, b): class
    column b repeats column a (a < b), so the two tie exactly and the first wins; b is left out and the gap is taken to the best of the rest."""
    s = np.array(sem, np.float64)
    if twin is not None:
        s[twin[1]] = -np.inf
    top2 = np.partition(s, -2, axis=0)[-2:]
    return s.argmax(0), (top2[1] - top2[0]) > 2 * semantic_bound(top2[1], Q)


def mask_scores(mask) -> np.ndarray:
    """[Q] mean sigmoid over the pixels with logit > 0 (maskformer_model.py:376-377)."""
    pm = mask > 0
    n = mask.shape[0]
    return (sigmoid(mask) * pm).reshape(n, -1).sum(1) / (pm.reshape(n, -1).sum(1) + 1e-6)


def loose_pixels(mask, exact) -> np.ndarray:
    """[Q, oh, ow] pixels whose sign an fp32 interpolation may take differently: none where every interpolated value is exact, else
    |logit| < 8 * 2^-24 * max|logit|."""
    if exact:
        return np.zeros(mask.shape, bool)
    return np.abs(mask) < 8 * 2.0 ** -24 * np.abs(mask).max()


def instance(mask_cls, mask, K, thing_ids, topk=100, panoptic_on=True) -> dict:
    """instance_inference (maskformer_model.py:344-380).  query / cls / prob / score / masks of the n kept entries in selection order;
    kth: the probability of the last selected entry; gap [n]: |prob - kth| / kth of every kept entry; band_count(rel): how many of ALL Q*K
    probabilities lie within rel * kth of kth (the entries whose membership an fp32 softmax may decide differently)."""
    p = softmax(mask_cls)[:, :K].reshape(-1)
    n_sel = min(topk, p.size)
    order = np.lexsort((np.arange(p.size), -p))[:n_sel]
    kth = p[order[-1]]
    q, c = order // K, order % K
    if panoptic_on:
        thing = set(int(t) for t in thing_ids)
        ok = np.array([int(x) in thing for x in c], bool)
        order, q, c = order[ok], q[ok], c[ok]
    pm = mask[q] > 0
    mscore = mask_scores(mask)[q]
    return {"query": q, "cls": c, "prob": p[order], "score": p[order] * mscore, "masks": pm, "kth": kth, "gap": np.abs(p[order] - kth) / kth,
            "band_count": lambda rel: int((np.abs(p - kth) <= rel * kth).sum()), "n_selected": n_sel}


def inst_stats(mask):
    """(sum, count) per query as the device accumulates them: over the pixels with logit > 0, the fp16-rounded sigmoid (never below 0.5: a tiny positive logit rounds
    there) in whole units of 2^-11 (exact integers), and their count.
    fragile: pixels whose float64 sigmoid lies within 4 fp32 ulps of an fp16 rounding boundary (the device evaluates the sigmoid in fp32
    with a 1-ulp exp and a 1-ulp reciprocal, so only those may round differently)."""
    m = np.asarray(mask, np.float64)
    pos = m > 0
    s = sigmoid(m)
    h = s.astype(np.float16)
    h = np.where(pos, np.maximum(h, np.float16(0.5)), h)
    units = np.where(pos, np.round(h.astype(np.float64) * 2048.0), 0.0).astype(np.int64)
    n = m.shape[0]
    ulp16 = np.spacing(s.astype(np.float16)).astype(np.float64)
    h64 = s.astype(np.float16).astype(np.float64)
    dist = np.minimum(np.abs(s - (h64 + ulp16 / 2)), np.abs(s - (h64 - ulp16 / 2)))
    fragile = pos & (dist <= 4 * np.spacing(s.astype(np.float32)).astype(np.float64))
    return units.reshape(n, -1).sum(1), pos.reshape(n, -1).sum(1), int(fragile.sum())


def postprocess(mask_cls, logits16, pad_hw, img_hw, out_hw, K, thing_ids, object_mask_threshold=0.0, overlap_threshold=0.8, topk=100,
                panoptic_on=True) -> dict:
    """One image through all three heads.  mask_cls [Q, K+1] fp32 log-probabilities, logits16 [Q, h4, w4] fp16-representable."""
    mask = upsample(logits16, pad_hw, img_hw, out_hw)
    return {"mask": mask, "sem": semantic(mask_cls, mask, K),
            "pan": panoptic(mask_cls, mask, K, thing_ids, object_mask_threshold, overlap_threshold),
            "inst": instance(mask_cls, mask, K, thing_ids, topk, panoptic_on)}
