"""COCO compressed RLE on the host (numpy): pycocotools' `mask.encode` / `decode` / `area` restated from maskApi.c, and detectron2's
`instances_to_coco_json` for this package's instance results.

The string format (maskApi.c rleToString): runs are taken over the column-major flattening j = x * h + y and continue across columns;
cnts[0] counts the leading zeros (0 when the mask starts with a one), the counts then alternate between runs of ones and zeros.  Count i
is written as x = cnts[i] - cnts[i-2] (only for i > 2), five bits per character from the low end, bit 0x20 set while more characters
follow, plus 48.  `odise_hip_rle_encode` / `odise_hip_instance_rle` produce the same bytes on the device; this module is the host
fallback for host masks and the reference of the tests.
"""
from __future__ import annotations

import numpy as np


def mask_counts(mask) -> np.ndarray:
    """Run lengths (int64) of a 2-D mask (any nonzero value is 1) over the column-major order, starting with the zeros."""
    m = np.asarray(mask)
    assert m.ndim == 2, m.shape
    flat = (m != 0).ravel(order="F").astype(np.int8)
    edges = np.flatnonzero(np.diff(flat, prepend=np.int8(0)))          # pixel j differs from pixel j - 1 (pixel -1 = 0)
    return np.diff(np.concatenate(([0], edges, [flat.size]))).astype(np.int64)


def counts_to_string(cnts) -> str:
    """maskApi.c rleToString."""
    out = []
    cnts = [int(c) for c in cnts]
    for i, c in enumerate(cnts):
        x = c - cnts[i - 2] if i > 2 else c
        while True:
            ch = x & 0x1F
            x >>= 5                                                     # arithmetic shift (Python ints)
            more = x != -1 if ch & 0x10 else x != 0
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
            if not more:
                break
    return "".join(out)


def string_to_counts(s: str) -> np.ndarray:
    """maskApi.c rleFrString."""
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.asarray(cnts, np.int64)


def encode(mask) -> dict:
    """pycocotools `mask.encode(np.asfortranarray(mask.astype(np.uint8)))` with the counts decoded to str."""
    m = np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_to_string(mask_counts(m))}


def decode(rle: dict) -> np.ndarray:
    """uint8 [h, w] mask of an RLE dict (counts as str or bytes)."""
    h, w = (int(v) for v in rle["size"])
    s = rle["counts"]
    cnts = string_to_counts(s.decode("utf-8") if isinstance(s, (bytes, bytearray)) else s)
    assert int(cnts.sum()) == h * w, (int(cnts.sum()), h, w)
    vals = (np.arange(cnts.size) & 1).astype(np.uint8)
    return np.repeat(vals, cnts).reshape((h, w), order="F")


def area(rle: dict) -> int:
    """Pixels of the mask: the sum of the counts of ones (odd indices)."""
    s = rle["counts"]
    return int(string_to_counts(s.decode("utf-8") if isinstance(s, (bytes, bytearray)) else s)[1::2].sum())


def instances_to_coco_json(instances: dict, img_id, boxes=None) -> list:
    """detectron2.evaluation.coco_evaluation.instances_to_coco_json for one image's "instances" of HipCategoryODISE: records
    {"image_id", "category_id" (contiguous class; the evaluator maps it to the dataset id), "bbox", "score", "segmentation"}.  The
    reference's instance head returns zero boxes (maskformer_model.py:372), which XYXY -> XYWH keeps zero.  Takes the default result
    (`pred_masks` [n, h, w]: host array, torch tensor, or device array, which is encoded on its device) or the `instance_rle` result
    (`pred_masks_rle`: the strings are already there).  boxes: XYXY [n, 4] (HipCategoryODISE.instance_boxes -> "pred_boxes",
    `Context.instance_boxes`), written as XYWH floats the way BoxMode.convert(XYXY_ABS, XYWH_ABS) does; without them the zeros stay."""
    scores = np.asarray(instances["scores"], np.float32)
    classes = np.asarray(instances["pred_classes"])
    n = len(scores)
    if n == 0:
        return []
    if "pred_masks_rle" in instances:
        rles = list(instances["pred_masks_rle"])
    else:
        masks = instances["pred_masks"]
        if hasattr(masks, "ctx") and hasattr(masks, "ptr"):            # runtime.DeviceArray: encode where it lives
            rles, _ = masks.ctx.rle_encode(masks)
        else:
            if hasattr(masks, "detach"):
                masks = masks.detach().cpu().numpy()
            rles = [encode(m) for m in np.asarray(masks)]
    assert len(rles) == n, (len(rles), n)
    if boxes is None:
        xywh = [[0.0, 0.0, 0.0, 0.0]] * n
    else:
        b = np.asarray(boxes, np.float64).reshape(-1, 4)
        assert len(b) == n, (len(b), n)
        xywh = [[float(x0), float(y0), float(x1 - x0), float(y1 - y0)] for x0, y0, x1, y1 in b]
    return [{"image_id": img_id, "category_id": int(classes[k]), "bbox": list(xywh[k]), "score": float(scores[k]),
             "segmentation": rles[k]} for k in range(n)]
