"""Hand-worked pictures for the LVIS specification (odise_amd/lvis_eval.py), each built to separate one clause of it; shared by
tests/test_lvis_eval_cpu.py and the GPU tests.  Categories are their own contiguous ids."""
import json
import os

import numpy as np

from odise_amd import coco_rle
from odise_amd import lvis_eval as LE


def rect(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def ann(mask, cat, **extra):
    """An LVIS annotation of a mask: compressed RLE, `area` = its pixels unless given."""
    a = {"category_id": int(cat), "area": float(np.count_nonzero(mask)), "segmentation": coco_rle.encode(mask)}
    a.update(extra)
    return a


def rows_of(dets, anns, K, neg=(), nex=(), image=0):
    """dets: [(mask, score, category)] -> lvis_eval.image_rows of the picture (rows, flags) and its gt table."""
    ident = {k: k for k in range(K)}
    h, w = (dets[0][0] if dets else LE.IE.decode_runs(LE.IE.annotation_counts(anns[0]["segmentation"]), *anns[0]["segmentation"]["size"])).shape
    table = LE.gt_rows(anns, ident)[0]
    masks = np.stack([d[0] for d in dets]) if dets else np.zeros((0, h, w), np.uint8)
    counts = [LE.IE.annotation_counts(a["segmentation"]) for a in anns]
    rows, flags = LE.image_rows(masks, [d[1] for d in dets], [d[2] for d in dets], counts, table, neg, nex, image, num_categories=K)
    return rows, flags, table


def bits(word, a):
    """The ten threshold bits of range a of a matched / ignored word."""
    return (int(word) >> (10 * a)) & 0x3FF


ALL40 = (1 << 40) - 1


def three_pictures():
    """A dataset of three pictures over four categories (ids 10, 20, 30, 40; frequencies f, c, r, r) -> (gt dict, results list).
    picture 1: an object of 10 found exactly, a detection of 20 that is in neither list (dropped) and one of 30 that is in neg (a false
               positive of 30, which has its object in picture 2).
    picture 2: an object of 30 given as a polygon and found at a lower score than picture 1's false positive; an object of 20 found.
    picture 3: no detections; an object of 10 that is missed; 40 not exhaustive, no ground truth anywhere (every cell -1)."""
    h, w = 40, 50
    images = [{"id": 1, "height": h, "width": w, "neg_category_ids": [30], "not_exhaustive_category_ids": []},
              {"id": 2, "height": h, "width": w, "neg_category_ids": [], "not_exhaustive_category_ids": [20]},
              {"id": 3, "height": h, "width": w, "neg_category_ids": [20], "not_exhaustive_category_ids": [40]}]
    cats = [{"id": 10, "name": "ten", "frequency": "f"}, {"id": 20, "name": "twenty", "frequency": "c"},
            {"id": 30, "name": "thirty", "frequency": "r"}, {"id": 40, "name": "forty", "frequency": "r"}]
    a, b, c, d = rect(h, w, 2, 12, 3, 13), rect(h, w, 20, 30, 20, 40), rect(h, w, 5, 25, 5, 25), rect(h, w, 0, 8, 30, 45)
    poly = [[5.0, 5.0, 25.0, 5.0, 25.0, 25.0, 5.0, 25.0]]
    anns = [dict(ann(a, 10), id=1, image_id=1), {"id": 2, "image_id": 2, "category_id": 30, "area": 400.0, "segmentation": poly},
            dict(ann(d, 20), id=3, image_id=2), dict(ann(b, 10), id=4, image_id=3)]
    det = lambda img, m, cat, s: {"image_id": img, "category_id": cat, "score": s, "segmentation": coco_rle.encode(m)}
    res = [det(1, a, 10, .9), det(1, b, 20, .8), det(1, b, 30, .7), det(2, c, 30, .6), det(2, d, 20, .5)]
    return {"images": images, "categories": cats, "annotations": anns}, res


def write_pair(tmp_path):
    gt, res = three_pictures()
    rp, gp = os.path.join(str(tmp_path), "lvis_results.json"), os.path.join(str(tmp_path), "lvis_gt.json")
    with open(rp, "w") as f:
        json.dump(res, f)
    with open(gp, "w") as f:
        json.dump(gt, f)
    return rp, gp
