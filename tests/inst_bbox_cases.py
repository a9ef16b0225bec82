"""Crafted inputs of the bbox tests (tests/test_instance_bbox_cpu.py, tests/test_gpu_instance_bbox.py) on top of tests/inst_cases.py:
annotations with their `bbox`, the literal detectron2 formulation of BitMasks.get_bounding_boxes, and the picture on which bbox and segm
matching part ways."""
import numpy as np
import torch

import inst_cases as IC
from odise_amd import instance_eval as IE


def torch_boxes(masks) -> np.ndarray:
    """detectron2.structures.BitMasks.get_bounding_boxes as it is written there (torch.any over a dimension, torch.where)."""
    t = torch.from_numpy(np.asarray(masks) != 0)
    boxes = torch.zeros(t.shape[0], 4, dtype=torch.float32)
    x_any, y_any = torch.any(t, dim=1), torch.any(t, dim=2)
    for idx in range(t.shape[0]):
        x, y = torch.where(x_any[idx, :])[0], torch.where(y_any[idx, :])[0]
        if len(x) > 0 and len(y) > 0:
            boxes[idx, :] = torch.as_tensor([x[0], y[0], x[-1] + 1, y[-1] + 1], dtype=torch.float32)
    return boxes.numpy()


def ann_mask(a) -> np.ndarray:
    h, w = a["segmentation"]["size"]
    return IE.decode_runs(IE.annotation_counts(a["segmentation"]), h, w)


def with_bbox(anns, jitter=None):
    """The annotations with `bbox` = the XYWH box of their mask; jitter (a Generator) moves every member by a fraction of a pixel, as the
    boxes of COCO's polygon annotations lie."""
    out = []
    for a in anns:
        b = IE.xyxy_to_xywh(IE.mask_boxes(ann_mask(a)[None]))[0]
        if jitter is not None:
            b = b + np.round(jitter.random(4) * 16) / 16
        out.append(dict(a, bbox=[float(v) for v in b]))
    return out


def bbox_case(c, jitter=None):
    return dict(c, annotations=with_bbox(c["annotations"], jitter))


def ell_case():
    """Two L-shaped detections with ONE box, [10, 10, 30, 30]: the lower-left L (score .8) is the ground truth's own mask, the upper-right L
    (score .9) shares its two 4 x 4 corners with it, 32 pixels of 144.  segm: the first detection misses (32 / 256), the second matches at every
    threshold.  bbox: both boxes are the ground truth's; the first detection takes it, the second finds it taken."""
    lower = IC.rect(10, 30, 10, 14) | IC.rect(26, 30, 10, 30)
    upper = IC.rect(10, 14, 10, 30) | IC.rect(10, 30, 26, 30)
    return bbox_case(IC.case([upper, lower], [.9, .8], [0, 0], [IC.ann(lower)]))


def want_rows(c, image, topk, iou_type="bbox"):
    """-> (rows [topk] padded with zeros, n, flags, gt_rows' tuple, gt boxes) of the host loop"""
    gt = IE.gt_rows(c["annotations"], {k: k for k in range(c["K"])})
    table, runs, offs = gt
    counts = [runs[offs[i]:offs[i + 1]] for i in range(len(table))]
    boxes = IE.gt_boxes(c["annotations"])
    rows, flags = IE.image_rows(c["masks"], c["scores"], c["classes"], counts, table, image, num_categories=c["K"], iou_type=iou_type, gt_boxes=boxes)
    full = np.zeros(topk, IE.ROW_DTYPE)
    full[:len(rows)] = rows
    return full, len(rows), flags, gt, boxes
