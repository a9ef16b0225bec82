"""SemSegEvaluator (odise/evaluation/d2_evaluator.py:64 over detectron2's SemSegEvaluator) on the device, and its host restatement.

`HipSemSegEvaluator.process` enqueues one `odise_hip_semantic_eval` per picture on the prediction as it lies in HBM - the int32 label map
of the fused arg-max, or the score tensor - which adds to the two confusion matrices and writes the per-class RLE strings, and settles
the picture (a retry reads the prediction again) before the model may overwrite that buffer; `evaluate` reads the strings, sums the matrices across ranks and does the arithmetic below on the host.  detectron2 is not a dependency of this
package, so the rules are restated here and this module is their specification.  With `pq=True` the per-picture call is
`odise_hip_semantic_eval_pq`, which also counts the PQ-for-semantic-segmentation statistics (odise_amd/semseg_pq.py: their specification)
from the same label map, and `evaluate` appends PQ / SQ / RQ and PQ-<name> per class behind the keys below:

process(inputs, outputs), per picture
    pred = output["sem_seg"].argmax(dim=0) as int; gt = the annotation as int, gt[gt == ignore_label] = num_classes
    conf_matrix   += bincount((num_classes + 1) * pred + gt, minlength=(num_classes + 1)^2)      rows = prediction
    b_conf_matrix += the same of (_mask_to_boundary(pred), _mask_to_boundary(gt))                 (num_classes < 255; sem_boundary.py)
    predictions.extend(encode_json_sem_seg(pred, input["file_name"]))

encode_json_sem_seg(sem_seg, input_file_name)
    for label in np.unique(sem_seg):
        dataset_id = contiguous_id_to_dataset_id[label] when the dataset has such a mapping (the label must be in it), else int(label)
        mask_rle = mask_util.encode(np.array((sem_seg == label)[:, :, None], order="F", dtype=uint8))[0], counts decoded to str
        {"file_name": input_file_name, "category_id": dataset_id, "segmentation": mask_rle}

evaluate()
    the matrices of all ranks are summed, the prediction rows of all ranks concatenated in rank order -> sem_seg_predictions.json
    tp = conf.diagonal()[:-1]; pos_gt = sum(conf[:-1, :-1], axis=0); pos_pred = sum(conf[:-1, :-1], axis=1)
    acc   valid where pos_gt > 0:               tp / pos_gt
    iou   valid where pos_gt > 0 and union > 0: tp / union,  union = pos_gt + pos_pred - tp
    mACC = mean(acc over acc_valid); mIoU = mean(iou over iou_valid); fwIoU = sum(iou * pos_gt / sum(pos_gt) over iou_valid)
    pACC = sum(tp) / sum(pos_gt)
    with the boundary matrix: b_iou = b_tp / b_union where b_union > 0, from b_conf the same way
    res: mIoU, fwIoU, then per class IoU-<name> (followed by BoundaryIoU-<name> and min(IoU, B-Iou)-<name>), mACC, pACC, ACC-<name>;
         everything times 100, an invalid entry is NaN
    ODISE's wrapper returns {f"{dataset_name}/{prefix}sem_seg": res}, the prefix with a "_" appended when it has none.
"""
from __future__ import annotations

import json
import os
from collections import OrderedDict
from typing import Dict, Optional, Sequence

import numpy as np

from . import coco_rle
from . import sem_boundary as SB

FLAG_NAMES = {1: "a predicted label outside [0, num_classes)"}


def flag_names(flags: int) -> list:
    return [name for bit, name in FLAG_NAMES.items() if flags & bit]


def dataset_id(label: int, contiguous_id_to_dataset_id: Optional[Dict[int, int]]) -> int:
    if contiguous_id_to_dataset_id is None:
        return int(label)
    assert int(label) in contiguous_id_to_dataset_id, f"Label {int(label)} is not in the metadata info"
    return int(contiguous_id_to_dataset_id[int(label)])


def encode_json_sem_seg(labels, file_name, contiguous_id_to_dataset_id: Optional[Dict[int, int]] = None) -> list:
    """The literal restatement: one row per label of np.unique(labels), ascending."""
    labels = np.asarray(labels)
    assert labels.ndim == 2, labels.shape
    rows = []
    for label in np.unique(labels):
        did = dataset_id(label, contiguous_id_to_dataset_id)
        rows.append({"file_name": file_name, "category_id": did, "segmentation": coco_rle.encode((labels == label).astype(np.uint8))})
    return rows


def rows_from_rle(classes, rles, file_name, contiguous_id_to_dataset_id: Optional[Dict[int, int]] = None) -> list:
    """The same rows from what `Context.semantic_eval` returns (classes ascending, their RLE dicts)."""
    return [{"file_name": file_name, "category_id": dataset_id(c, contiguous_id_to_dataset_id), "segmentation": r} for c, r in zip(classes, rles)]


def confusion(pred, gt, K: int) -> np.ndarray:
    """int64 [(K+1), (K+1)], rows = prediction: what one picture adds to conf_matrix.  pred in [0, K); gt outside [0, K] counts as K."""
    n = K + 1
    g = SB.clamp_labels(gt, K).astype(np.int64)
    return np.bincount((n * np.asarray(pred).astype(np.int64) + g).reshape(-1), minlength=n * n).reshape(n, n).astype(np.int64)


def _iou_parts(conf):
    conf = np.asarray(conf, np.int64)
    tp = conf.diagonal()[:-1].astype(np.float64)
    pos_gt = conf[:-1, :-1].sum(axis=0).astype(np.float64)
    pos_pred = conf[:-1, :-1].sum(axis=1).astype(np.float64)
    return tp, pos_gt, pos_pred


def results(conf, b_conf, class_names: Sequence[str]) -> "OrderedDict[str, float]":
    """The arithmetic of SemSegEvaluator.evaluate on the summed matrices (b_conf None: no Boundary IoU rows)."""
    K = len(class_names)
    assert np.asarray(conf).shape == (K + 1, K + 1), (np.asarray(conf).shape, K)
    acc = np.full(K, np.nan)
    iou = np.full(K, np.nan)
    tp, pos_gt, pos_pred = _iou_parts(conf)
    with np.errstate(divide="ignore", invalid="ignore"):
        class_weights = pos_gt / np.sum(pos_gt)
        acc_valid = pos_gt > 0
        acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
        union = pos_gt + pos_pred - tp
        iou_valid = np.logical_and(acc_valid, union > 0)
        iou[iou_valid] = tp[iou_valid] / union[iou_valid]
        macc = np.sum(acc[acc_valid]) / np.sum(acc_valid)
        miou = np.sum(iou[iou_valid]) / np.sum(iou_valid)
        fiou = np.sum(iou[iou_valid] * class_weights[iou_valid])
        pacc = np.sum(tp) / np.sum(pos_gt)
        if b_conf is not None:
            assert np.asarray(b_conf).shape == (K + 1, K + 1)
            b_iou = np.full(K, np.nan)
            b_tp, b_pos_gt, b_pos_pred = _iou_parts(b_conf)
            b_union = b_pos_gt + b_pos_pred - b_tp
            b_iou_valid = b_union > 0
            b_iou[b_iou_valid] = b_tp[b_iou_valid] / b_union[b_iou_valid]
    res = OrderedDict()
    res["mIoU"] = 100 * float(miou)
    res["fwIoU"] = 100 * float(fiou)
    for i, name in enumerate(class_names):
        res[f"IoU-{name}"] = 100 * float(iou[i])
        if b_conf is not None:
            res[f"BoundaryIoU-{name}"] = 100 * float(b_iou[i])
            res[f"min(IoU, B-Iou)-{name}"] = 100 * float(min(iou[i], b_iou[i]))
    res["mACC"] = 100 * float(macc)
    res["pACC"] = 100 * float(pacc)
    for i, name in enumerate(class_names):
        res[f"ACC-{name}"] = 100 * float(acc[i])
    return res


def result_key(dataset_name: str, prefix: str = "") -> str:
    if len(prefix) and not prefix.endswith("_"):
        prefix += "_"
    return f"{dataset_name}/{prefix}sem_seg"


def gather(conf: np.ndarray, b_conf: Optional[np.ndarray], rows: list, flags: int):
    """The exchange step of evaluate(): the matrices summed (`distributed.sum_confusion`, one all-reduce for both), the rows of all ranks
    in rank order, the flags OR-ed.  One process: the arguments as they are."""
    import torch
    import torch.distributed as dist

    from . import distributed as D
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return conf, b_conf, rows, int(flags)
    both = np.stack([conf] + ([b_conf] if b_conf is not None else [])).astype(np.int64)
    both = D.sum_confusion(torch.from_numpy(both)).numpy()
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, (rows, int(flags)))
    all_rows, seen = [], 0
    for r, f in parts:
        all_rows += r
        seen |= int(f)
    return both[0], (both[1] if b_conf is not None else None), all_rows, seen


def _rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class HipSemSegEvaluator:
    def __init__(self, ctx, class_names: Sequence[str], ignore_label: int, dataset_name: str, prefix: str = "",
                 contiguous_id_to_dataset_id: Optional[Dict[int, int]] = None, compute_boundary_iou: Optional[bool] = None, pq: bool = False):
        """class_names [K] (metadata.stuff_classes), ignore_label (metadata.ignore_label), contiguous_id_to_dataset_id
        (metadata.stuff_dataset_id_to_contiguous_id reversed, when the dataset has it); compute_boundary_iou None = K < 255, as the
        reference decides when OpenCV is importable.  pq: also count the PQ-for-semantic-segmentation statistics (semseg_pq.py) in the
        same call per picture; `evaluate` then appends PQ, SQ, RQ and PQ-<name> per class and keeps `self.pq_stats`."""
        self.ctx = ctx
        self.class_names = list(class_names)
        self.K = len(self.class_names)
        self.ignore_label, self.dataset_name, self.prefix = int(ignore_label), dataset_name, prefix
        self.to_dataset = None if contiguous_id_to_dataset_id is None else {int(k): int(v) for k, v in contiguous_id_to_dataset_id.items()}
        self.boundary = self.K <= SB.MAX_CLASSES if compute_boundary_iou is None else bool(compute_boundary_iou)
        assert not self.boundary or self.K <= SB.MAX_CLASSES, f"Boundary IoU needs at most {SB.MAX_CLASSES} classes"
        n = (self.K + 1) ** 2
        # one buffer, one copy in evaluate(): conf | b_conf | a word whose first int32 holds the flags
        self._buf = ctx.empty((2 * n + 1,), np.int64)
        self.conf = self._buf.view((self.K + 1, self.K + 1), np.int64)
        self.b_conf = self._buf.view((self.K + 1, self.K + 1), np.int64, 8 * n) if self.boundary else None
        self.flags = self._buf.view((1,), np.int32, 16 * n)
        self.pq = bool(pq)
        if self.pq:
            from .panoptic_quality import STAT_DTYPE
            self.stats = ctx.empty((self.K,), STAT_DTYPE)                   # a buffer of its own: the one above stays as it is
        self.reset()

    def reset(self) -> None:
        from ._lib import check
        check(self.ctx.lib.odise_hip_memset(self.ctx.h, self._buf.ptr, 0, self._buf.nbytes), "memset")
        if self.pq:
            check(self.ctx.lib.odise_hip_memset(self.ctx.h, self.stats.ptr, 0, self.stats.nbytes), "memset")
        self._pending = []

    def process(self, pred, gt, file_name, pred_kept: bool = False) -> None:
        """One picture.  pred: a device label map int32 [H,W] (the fused arg-max, "sem_seg_argmax" of HipCategoryODISE) or a device score
        tensor float32 [K,H,W] ("sem_seg").  gt: the annotation [H,W]; a HOST array gets gt == ignore_label mapped to K here and goes up
        in an upload that WAITS for the stream (the convenience of HipPanopticEvaluator.process); a DeviceArray must ALREADY be int32 with
        the ignore label mapped to K (any value outside [0,K] counts as K) and keeps the call asynchronous.

        The model's outputs are pooled buffers that the next forward overwrites, and a picture with more than MAX_SEGMENTS classes, or
        with strings longer than `Context.sem_rle_bytes`, needs the call once more ON `pred`.  So by default the picture is settled here:
        n_classes and the offsets are read back (a few hundred bytes, one wait for this picture's kernels), a retry - rare - is enqueued
        while `pred` still holds the picture, and `pred` is let go of.  pred_kept=True: the caller leaves `pred` untouched until
        evaluate() (a buffer of its own); then nothing here waits for the device and evaluate() settles.  Either way the strings stay on
        the device until evaluate()."""
        from .runtime import DeviceArray
        if not isinstance(gt, DeviceArray):
            g = np.asarray(gt).astype(np.int32)
            g[g == self.ignore_label] = self.K
            gt = self.ctx.to_device(np.ascontiguousarray(g))
        if self.pq:
            pending = self.ctx.semantic_eval_async(pred, self.K, gt, conf=self.conf, b_conf=self.b_conf, flags=self.flags, pq_stats=self.stats)
        else:
            pending = self.ctx.semantic_eval_async(pred, self.K, gt, conf=self.conf, b_conf=self.b_conf, flags=self.flags)
        if not pred_kept:
            pending.settle()
        self._pending.append((file_name, pending))

    def rows(self) -> list:
        """This rank's prediction rows so far (resolves the pending strings: one read per picture)."""
        out = []
        for file_name, pending in self._pending:
            classes, rles, _ = pending.result()
            out += rows_from_rle(classes, rles, file_name, self.to_dataset)
        return out

    def evaluate(self, output_dir: Optional[str] = None) -> dict:
        """Every rank gets the summed matrices and all rows and returns the results (detectron2 returns them on the main rank only);
        sem_seg_predictions.json is written by rank 0 alone, as there."""
        host = self._buf.numpy()
        n = (self.K + 1) ** 2
        conf = host[:n].reshape(self.K + 1, self.K + 1)
        b_conf = host[n:2 * n].reshape(self.K + 1, self.K + 1) if self.boundary else None
        flags = int(host[2 * n:].view(np.int32)[0])
        rows = [] if flags else self.rows()                                  # a malformed map has no row for its bad labels: raise below
        conf, b_conf, rows, flags = gather(conf, b_conf, rows, flags)        # every rank raises when any rank saw a flag
        if flags:
            raise RuntimeError("semantic evaluation: malformed prediction(s): " + "; ".join(flag_names(flags)))
        self.conf_matrix, self.b_conf_matrix, self.predictions = conf, b_conf, rows
        if output_dir and _rank() == 0:
            os.makedirs(output_dir, exist_ok=True)
            with open(os.path.join(output_dir, "sem_seg_predictions.json"), "w") as f:
                f.write(json.dumps(rows))
        res = results(conf, b_conf, self.class_names)
        if self.pq:
            from . import distributed as D
            from . import semseg_pq as SP
            from .panoptic_quality import PQStats
            self.pq_stats = D.sum_pq_stats(PQStats.from_records(self.stats.numpy()))   # K * 32 bytes; the flags travelled with gather()
            res.update(SP.evaluator_results(self.pq_stats, self.class_names))
        return {result_key(self.dataset_name, self.prefix): res}
