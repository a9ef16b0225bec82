"""COCOPanopticEvaluator (odise/evaluation/d2_evaluator.py:49) on the device: `process` enqueues one `odise_hip_panoptic_quality` per
picture on the panoptic record of `odise_hip_infer` - no PNG, no copy of the map, and no synchronisation when the ground truth is
already on the device - and `evaluate` reads the small accumulator back once, sums it and ORs the flags across ranks and does the metric
arithmetic on the host (odise_amd/panoptic_quality.py).  With `boundary=True` the call is `odise_hip_panoptic_quality_boundary` and Boundary PQ
(the project's restatement of Cheng et al., CVPR 2021; parity with the published boundary-iou package is unpinned) is scored beside PQ."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from . import distributed as D
from . import panoptic_quality as PQ
from .runtime import Context, DeviceArray


class HipPanopticEvaluator:
    def __init__(self, ctx: Context, dataset_id_to_contiguous_id: Dict[int, int], isthing: Sequence[bool], boundary: bool = False,
                 radius=None):
        """dataset_id_to_contiguous_id: the annotation's category ids -> 0..C-1, the space the model's category_id lives in (detectron2
        metadata: thing_ / stuff_dataset_id_to_contiguous_id merged); isthing [C] per contiguous id.  boundary: also accumulate the
        Boundary PQ statistics (`evaluate` then adds the B* keys), at `radius` erosions (None: the formula of `boundary_radius`)."""
        self.ctx = ctx
        self.to_contiguous = {int(k): int(v) for k, v in dataset_id_to_contiguous_id.items()}
        self.isthing = [bool(t) for t in isthing]
        self.C = len(self.isthing)
        assert all(0 <= v < self.C for v in self.to_contiguous.values()), "contiguous ids must lie in [0, len(isthing))"
        self.boundary, self.radius = bool(boundary), int(radius or 0)
        # one buffer, one copy in evaluate(): C records (with boundary: C more, the Boundary PQ statistics), then a record whose first
        # int32 holds the flags
        self.n_records = (2 if self.boundary else 1) * self.C
        self._buf = ctx.empty((self.n_records + 1,), PQ.STAT_DTYPE)
        self.stats = self._buf.view((self.C,), PQ.STAT_DTYPE)
        self.b_stats = self._buf.view((self.C,), PQ.STAT_DTYPE, self.C * PQ.STAT_DTYPE.itemsize) if self.boundary else None
        self.flags = self._buf.view((1,), np.int32, self.n_records * PQ.STAT_DTYPE.itemsize)
        self.reset()

    def reset(self) -> None:
        from ._lib import check
        check(self.ctx.lib.odise_hip_memset(self.ctx.h, self._buf.ptr, 0, self._buf.nbytes), "memset")

    def gt_table(self, segments_info) -> np.ndarray:
        """The annotation's segments_info dicts -> rows (id, contiguous category, iscrowd, area)."""
        return np.asarray([[int(s["id"]), self.to_contiguous[int(s["category_id"])], int(s.get("iscrowd", 0)), int(s["area"])]
                           for s in segments_info], np.int32).reshape(-1, 4)

    def process(self, record: DeviceArray, hw, gt_rgb, gt_segments_info) -> None:
        """record: the picture's panoptic record on the device; gt_rgb: the annotation PNG as decoded, uint8 [H,W,3]; gt_segments_info: the
        annotation's dicts (id, category_id as in the dataset, iscrowd, area).
        A DeviceArray gt_rgb (decoded or uploaded ahead by the loader) keeps the call asynchronous.  A host array is a convenience that
        WAITS for the device twice per picture: `to_device` synchronises on the upload, and the temporary is freed on return by the
        library's synchronising free - which is also what keeps it alive until the two kernels have read it."""
        if not isinstance(gt_rgb, DeviceArray):
            gt_rgb = self.ctx.to_device(np.ascontiguousarray(gt_rgb, np.uint8))
        if self.boundary:
            self.ctx.panoptic_quality_boundary_record(record, hw, gt_rgb, self.gt_table(gt_segments_info), self.C, self.stats, self.b_stats,
                                                      self.flags, self.radius)
        else:
            self.ctx.panoptic_quality_record(record, hw, gt_rgb, self.gt_table(gt_segments_info), self.C, self.stats, self.flags)

    def evaluate(self) -> dict:
        host = self._buf.numpy()                                                     # C (or 2 C) * 32 bytes (+ the flags record)
        n = self.n_records
        flags = int(host[n:].view(np.int32)[0])
        total, flags = D.sum_pq_stats(PQ.PQStats.from_records(host[:n]), flags)      # every rank raises when any rank saw a flag
        if flags:
            raise RuntimeError("panoptic evaluation: malformed prediction(s): " + "; ".join(PQ.flag_names(flags)))
        records = total.to_records()                                                 # one sum across ranks for both halves
        self.pq_stats = PQ.PQStats.from_records(records[:self.C])
        out = PQ.results(self.pq_stats, self.isthing)
        if self.boundary:
            self.boundary_stats = PQ.PQStats.from_records(records[self.C:])
            out.update(PQ.boundary_results(self.boundary_stats, self.isthing))
        return out
