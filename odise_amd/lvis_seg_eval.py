"""detectron2's LVISEvaluator for "segm" on the device: `process` enqueues one `odise_hip_lvis_eval` per picture - the walk of
`odise_hip_instance_eval` at up to 300 detections over all categories with LVIS' federated rules (neg_category_ids,
not_exhaustive_category_ids) - and `evaluate` runs LVISEval.accumulate on the device too (`odise_hip_lvis_accumulate`), which leaves the
host summarize / results (odise_amd/lvis_eval.py, where the rule is written down; parity with the `lvis` package is unpinned).

It stands on the plumbing of HipInstanceSegEvaluator: row blocks that grow by whole blocks, the gather across ranks, every rank raising
when any rank saw a flag.

The instance head has 100 queries, so a 300-row table holds (query, class) pairs; the device packs every distinct query once.  The
evaluator takes that table from the caller (`process` / `process_selection`); dense masks go through `pred_masks` or `process_masks`.
Scope: iouType "segm"."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from . import lvis_eval as LE
from .instance_seg_eval import HipInstanceSegEvaluator
from .runtime import Context


class HipLvisEvaluator(HipInstanceSegEvaluator):
    MAX_TOPK = LE.MAX_DETS

    def __init__(self, ctx: Context, thing_dataset_id_to_contiguous_id: Dict[int, int], class_names: Sequence[str], frequencies: Sequence[str],
                 topk: int = LE.MAX_DETS):
        """thing_dataset_id_to_contiguous_id and class_names as for HipInstanceSegEvaluator; frequencies: "r", "c" or "f" per contiguous
        id (the categories' `frequency`); topk: the rows of the table a picture comes with, at most 300 (LVISEval's max_dets)."""
        super().__init__(ctx, thing_dataset_id_to_contiguous_id, class_names, topk, tasks=("segm",))
        self.frequencies = [str(f) for f in frequencies]
        assert len(self.frequencies) == self.K and set(self.frequencies) <= set(LE.FREQUENCIES), (len(self.frequencies), self.K)

    def _accumulate_device(self, blocks, npig):
        return self.ctx.lvis_accumulate(blocks, npig, self.K, self.topk)

    def _accumulate_host(self, rows, npig):
        return LE.accumulate(rows, npig, self.K)

    def _results(self) -> dict:
        return LE.results(self.precision, self.recall, self.frequencies)

    _flag_names = staticmethod(LE.flag_names)

    def _contiguous(self, ids, what: str) -> list:
        bad = [int(c) for c in ids if int(c) not in self.to_contiguous]
        if bad:
            raise ValueError(f"lvis evaluation: {what} holds dataset ids outside the mapping: {bad}")
        return [self.to_contiguous[int(c)] for c in ids]

    def process(self, b: int, inst_table_row, inst_scores_row, pad_hw, img_hw, out_hw, annotations, neg_category_ids,
                not_exhaustive_category_ids, image_index: int, pred_masks=None) -> None:
        """One picture, as HipInstanceSegEvaluator.process: inst_table_row [1 + 2 topk] = n | query | class and inst_scores_row [topk] hold
        the picture's detections cut at 300 (lvis_eval.limit_dets); annotations: the picture's dicts (category_id, area, segmentation = RLE
        dict or polygons, optionally `ignore`); neg_category_ids / not_exhaustive_category_ids: the picture's lists of DATASET ids - one
        outside the mapping raises ValueError.  With `pred_masks` (DeviceArray [topk, h, w]) the detections are those dense masks."""
        neg = self._contiguous(neg_category_ids, "neg_category_ids")
        nex = self._contiguous(not_exhaustive_category_ids, "not_exhaustive_category_ids")
        table, runs, offsets, xy, poly_offsets, gt_polys = LE.gt_rows(annotations, self.to_contiguous, polygons=True, hw=out_hw)
        assert len(table) <= LE.MAX_GT, f"{len(table)} ground-truth masks in one picture (at most {LE.MAX_GT})"
        self._npig += LE.npig(table, self.K)
        gt = self.ctx.instance_gt_to_device(table, runs, offsets, *((xy, poly_offsets, gt_polys) if len(poly_offsets) > 1 else ()),
                                            lvis_bits=(LE.category_bits(neg, self.K), LE.category_bits(nex, self.K)))
        slot = self._slot()
        self._images.append(int(image_index))
        self.ctx.lvis_eval(out_hw, inst_table_row, inst_scores_row, self.topk, gt, self.K, int(image_index), *slot["segm"], self.flags,
                           masks=pred_masks, b=b, pad_hw=pad_hw, img_hw=img_hw)

    def process_selection(self, selection: dict, annotations_per_image, neg_per_image, not_exhaustive_per_image, image_indices) -> None:
        """`process` for every picture of a batch from a selection dict (inst_table [B, 1 + 2 topk], inst_scores [B, topk], pad_hw,
        img_hw [B], out_hw [B], topk), the shape of `HipCategoryODISE.last_selection`."""
        topk = selection["topk"]
        assert topk == self.topk, (topk, self.topk)
        for b, (anns, neg, nex, idx) in enumerate(zip(annotations_per_image, neg_per_image, not_exhaustive_per_image, image_indices)):
            self.process(b, selection["inst_table"].view((1 + 2 * topk,), np.int32, b * (1 + 2 * topk) * 4),
                         selection["inst_scores"].view((topk,), np.float32, b * topk * 4), selection["pad_hw"], selection["img_hw"][b],
                         selection["out_hw"][b], anns, neg, nex, idx)

    def process_masks(self, masks, scores, classes, annotations, neg_category_ids, not_exhaustive_category_ids, image_index: int) -> None:
        """`process` of host masks uint8 [n, h, w] with scores [n] and contiguous classes [n], n <= topk, already cut (lvis_eval.limit_dets):
        they are padded to topk and uploaded with a table of their own."""
        masks = np.ascontiguousarray(masks, np.uint8)
        n, h, w = masks.shape
        assert n <= self.topk, (n, self.topk)
        table = np.zeros(1 + 2 * self.topk, np.int32)
        table[0] = n
        table[1:1 + n] = np.arange(n)
        table[1 + self.topk:1 + self.topk + n] = np.asarray(classes, np.int32).reshape(-1)[:n]
        sc = np.zeros(self.topk, np.float32)
        sc[:n] = np.asarray(scores, np.float32).reshape(-1)[:n]
        dense = np.zeros((self.topk, h, w), np.uint8)
        dense[:n] = masks
        self.process(0, self.ctx.to_device(table), self.ctx.to_device(sc), (0, 0), (0, 0), (h, w), annotations, neg_category_ids,
                     not_exhaustive_category_ids, image_index, pred_masks=self.ctx.to_device(dense))

    def evaluate(self, accumulate_on: str = "device") -> dict:
        """-> {"segm": detectron2's LVIS dict (AP, AP50, AP75, APs, APm, APl, APr, APc, APf, each times 100)}; accumulate_on as for
        HipInstanceSegEvaluator, the two paths bit-identical."""
        return {"segm": super().evaluate(accumulate_on)}
