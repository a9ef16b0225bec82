"""InstanceSegEvaluator / COCOEvaluator(tasks=("segm",)) (odise/evaluation/d2_evaluator.py:29,104) on the device: `process` enqueues one
`odise_hip_instance_eval` per picture on the instance selection of `odise_hip_infer` - the masks are sampled from the mask logits, matched
against the ground truth and reduced to one 32-byte row per detection, no RLE string and no JSON - and `evaluate` runs
COCOeval.accumulate on the device too (`odise_hip_instance_accumulate`: on one rank the rows never leave it; across ranks they are
gathered on the host first and go up again as one block), which leaves the host summarize / results (odise_amd/instance_eval.py).

Ground truth is what COCO's instance annotations hold: polygons (rasterised on the device, pycocotools' annToRLE bit for bit) for the
objects, RLE (compressed or uncompressed) for the crowds, mixed freely in one picture.

tasks=("bbox",) or ("bbox", "segm") is COCOEvaluator's bbox task beside (or without) segm: `process` enqueues one
`odise_hip_instance_eval_bbox`, which takes the detections' boxes from the same packed masks (BitMasks.get_bounding_boxes, the line the
reference leaves out as slow) and matches them against the annotations' `bbox`; every task keeps row blocks of its own, the row format
and everything behind it are shared.

"boundary" in `tasks` (any combination with the other two) is Boundary AP (Cheng et al., "Boundary IoU", CVPR 2021; LVIS' third
iouType): the same matching on min(mask IoU, boundary IoU), the boundaries eroded out of the packed words on the device
(`odise_hip_instance_eval_boundary`, csrc/inst_boundary.hip) behind the same pack and the same decode.  Its rule is restated from the paper
and detectron2's `_mask_to_boundary`; parity with the published boundary-iou package is unpinned (odise_amd/instance_eval.py)."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from . import distributed as D
from . import instance_eval as IE
from .runtime import Context, DeviceArray, InstanceAccumulateError


class HipInstanceSegEvaluator:
    CHUNK = 64          # pictures per block of the row buffer: it grows by whole blocks, rows already written stay where they are

    TASKS = ("bbox", "segm", "boundary")                                       # detectron2's order of the result groups, then Boundary AP
    MAX_TOPK = IE.MAX_DETECTIONS

    # what `evaluate` does behind the gather; HipLvisEvaluator (lvis_seg_eval.py) stands on the same plumbing with its own four
    def _accumulate_device(self, blocks, npig):
        return self.ctx.instance_accumulate(blocks, npig, self.K, self.topk)

    def _accumulate_host(self, rows, npig):
        return IE.accumulate(rows, npig, self.K)

    def _results(self) -> dict:
        return IE.results(self.precision, self.recall, self.class_names)

    _flag_names = staticmethod(IE.flag_names)

    def __init__(self, ctx: Context, thing_dataset_id_to_contiguous_id: Dict[int, int], class_names: Sequence[str], topk: int = 100,
                 tasks: Sequence[str] = ("segm",), boundary_radius: int = 0):
        """thing_dataset_id_to_contiguous_id: the annotation's category ids -> 0..K-1, the space the model's pred_classes live in;
        class_names [K] per contiguous id; topk: the model's test_topk_per_image (at most 100, COCOeval's last maxDets);
        tasks: any of "bbox", "segm", "boundary" - with "bbox" every annotation needs its `bbox`; boundary_radius: the erosion radius of
        the boundary task, 0 = the formula of the picture's size (sem_boundary.boundary_radius)."""
        self.ctx = ctx
        assert len(tasks) > 0 and set(tasks) <= set(self.TASKS) and len(set(tasks)) == len(tasks), tasks
        self.tasks = tuple(t for t in self.TASKS if t in tasks)
        self.to_contiguous = {int(k): int(v) for k, v in thing_dataset_id_to_contiguous_id.items()}
        self.class_names = list(class_names)
        self.K, self.topk, self.boundary_radius = len(self.class_names), int(topk), int(boundary_radius)
        assert all(0 <= v < self.K for v in self.to_contiguous.values()), "contiguous ids must lie in [0, len(class_names))"
        assert 1 <= self.topk <= self.MAX_TOPK, self.topk
        self.flags = ctx.zeros((1,), np.int32)
        self.reset()

    def reset(self) -> None:
        from ._lib import check
        check(self.ctx.lib.odise_hip_memset(self.ctx.h, self.flags.ptr, 0, 4), "memset")
        self._task_chunks, self._pictures, self._images = {t: [] for t in self.tasks}, 0, []
        self._chunks = self._task_chunks[self._main_task()]                    # the segm task's blocks when it is there
        self._npig = np.zeros((self.K, 4), np.int64)

    def _main_task(self) -> str:
        return "segm" if "segm" in self.tasks else self.tasks[-1]

    def _slot(self):
        """{task: (rows [topk], n_rows [1])} of the next picture."""
        i = self._pictures % self.CHUNK
        out = {}
        for t in self.tasks:
            if i == 0:
                self._task_chunks[t].append((self.ctx.empty((self.CHUNK * self.topk,), IE.ROW_DTYPE), self.ctx.zeros((self.CHUNK,), np.int32)))
            rows, counts = self._task_chunks[t][-1]
            out[t] = rows.view((self.topk,), IE.ROW_DTYPE, i * self.topk * IE.ROW_DTYPE.itemsize), counts.view((1,), np.int32, 4 * i)
        self._pictures += 1
        return out

    def process(self, b: int, inst_table_row, inst_scores_row, pad_hw, img_hw, out_hw, annotations, image_index: int, pred_masks=None) -> None:
        """One picture: inst_table_row [1 + 2 topk] / inst_scores_row [topk] = image b's rows of the device instance table of the last
        call (HipCategoryODISE.keep_instance_selection -> last_selection), pad_hw / img_hw / out_hw as in `Context.instance_rle`;
        annotations: the picture's dicts (category_id as in the dataset, iscrowd, area, segmentation = RLE dict or a list of polygons);
        image_index: any number
        that orders the pictures the same way on every run (the position in the dataset).  With `pred_masks` (DeviceArray [topk, h, w],
        float32 or uint8) the detections are those dense masks instead of the mask logits.
        The ground truth goes up as one packed upload, which WAITS for the stream, and the temporary is freed on return by the library's
        synchronising free - which is also what keeps it alive until the kernels have read it.  The kernels themselves never wait."""
        table, runs, offsets, xy, poly_offsets, gt_polys = IE.gt_rows(annotations, self.to_contiguous, polygons=True, hw=out_hw)
        assert len(table) <= IE.MAX_GT, f"{len(table)} ground-truth masks in one picture (at most {IE.MAX_GT})"
        self._npig += IE.npig(table, self.K)
        boxes = IE.gt_boxes(annotations) if "bbox" in self.tasks else None
        gt = self.ctx.instance_gt_to_device(table, runs, offsets, *((xy, poly_offsets, gt_polys) if len(poly_offsets) > 1 else ()), boxes=boxes)
        slot = self._slot()
        self._images.append(int(image_index))
        boundary = slot["boundary"] + (self.boundary_radius,) if "boundary" in self.tasks else None
        if "bbox" in self.tasks:
            self.ctx.instance_eval_bbox(out_hw, inst_table_row, inst_scores_row, self.topk, gt, self.K, int(image_index), *slot["bbox"], self.flags,
                                        *slot.get("segm", (None, None)), masks=pred_masks, b=b, pad_hw=pad_hw, img_hw=img_hw, boundary=boundary)
        else:
            self.ctx.instance_eval(out_hw, inst_table_row, inst_scores_row, self.topk, gt, self.K, int(image_index), *slot.get("segm", (None, None)),
                                   self.flags, masks=pred_masks, b=b, pad_hw=pad_hw, img_hw=img_hw, boundary=boundary)

    def process_selection(self, selection: dict, annotations_per_image, image_indices) -> None:
        """`process` for every picture of a batch from `HipCategoryODISE.last_selection`."""
        topk = selection["topk"]
        assert topk == self.topk, (topk, self.topk)
        for b, (anns, idx) in enumerate(zip(annotations_per_image, image_indices)):
            self.process(b, selection["inst_table"].view((1 + 2 * topk,), np.int32, b * (1 + 2 * topk) * 4),
                         selection["inst_scores"].view((topk,), np.float32, b * topk * 4), selection["pad_hw"], selection["img_hw"][b],
                         selection["out_hw"][b], anns, idx)

    def rows(self, task: str = None) -> np.ndarray:
        """This rank's rows of a task so far (one read per block of pictures); task: "segm" where it runs, else the last of the tasks."""
        out = []
        for c, (rows, counts) in enumerate(self._task_chunks[task or self._main_task()]):
            host, n = rows.numpy().reshape(self.CHUNK, self.topk), counts.numpy()
            used = min(self.CHUNK, self._pictures - c * self.CHUNK)
            out += [host[i, :n[i]] for i in range(used)]
        return np.concatenate(out) if out else np.zeros(0, IE.ROW_DTYPE)

    @staticmethod
    def slots_of(rows: np.ndarray, topk: int):
        """Compact rows (every picture's rows back to back) -> (rows [slots * topk], counts int32 [slots]), a slot per run of one `image`
        number, or None when an image number comes back after another one or a run is longer than topk: pictures that the host function
        would merge."""
        rows = np.asarray(rows, IE.ROW_DTYPE).reshape(-1)
        first = np.flatnonzero(np.r_[True, rows["image"][1:] != rows["image"][:-1]]) if len(rows) else np.zeros(0, np.int64)
        counts = np.diff(np.r_[first, len(rows)]).astype(np.int32)
        if len(np.unique(rows["image"][first])) != len(first) or (counts > topk).any():
            return None
        out = np.zeros((len(first), topk), IE.ROW_DTYPE)
        out[np.repeat(np.arange(len(first)), counts), np.arange(len(rows)) - np.repeat(first, counts)] = rows
        return out.reshape(-1), counts

    def evaluate(self, accumulate_on: str = "device") -> dict:
        """accumulate_on: "device" = odise_hip_instance_accumulate, "host" = instance_eval.accumulate; the results are bit-identical.  When an
        image number was given twice the host path is taken whatever was asked: the host function merges such pictures and the device
        order is not defined for them.
        -> detectron2's results of the task; with tasks other than ("segm",) one such group per task, {"bbox": .., "segm": .., "boundary": ..}.
        `precision` / `recall` are those of the last task, `task_precision` / `task_recall` hold every task's."""
        import torch
        import torch.distributed as dist
        assert accumulate_on in ("device", "host"), accumulate_on
        many = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        flags, npig = int(self.flags.numpy()[0]), self._npig
        gathered = None
        if many:
            parts = [None] * dist.get_world_size()
            dist.all_gather_object(parts, ({t: self.rows(t) for t in self.tasks}, flags))
            gathered = {t: np.concatenate([p[0][t] for p in parts]) for t in self.tasks}
            for p in parts:
                flags |= int(p[1])                                           # every rank raises when any rank saw a flag
            npig = D.sum_confusion(torch.from_numpy(npig.copy())).numpy()
        if flags:
            raise RuntimeError("instance evaluation: malformed input(s): " + "; ".join(self._flag_names(flags)))
        self.task_precision, self.task_recall, out = {}, {}, {}
        for t in self.tasks:
            blocks = None
            if many:
                if accumulate_on == "device":
                    block = self.slots_of(gathered[t], self.topk)            # the same decision on every rank: it is made on the gathered rows
                    blocks = [block] if block is not None else None
            elif accumulate_on == "device" and len(set(self._images)) == len(self._images):
                blocks = self._task_chunks[t]                                # as they lie
            if blocks is not None:
                try:
                    self.precision, self.recall = self._accumulate_device(blocks, npig)
                except InstanceAccumulateError as e:
                    if e.flags != IE.ACCUM_FLAG_NAN_SCORE:
                        raise
                    blocks = None                                            # a NaN score: the device sort has no place for it, numpy's has
            if blocks is None:
                self.precision, self.recall = self._accumulate_host(gathered[t] if many else self.rows(t), npig)
            self.task_precision[t], self.task_recall[t] = self.precision, self.recall
            out[t] = self._results()
        return out["segm"] if self.tasks == ("segm",) else out
