"""YouTube-VIS AP (mask2former_video/data_video/ytvis_eval.py) on the device: `process_frame` enqueues one `odise_hip_video_eval_frame` per
frame - the masks are packed (dense, or sampled from the mask logits of the last head forward), intersected with the frame's ground truth
and added to the 64-bit sums of their tracks, no mask and no per-frame matrix crossing to the host - `end_video` one
`odise_hip_video_eval_finish`, which walks the tracks of the video and leaves one 32-byte row per track, and `evaluate` runs
COCOeval.accumulate on those rows on the device (`odise_hip_instance_accumulate`, a video standing where a picture stands).  The host
keeps summarize / results (odise_amd/instance_eval.py) and the rule in numpy (odise_amd/video_eval.py, where its status is written down:
restated from ytvoseval.py, parity with the reference evaluator unpinned).

Which track a detection belongs to is the caller's: `det_slot` names it per table index.  The library's own trackers hand out colours,
not identities; feeding det_slot from them is not part of this evaluator."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import instance_eval as IE
from . import video_eval as VE
from .runtime import Context, DeviceArray, InstanceAccumulateError


class HipVideoInstanceEvaluator:
    CHUNK = 64          # videos per block of the row buffer

    def __init__(self, ctx: Context, thing_dataset_id_to_contiguous_id: Dict[int, int], class_names: Sequence[str], max_tracks: int = 100,
                 max_gt: int = VE.MAX_GT):
        """thing_dataset_id_to_contiguous_id: the annotation's category ids -> 0..K-1; class_names [K]; max_tracks: predicted tracks per
        video (at most 100, the evaluator's last maxDets); max_gt: ground-truth tracks per video (at most 1024)."""
        self.ctx = ctx
        self.to_contiguous = {int(k): int(v) for k, v in thing_dataset_id_to_contiguous_id.items()}
        self.class_names = list(class_names)
        self.K, self.max_tracks, self.max_gt = len(self.class_names), int(max_tracks), int(max_gt)
        assert all(0 <= v < self.K for v in self.to_contiguous.values()), "contiguous ids must lie in [0, len(class_names))"
        assert 1 <= self.max_tracks <= VE.MAX_TRACKS and 0 <= self.max_gt <= VE.MAX_GT, (self.max_tracks, self.max_gt)
        self.flags = ctx.zeros((1,), np.int32)
        self.state = ctx.video_eval_state(self.max_tracks, self.max_gt)
        self.reset()

    def reset(self) -> None:
        from ._lib import check
        check(self.ctx.lib.odise_hip_memset(self.ctx.h, self.flags.ptr, 0, 4), "memset")
        self._chunks, self._videos, self._numbers = [], 0, []
        self._npig = np.zeros((self.K, 4), np.int64)
        self._gt = None

    def begin_video(self, video_index: int, gt_tracks, count_gt: bool = True) -> None:
        """Start a video: video_index orders the videos the same way on every run; gt_tracks: the video's annotation dicts (category_id as
        in the dataset, iscrowd, `areas` or `avg_area`, `segmentations` = one RLE dict, list of polygons or None per frame).  count_gt
        False: the ground truth was counted by an earlier part of the same video (categories walked apart)."""
        table = VE.gt_track_rows(gt_tracks, self.to_contiguous)
        assert len(table) <= self.max_gt, f"{len(table)} ground-truth tracks in one video (at most {self.max_gt})"
        if count_gt:
            self._npig += IE.npig(table, self.K)
        self._gt = {"video": int(video_index), "tracks": list(gt_tracks), "table": table}
        self.ctx.video_eval_reset(self.state)

    def process_frame(self, frame: int, out_hw, det_slot, masks: Optional[DeviceArray] = None, table_row=None, scores_row=None, topk: Optional[int] = None,
                      b: int = 0, pad_hw=(0, 0), img_hw=(0, 0), annotations=None) -> None:
        """One frame: dense `masks` [topk, h, w] (float32 / uint8; table_row optional), or the selection table_row / scores_row of image
        b of the last head forward (then `topk`, pad_hw and img_hw as in `Context.instance_eval`); det_slot int32 [topk] (host array or
        DeviceArray): the track of every table index, anything outside [0, max_tracks) = none.  The ground truth is entry `frame` of
        every track's `segmentations` that is not None, unless `annotations` = [(gt track, segmentation), ..] gives it.
        The ground truth goes up as one packed upload, which waits for the stream; the kernels never wait."""
        assert self._gt is not None, "process_frame before begin_video"
        if annotations is None:
            annotations = [(j, t["segmentations"][frame]) for j, t in enumerate(self._gt["tracks"]) if t["segmentations"][frame]]
        topk = int(masks.shape[0] if masks is not None else topk)
        slot = det_slot if isinstance(det_slot, DeviceArray) else self.ctx.to_device(np.ascontiguousarray(det_slot, np.int32).reshape(topk))
        gt = gt_slot = None
        if annotations:
            runs, offsets, xy, poly_offsets, gt_polys = VE.pack_segmentations([seg for _, seg in annotations], out_hw)
            gt = self.ctx.instance_gt_to_device(None, runs, offsets, *((xy, poly_offsets, gt_polys) if len(poly_offsets) > 1 else ()))
            gt_slot = self.ctx.to_device(np.asarray([j for j, _ in annotations], np.int32))
        self.ctx.video_eval_frame(self.state, out_hw, topk, slot, gt, gt_slot, self.flags, table_row=table_row, scores_row=scores_row, masks=masks,
                                  b=b, pad_hw=pad_hw, img_hw=img_hw)

    def end_video(self, track_scores, track_categories, iou: Optional[DeviceArray] = None, avg_area: Optional[DeviceArray] = None) -> None:
        """The end of the video: track_scores [n_tracks] and track_categories [n_tracks] (contiguous ids), track s being slot s."""
        assert self._gt is not None, "end_video before begin_video"
        scores = np.ascontiguousarray(track_scores, np.float32).reshape(-1)
        cats = np.ascontiguousarray(track_categories, np.int32).reshape(-1)
        n, table = len(scores), self._gt["table"]
        assert len(cats) == n and n <= self.max_tracks, (n, len(cats), self.max_tracks)
        up = self.ctx.to_device(np.concatenate([scores.view(np.uint8), cats.view(np.uint8), table.reshape(-1).view(np.uint8)]))   # one upload
        i = self._videos % self.CHUNK
        if i == 0:
            self._chunks.append((self.ctx.empty((self.CHUNK * self.max_tracks,), IE.ROW_DTYPE), self.ctx.zeros((self.CHUNK,), np.int32)))
        rows, counts = self._chunks[-1]
        self._videos += 1
        self._numbers.append(self._gt["video"])
        self.ctx.video_eval_finish(self.state, n, up.ptr, up.ptr + 4 * n, up.ptr + 8 * n, len(table), self.K, self._gt["video"],
                                   rows.view((self.max_tracks,), IE.ROW_DTYPE, i * self.max_tracks * IE.ROW_DTYPE.itemsize),
                                   counts.view((1,), np.int32, 4 * i), self.flags, iou=iou, avg_area=avg_area)
        self._gt = None

    def rows(self) -> np.ndarray:
        """The rows so far, every video's in descending score (one read per block of videos)."""
        out = []
        for c, (rows, counts) in enumerate(self._chunks):
            host, n = rows.numpy().reshape(self.CHUNK, self.max_tracks), counts.numpy()
            out += [host[i, :n[i]] for i in range(min(self.CHUNK, self._videos - c * self.CHUNK))]
        return np.concatenate(out) if out else np.zeros(0, IE.ROW_DTYPE)

    def evaluate(self, accumulate_on: str = "device") -> dict:
        """-> {"segm": detectron2's results dict} (what HipInstanceSegEvaluator.evaluate returns for segm); `precision` / `recall` stay on
        the evaluator.  accumulate_on: "device" = odise_hip_instance_accumulate, "host" = instance_eval.accumulate, bit-identical; a
        video number given twice (a video walked in parts) takes the host path, which merges such rows.  Any flag raised since `reset`
        makes this RuntimeError, flag 16 (a slot used twice in one frame) included: the sums of such a video are those of the two masks,
        not of their union, which is not what the reference would have scored.  A caller that wants to go on reads `flags` itself."""
        assert accumulate_on in ("device", "host"), accumulate_on
        flags = int(self.flags.numpy()[0])
        if flags:
            raise RuntimeError("video instance evaluation: malformed input(s): " + "; ".join(VE.flag_names(flags)))
        done = False
        if accumulate_on == "device" and len(set(self._numbers)) == len(self._numbers):
            try:
                self.precision, self.recall = self.ctx.instance_accumulate(self._chunks, self._npig, self.K, self.max_tracks)
                done = True
            except InstanceAccumulateError as e:
                if e.flags != IE.ACCUM_FLAG_NAN_SCORE:
                    raise
        if not done:
            self.precision, self.recall = IE.accumulate(self.rows(), self._npig, self.K)
        return {"segm": IE.results(self.precision, self.recall, self.class_names)}
