"""Multi-scale and flip test-time augmentation of the semantic head.

`HipSemanticTTA` restates Mask2Former's `SemanticSegmentorWithTTA` (mask2former/test_time_augmentation.py) over detectron2's
`DatasetMapperTTA`: the picture at every `min_size` (ResizeShortestEdge(min_size, max_size), Pillow-exact on the device), each followed by
the same resized picture mirrored when `flip` is set; every view runs the model on its own (`self.model([input])` there, one
`odise_hip_infer` here - the library pads a batch to its largest member, so views of different sizes never share a call); the views'
`sem_seg` at the ORIGINAL size are averaged.

The reference adds K x h x w tensors (`final_predictions += ...`).  Here no view's `sem_seg` exists: each call runs with its own semantic
output off, `odise_hip_tta_add_view` keeps the view's pixel-major sigmoid matrix and class probabilities, and `odise_hip_tta_finish` is one
product over all views' queries - the mean, or with the model's `semantic_argmax` its arg-max without the [K, h, w] tensor.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Sequence, Tuple

import numpy as np

from .ingest import resize_shortest_edge_shape
from .runtime import DeviceArray

MAX_HANDLES = 2          # cached odise_tta handles (S_cat of a 1280 x 1280 picture with 6 views of 100 queries is 2 GB)


def tta_views(h: int, w: int, min_sizes: Sequence[int], max_size: int, flip: bool = True) -> List[Tuple[Tuple[int, int], bool]]:
    """DatasetMapperTTA's view list for an h x w picture, in its order: [((view_h, view_w), mirrored), ...]."""
    views = []
    for m in min_sizes:
        hw = resize_shortest_edge_shape(int(h), int(w), int(m), int(max_size))
        views.append((hw, False))
        if flip:
            views.append((hw, True))
    return views


class HipSemanticTTA:
    """SemanticSegmentorWithTTA over a `HipCategoryODISE` (semantic_on) or a `HipOpenPanopticInference(semantic_on=True)`: the same
    `batched_inputs` in, a list of {"sem_seg": fp32 [K,h,w]} out - or {"sem_seg_argmax": int32 [h,w]} when the model's `semantic_argmax` is
    set, which is what `HipSemSegEvaluator` takes and never holds the K x h x w tensor."""

    def __init__(self, model, min_sizes: Sequence[int], max_size: int, flip: bool = True):
        assert len(min_sizes) >= 1, "HipSemanticTTA: no min_sizes"
        self.model, self.min_sizes, self.max_size, self.flip = model, tuple(int(m) for m in min_sizes), int(max_size), bool(flip)
        self._handles: "OrderedDict[tuple, object]" = OrderedDict()

    def views(self, h: int, w: int):
        return tta_views(h, w, self.min_sizes, self.max_size, self.flip)

    # ---- handles: one per (out_h, out_w, K, views), least recently used first ------------------------------------------------------------
    def _handle(self, ctx, hw, K: int, Q: int, A: int):
        key = (int(hw[0]), int(hw[1]), int(K), int(A))
        t = self._handles.pop(key, None)
        if t is None or t.Q != Q:
            if t is not None:
                t.close()
            while len(self._handles) >= MAX_HANDLES:
                self._handles.popitem(last=False)[1].close()
            t = ctx.tta_create(hw, K, Q, A)
        self._handles[key] = t
        t.reset()
        return t

    def close(self) -> None:
        while self._handles:
            self._handles.popitem()[1].close()

    # ---- one picture ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _picture(ctx, x: dict) -> DeviceArray:
        """The input's "image" as uint8 [H,W,3] on the device, at the ORIGINAL size (DatasetMapperTTA undoes the mapper's resize first)."""
        if "image" not in x:                                              # SemanticSegmentorWithTTA reads the file itself then
            from .demo import read_picture
            im = read_picture(ctx, x["file_name"])
        else:
            im = x["image"]
        if not isinstance(im, DeviceArray):
            if hasattr(im, "detach"):
                im = im.detach().cpu().numpy()
            im = np.asarray(im).transpose(1, 2, 0)
            if im.dtype != np.uint8:                                       # a float picture 0..255: to the nearest value, not truncated
                im = np.clip(np.rint(im), 0, 255).astype(np.uint8)
            im = ctx.to_device(np.ascontiguousarray(im))
        assert im.dtype == np.uint8 and len(im.shape) == 3 and im.shape[2] == 3, "HipSemanticTTA: uint8 [H,W,3] on the device, or CHW on the host"
        H, W = int(x.get("height", im.shape[0])), int(x.get("width", im.shape[1]))
        if (H, W) != tuple(im.shape[:2]):
            im = ctx.resize_bilinear_u8(im, H, W)
        return im

    def _one(self, inner, x: dict, index: int, to_host: bool, alloc=None) -> dict:
        ctx = inner.ctx
        picture = self._picture(ctx, x)
        H, W = picture.shape[:2]
        K, Q = int(inner.num_classes), int(inner.num_queries)
        views = self.views(H, W)
        handle = self._handle(ctx, (H, W), K, Q, len(views))
        cls = inner._buf("tta_mask_cls", (1, Q, K + 1), np.float32)
        resized, resized_hw = None, None
        for hw, mirrored in views:
            if resized_hw != hw:                                           # a view and its mirror share the resized picture
                resized, resized_hw = (picture if hw == (H, W) else ctx.resize_bilinear_u8(picture, hw[0], hw[1])), hw
            image = ctx.hflip_u8_hwc(resized, inner._buf("tta_mirror", (hw[0], hw[1], 3), np.uint8)) if mirrored else resized
            inner.infer_device([image], 0, [hw], [(H, W)], mask_cls_out=cls)   # every head's own output is off: nothing is read back
            div = int(inner.size_divisibility)                             # the padded size of this call, as infer_device has it
            handle.add_view(0, cls, (-(-hw[0] // div) * div, -(-hw[1] // div) * div), hw, mirrored)
        alloc = alloc or inner._buf                                        # (tag, shape, dtype) -> DeviceArray, as pipeline._post_desc takes it
        if inner.semantic_argmax:
            out = alloc(f"amax{index}", (H, W), np.int32)
            handle.finish(sem_argmax=out)
            return {"sem_seg_argmax": out.numpy() if to_host else out}
        out = alloc(f"sem{index}", (K, H, W), np.float32)
        handle.finish(sem_seg=out)
        return {"sem_seg": out.numpy() if to_host else out}

    def forward(self, batched_inputs, to_host: bool = True, alloc=None) -> list:
        """`alloc(tag, shape, dtype) -> DeviceArray` lets the caller own the results ("sem<i>" / "amax<i>", as HipCategoryODISE.forward's)."""
        from .pipeline import HipOpenPanopticInference
        wrapper = self.model if isinstance(self.model, HipOpenPanopticInference) else None
        inner = wrapper.model if wrapper is not None else self.model
        saved = inner.open_state_dict() if wrapper is not None else None
        if wrapper is not None:
            inner.load_open_state_dict(wrapper.open_state_dict)
        heads = inner.semantic_on, inner.panoptic_on, inner.instance_on
        try:
            assert inner.semantic_on, "HipSemanticTTA: the model's semantic head is off"
            inner.semantic_on = inner.panoptic_on = inner.instance_on = False     # of the views' own calls
            return [self._one(inner, x, i, to_host, alloc) for i, x in enumerate(batched_inputs)]
        finally:
            inner.semantic_on, inner.panoptic_on, inner.instance_on = heads
            if wrapper is not None:
                inner.load_open_state_dict(saved)

    __call__ = forward
