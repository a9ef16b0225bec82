"""`mask2former.test_time_augmentation.SemanticSegmentorWithTTA` on libodise_hip.so (reference:
third_party/Mask2Former/mask2former/test_time_augmentation.py): multi-scale / flip test-time augmentation of the semantic scores.  The view
list (detectron2's DatasetMapperTTA: every `cfg.TEST.AUG.MIN_SIZES` entry, each followed by its mirror when `FLIP`), the per-view model call
and the mean at the original size are `odise_amd.tta.HipSemanticTTA`; no view's [K, h, w] tensor is ever added up."""
import torch
from torch import nn

from odise_amd.tta import HipSemanticTTA

__all__ = ["SemanticSegmentorWithTTA"]

# detectron2's defaults of cfg.TEST.AUG (config/defaults.py)
_MIN_SIZES, _MAX_SIZE, _FLIP = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200), 4000, True


def _aug_settings(cfg):
    aug = getattr(getattr(cfg, "TEST", None), "AUG", None)
    if aug is None and isinstance(cfg, dict):
        aug = cfg.get("TEST", {}).get("AUG")
    get = (lambda k, d: aug.get(k, d)) if isinstance(aug, dict) else (lambda k, d: getattr(aug, k, d))
    if aug is None:
        return _MIN_SIZES, _MAX_SIZE, _FLIP
    return tuple(int(m) for m in get("MIN_SIZES", _MIN_SIZES)), int(get("MAX_SIZE", _MAX_SIZE)), bool(get("FLIP", _FLIP))


class SemanticSegmentorWithTTA(nn.Module):
    """`model`: the overlay's CategoryODISE / CaptionODISE (a torch module on the library), an OpenPanopticInference around one, or a
    HipCategoryODISE / HipOpenPanopticInference.  `batch_size` is accepted for the signature; every view is one model call, as in the reference."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1):
        super().__init__()
        if tta_mapper is not None:
            raise NotImplementedError("libodise_hip builds the views itself (DatasetMapperTTA's list from cfg.TEST.AUG): a custom tta_mapper is not supported")
        if isinstance(model, nn.parallel.DistributedDataParallel):
            model = model.module
        object.__setattr__(self, "model", model)        # not a submodule: the wrapper owns no weights
        self.cfg, self.batch_size = cfg, batch_size
        self.min_sizes, self.max_size, self.flip = _aug_settings(cfg)
        self._tta = None

    def _resolve(self):
        """-> (the ODISE module that owns the fused engine or None, the open state to run under or None).  `model` may be the overlay's
        CategoryODISE / CaptionODISE, an OpenPanopticInference-style module around one (`.model` + `.open_state_dict`: the views then run under
        the wrapper's vocabulary and switches, as its own forward would set them), or a Hip* object of odise_amd.pipeline."""
        model = self.model
        if not isinstance(model, nn.Module):
            return None, None
        if hasattr(model, "_engine") and hasattr(model, "_set_vocabulary"):
            return model, None
        inner = getattr(model, "model", None)
        if isinstance(getattr(model, "open_state_dict", None), dict) and hasattr(inner, "_engine") and hasattr(inner, "_set_vocabulary"):
            return inner, model.open_state_dict
        raise TypeError(f"SemanticSegmentorWithTTA: {type(model).__name__} is neither an ODISE model on libodise_hip nor a wrapper around one")

    def forward(self, batched_inputs):
        odise, state = self._resolve()
        if odise is None:
            return self._run(self.model, torch.device("cpu"), batched_inputs)
        saved = odise.open_state_dict() if state is not None else None
        if state is not None:
            odise.load_open_state_dict(state)
        try:
            engine = odise._engine()                     # the fused engine with the module's switches, then the current vocabulary
            text_head = getattr(odise, "category_head", None)
            odise._set_vocabulary(engine, text_head if text_head is not None else odise.word_head)
            return self._run(engine, odise.device, batched_inputs)
        finally:
            if state is not None:
                odise.load_open_state_dict(saved)

    def _run(self, engine, device, batched_inputs):
        if self._tta is None or self._tta.model is not engine:
            if self._tta is not None:
                self._tta.close()
            self._tta = HipSemanticTTA(engine, self.min_sizes, self.max_size, self.flip)
        if device.type != "cuda":                        # a model on the CPU returns CPU tensors: the result crosses PCIe once
            return [{k: torch.from_numpy(v) for k, v in r.items()} for r in self._tta.forward(batched_inputs, to_host=True)]
        from odise_amd import dropin                     # a model on the device: the library writes torch tensors there in place
        outs = dropin.TorchOutputs(device)

        def alloc(tag, shape, dtype):
            view = outs(tag, shape, dtype)
            outs.ready()
            return view
        results = self._tta.forward(batched_inputs, to_host=False, alloc=alloc)
        (engine.ctx if hasattr(engine, "ctx") else engine.model.ctx).sync()   # the tensors are complete when the caller's stream touches them
        return [{k: outs.tensors[("sem" if k == "sem_seg" else "amax") + str(i)] for k in r} for i, r in enumerate(results)]
