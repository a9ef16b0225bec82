"""`python -m odise_amd.demo (--input FILE... | --video-input SRC [--ttl N] [--track-masks]) --output DIR [--vocab "a, b; c"] [--synthetic] [--task panoptic|semantic|instance] [--tta 768,1024,1280 [--no-tta-flip]]`:
demo/demo.py on the device path.

A picture is read (JPEG through HipDatasetMapper, anything else through Pillow), resized by ResizeShortestEdge(1024, 2560) on the device,
run through HipOpenPanopticInference with demo.py's settings (overlap_threshold = 0, alpha / beta = 0.35 / 0.65, demo.py:316-318), and
its panoptic record - still in HBM - is drawn by HipVisualizer.draw_panoptic_seg and saved with Pillow as DIR/<name>.png.

`--task semantic` / `--task instance` take the other branch of run_on_image: the wrapper is built with that head on (and panoptic off), and
the semantic map (HipVisualizer.draw_sem_seg), then the instance selection (draw_instance_predictions, scores below
`--confidence-threshold` left out) are drawn, the instances on top.

`--task semantic --tta 768,1024,1280` averages the semantic scores over the picture at these short-edge sizes, each also mirrored unless
`--no-tta-flip` (odise_amd/tta.py HipSemanticTTA: Mask2Former's SemanticSegmentorWithTTA), and draws the arg-max of the mean.

`--video-input SRC` takes run_on_video (demo.py:201-243) instead: SRC is a directory of frames (read in sorted name order) or a multi-frame
file Pillow opens (no container decoding); every frame goes through the same model call and is drawn by
HipVideoVisualizer.draw_panoptic_seg_predictions, which keeps a thing's colour from frame to frame (`--ttl` frames of memory), and saved as
DIR/frame_%06d.png - or, when `--output` ends in .gif, all frames as one animated GIF.  `--task semantic` draws every frame on its own;
`--task instance` is refused (the reference tracks pred_boxes there, which are all zeros on this model) unless `--track-masks` is given:
then the instances of every frame are matched to the earlier ones on mask IoU (HipVideoVisualizer.draw_instance_predictions: detectron2's
rule for instances without a box; not what the reference's zero boxes produce, which is a fresh colour per instance and frame) and
`--confidence-threshold` is honoured as on single pictures.

Weights come from `$ODISE_MODEL_ZOO` through odise_amd/checkpoint.py; `--synthetic` takes random tensors of the real shapes and seeded
text banks instead (odise_amd/synthetic.py), which draws arbitrary segments but needs no file.
"""
from __future__ import annotations

import argparse
import os
import zlib
from typing import List, Optional, Sequence

import numpy as np


def parse_args(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m odise_amd.demo", description="Panoptic segmentation of pictures, drawn and saved as PNG.")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", nargs="+", metavar="FILE", help="pictures (JPEG is decoded on the device)")
    src.add_argument("--video-input", metavar="SRC", help="a directory of frames (sorted by name) or a multi-frame file Pillow opens")
    ap.add_argument("--output", required=True, metavar="DIR", help="directory for the drawn pictures (--video-input: or a .gif file)")
    ap.add_argument("--ttl", type=int, default=8, help="--video-input: frames an unseen thing keeps its colour for (1..8)")
    ap.add_argument("--track-masks", action="store_true", help="--video-input --task instance: keep an instance's colour from frame to frame by "
                    "mask IoU (detectron2's rule for instances without a box; the reference's zero boxes track nothing)")
    ap.add_argument("--track-boxes", action="store_true", help="--video-input --task instance: give the instances the boxes of their masks and keep "
                    "an instance's colour from frame to frame by box IoU above 0.6 (detectron2's rule for instances with a box); implies --draw-boxes")
    ap.add_argument("--draw-boxes", action="store_true", help="--task instance: give the instances the boxes of their masks and draw them as "
                    "detectron2 draws instances with boxes (a frame per box, the order by box area, the label on the box corner)")
    ap.add_argument("--vocab", default="", help='extra classes, demo.py style: "black pickup truck, pickup truck; blue sky, sky"')
    ap.add_argument("--synthetic", action="store_true", help="random weights of the real shapes and seeded text banks: needs no checkpoint")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--task", choices=("panoptic", "semantic", "instance"), default="panoptic",
                    help="which head is on and drawn (semantic-only vocabularies, or the instance masks segm AP scores)")
    ap.add_argument("--confidence-threshold", type=float, default=0.5, help="--task instance: instances below this score are not drawn")
    ap.add_argument("--tta", default=None, metavar="SIZES", help="--task semantic: average the semantic scores over these short-edge sizes "
                    '("768,1024,1280"), each also mirrored (multi-scale / flip test-time augmentation)')
    ap.add_argument("--no-tta-flip", action="store_true", help="--tta: the sizes only, no mirrored views")
    args = ap.parse_args(argv)
    if args.tta is not None:
        if args.task != "semantic":
            ap.error(f"--tta with --task {args.task}: test-time augmentation exists for the semantic head only")
        try:
            args.tta = tuple(int(v) for v in args.tta.split(","))
        except ValueError:
            ap.error(f"--tta {args.tta!r}: comma-separated short-edge sizes expected")
        if not args.tta or min(args.tta) < 1:
            ap.error("--tta: sizes must be positive")
        if args.video_input is not None:
            ap.error("--tta with --video-input: test-time augmentation runs on single pictures")
    elif args.no_tta_flip:
        ap.error("--no-tta-flip without --tta")
    if args.track_masks and args.video_input is None:
        ap.error("--track-masks without --video-input: single pictures have nothing to track")
    if args.track_masks and args.task != "instance":
        ap.error(f"--track-masks with --task {args.task}: mask tracking exists for the instance head only")
    if args.track_boxes and args.video_input is None:
        ap.error("--track-boxes without --video-input: single pictures have nothing to track")
    if args.track_boxes and args.task != "instance":
        ap.error(f"--track-boxes with --task {args.task}: box tracking exists for the instance head only")
    if args.track_boxes and args.track_masks:
        ap.error("--track-boxes with --track-masks: an instance is tracked by its box or by its mask, not both")
    if args.draw_boxes and args.task != "instance":
        ap.error(f"--draw-boxes with --task {args.task}: only the instances of the instance head carry boxes")
    args.draw_boxes = args.draw_boxes or args.track_boxes
    if args.video_input is not None and args.task == "instance" and not (args.track_masks or args.track_boxes):
        ap.error("--task instance with --video-input: the reference tracks pred_boxes there, which are all zeros on this model")
    if not 1 <= args.ttl <= 8:
        ap.error(f"--ttl {args.ttl} outside 1..8")
    return args


def extra_classes(vocab: str) -> List[List[str]]:
    """demo.py:330-334: classes separated by ';', the synonyms of a class by ','."""
    return [[s.strip() for s in c.split(",") if s.strip()] for c in vocab.split(";") if c.strip()]


def output_path(out_dir: str, file_name: str) -> str:
    return os.path.join(out_dir, os.path.splitext(os.path.basename(file_name))[0] + ".png")


def _palette(n: int, seed: int) -> list:
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in c) for c in rng.integers(32, 224, (n, 3))]


def demo_metadata(labels: List[List[str]], num_things: int) -> dict:
    """What demo.py builds with MetadataCatalog: the first synonym of a class is its name; things come first."""
    names = [l[0] for l in labels]
    return {"thing_classes": names[:num_things], "stuff_classes": names, "thing_colors": _palette(num_things, 1), "stuff_colors": _palette(len(names), 2),
            "thing_ids": list(range(num_things))}


class _SeededText:
    """--synthetic: stands in for tokenizer + CLIP text tower (no merges file, no weights): a prompt string -> a seeded random row."""

    def __call__(self, strings):
        return list(strings)

    def build_text_embed(self, strings):
        return np.stack([np.random.default_rng(zlib.crc32(s.encode())).standard_normal(768) for s in strings]).astype(np.float32)


def build_model(ctx, labels: List[List[str]], num_things: int, synthetic: bool, task: str = "panoptic"):
    from .pipeline import HipCategoryODISE, HipOpenPanopticInference
    if synthetic:
        from .synthetic import synthetic_state
        hip = HipCategoryODISE(ctx, synthetic_state(), overlap_threshold=0.0)
        text = _SeededText()
        hip.attach_text(text, text, train_labels=labels)
    else:
        from .checkpoint import assemble_state, load_openai_clip
        from .text import HipTextEncoder
        from .tokenizer import SimpleTokenizer
        hip = HipCategoryODISE(ctx, assemble_state(ctx), overlap_threshold=0.0)
        hip.attach_text(SimpleTokenizer(), HipTextEncoder(ctx, load_openai_clip("clip://ViT-L-14-336")))
    hip._alpha, hip._beta = 0.35, 0.65                                   # demo.py:316-318
    metadata = demo_metadata(labels, num_things)
    return HipOpenPanopticInference(hip, labels, metadata, semantic_on=task == "semantic", instance_on=task == "instance",
                                    panoptic_on=task == "panoptic"), metadata


def default_labels(extra: List[List[str]]):
    """(labels, number of things).  With the reference's label files at hand ($ODISE_OPENSEG_LABELS) the COCO panoptic vocabulary of
    demo.py's `--label COCO`; without them only the classes given with --vocab (demo.py treats those as things and puts them first)."""
    from .checkpoint import default_train_labels
    try:
        coco = default_train_labels()
    except FileNotFoundError:
        coco = []
    labels = extra + coco
    if not labels:
        raise SystemExit("no vocabulary: give classes with --vocab or point ODISE_OPENSEG_LABELS at the reference's label files")
    return labels, len(extra) + (80 if coco else 0)


def read_picture(ctx, file_name: str):
    """-> DeviceArray uint8 [h,w,3]"""
    from ._lib import UnsupportedInput
    from .ingest import HipDatasetMapper
    try:
        return HipDatasetMapper(ctx, None)({"file_name": file_name})["image"]
    except UnsupportedInput:
        from PIL import Image, ImageOps
        with Image.open(file_name) as im:
            return ctx.to_device(np.ascontiguousarray(np.asarray(ImageOps.exif_transpose(im).convert("RGB"), np.uint8)))


def video_frames(src: str) -> list:
    """[(name, loader)] of --video-input: the files of a directory in sorted name order (loader(ctx) = read_picture), or the frames of
    a multi-frame file as Pillow's ImageSequence yields them (name = "<file>#<index>")."""
    if os.path.isdir(src):
        names = sorted(f for f in os.listdir(src) if os.path.isfile(os.path.join(src, f)))
        return [(os.path.join(src, f), (lambda ctx, p=os.path.join(src, f): read_picture(ctx, p))) for f in names]
    from PIL import Image, ImageSequence
    with Image.open(src) as im:
        frames = [np.ascontiguousarray(np.asarray(f.convert("RGB"), np.uint8)) for f in ImageSequence.Iterator(im)]
    return [(f"{src}#{k}", (lambda ctx, a=a: ctx.to_device(a))) for k, a in enumerate(frames)]


def frame_path(out_dir: str, index: int) -> str:
    return os.path.join(out_dir, "frame_%06d.png" % index)


def run_on_video(ctx, model, visualizer, frames, task: str = "panoptic", confidence_threshold: float = 0.5, draw_boxes: bool = False,
                 track_boxes: bool = False):
    """VisualizationDemo.run_on_video (demo.py:201-243): yields the drawn frames.  visualizer: a HipVideoVisualizer (panoptic: its
    tracker colours the things; semantic: every frame on its own; instance: its mask tracker colours the instances, or with track_boxes its box tracker; draw_boxes: the instances carry and show the boxes of their masks).  A frame of another size than the first is refused by name."""
    size = None
    options = {"confidence_threshold": confidence_threshold} if task == "instance" else {}   # the only branch that reads it
    if draw_boxes or track_boxes:
        options.update(draw_boxes=True, track_boxes=track_boxes)
    for name, load in frames:
        image_dev = load(ctx)
        hw = tuple(image_dev.shape[:2])
        size = size or hw
        if hw != size:
            raise SystemExit(f"{name}: a {hw[0]}x{hw[1]} frame in a video of {size[0]}x{size[1]}")
        yield run_on_image(ctx, model, visualizer, image_dev, task, video=True, **options)


def run_on_image(ctx, model, visualizer, image_dev, task: str = "panoptic", confidence_threshold: float = 0.5,
                 video: bool = False, tta=None, draw_boxes: bool = False, track_boxes: bool = False) -> np.ndarray:
    """VisualizationDemo.run_on_image (demo.py:173-199) for a picture that is on the device; the result never leaves it before it is drawn."""
    from ._lib import record_len
    from .ingest import HipDatasetMapper
    h, w = image_dev.shape[:2]
    inputs = HipDatasetMapper(ctx, 1024, 2560)._finish({"height": h, "width": w}, image_dev)
    record = ctx.empty((record_len(h, w),), np.int32) if task == "panoptic" else None
    inner = model.model
    saved = inner.open_state_dict()
    inner.load_open_state_dict(model.open_state_dict)
    keep, rle, amax = inner.keep_instance_selection, inner.instance_rle, inner.semantic_argmax
    if task == "instance":
        inner.keep_instance_selection, inner.instance_rle = True, True       # the selection stays on the device; no dense mask tensor
    if task == "semantic":
        inner.semantic_argmax = True                                         # the fused arg-max map; no [K,h,w] tensor
    try:
        if tta is not None:                                                  # HipSemanticTTA over `model`: its own views of the picture
            results = tta.forward([{"image": image_dev, "height": h, "width": w}], to_host=False)
        else:
            results = inner.infer_device([inputs["image"]], 0, [tuple(inputs["image"].shape[:2])], [(h, w)],
                                         pan_out=[record] if record is not None else None)
    finally:
        inner.load_open_state_dict(saved)
        inner.keep_instance_selection, inner.instance_rle, inner.semantic_argmax = keep, rle, amax
    if task == "panoptic":
        draw = visualizer.draw_panoptic_seg_predictions if video else visualizer.draw_panoptic_seg
        return draw(image_dev, record, (h, w))
    picture = image_dev                                                      # the else branch: semantic, then instances on top
    if "sem_seg" in results[0] or "sem_seg_argmax" in results[0]:
        sem = results[0].get("sem_seg_argmax", results[0].get("sem_seg"))
        picture = ctx.to_device(visualizer.draw_sem_seg(picture, sem, inner.num_classes))
    if task == "instance":
        sel = inner.last_selection
        topk = sel["topk"]
        boxes = dict(boxes=True, **({"track_boxes": track_boxes} if video else {})) if draw_boxes else {}
        picture = visualizer.draw_instance_predictions(picture, 0, sel["inst_table"].view((1 + 2 * topk,), np.int32),
                                                       sel["inst_scores"].view((topk,), np.float32), topk, sel["pad_hw"], sel["img_hw"][0],
                                                       sel["out_hw"][0], min_score=confidence_threshold, **boxes)
    return picture if isinstance(picture, np.ndarray) else picture.numpy()


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse_args(argv)
    from PIL import Image
    from .runtime import Context
    from .visualize import HipVideoVisualizer, HipVisualizer
    labels, num_things = default_labels(extra_classes(args.vocab))
    ctx = Context(args.device)
    model, metadata = build_model(ctx, labels, num_things, args.synthetic, args.task)
    if args.video_input is not None:
        visualizer = HipVideoVisualizer(ctx, metadata, ttl=args.ttl)
        drawn = run_on_video(ctx, model, visualizer, video_frames(args.video_input), args.task, args.confidence_threshold, args.draw_boxes,
                             args.track_boxes)
        if args.output.lower().endswith(".gif"):
            os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
            pictures = [Image.fromarray(p) for p in drawn]
            if not pictures:
                raise SystemExit(f"{args.video_input}: no frames")
            pictures[0].save(args.output, save_all=True, append_images=pictures[1:], duration=100, loop=0)
            print(f"{args.video_input} -> {args.output} ({len(pictures)} frames)")
        else:
            os.makedirs(args.output, exist_ok=True)
            for k, picture in enumerate(drawn):
                Image.fromarray(picture).save(frame_path(args.output, k))
                print(f"{args.video_input} frame {k} -> {frame_path(args.output, k)}")
        visualizer.close()
        ctx.close()
        return 0
    visualizer = HipVisualizer(ctx, metadata)
    os.makedirs(args.output, exist_ok=True)
    tta = None
    if args.tta is not None:
        from .tta import HipSemanticTTA
        tta = HipSemanticTTA(model, args.tta, 2560, flip=not args.no_tta_flip)
    for file_name in args.input:
        picture = run_on_image(ctx, model, visualizer, read_picture(ctx, file_name), args.task, args.confidence_threshold, tta=tta,
                               draw_boxes=args.draw_boxes)
        Image.fromarray(picture).save(output_path(args.output, file_name))
        print(f"{file_name} -> {output_path(args.output, file_name)}")
    if tta is not None:
        tta.close()
    ctx.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
