"""The YTVIS file pairs of the front-door tests (tests/test_video_eval_cpu.py, tests/test_gpu_video_eval.py)."""
import json

import numpy as np

from odise_amd import coco_rle

STAT_NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]


def box(h, w, y0, y1, x0, x1):
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    return m


def write_pair(tmp_path, perfect: bool, crowded: bool = False):
    """Two videos (12 x 10; three and two frames), two categories, three ground-truth tracks -> (results path, annotation path).
    perfect: the results are the ground truth's own masks, else there are none.  crowded: a third video with ground truth and no
    result, and 130 more results in the first video (80 of one category, 50 of the other: more than 100 tracks, so the video is walked
    in two parts), boxes that overlap the ground truth by varying amounts, with score ties."""
    h, w = 12, 10
    masks = {1: [box(h, w, 0, 5, 0, 5), box(h, w, 1, 6, 1, 6), None], 2: [None, box(h, w, 6, 12, 4, 10), box(h, w, 6, 11, 4, 9)],
             3: [box(h, w, 2, 9, 2, 8), box(h, w, 2, 9, 3, 9)], 4: [box(h, w, 1, 4, 1, 9)]}
    enc = lambda m: None if m is None else coco_rle.encode(m)
    anns = [{"id": 1, "video_id": 10, "category_id": 4, "iscrowd": 0, "segmentations": [enc(m) for m in masks[1]], "areas": [25, 25, None]},
            {"id": 2, "video_id": 10, "category_id": 9, "iscrowd": 0, "segmentations": [enc(m) for m in masks[2]], "areas": [None, 36, 25]},
            {"id": 3, "video_id": 20, "category_id": 4, "iscrowd": 0, "segmentations": [enc(m) for m in masks[3]], "areas": [42, 42]}]
    videos = [{"id": 10, "height": h, "width": w, "length": 3}, {"id": 20, "height": h, "width": w, "length": 2}]
    res = [{"video_id": a["video_id"], "score": .9 - .1 * k, "category_id": a["category_id"], "segmentations": a["segmentations"]}
           for k, a in enumerate(anns)] if perfect else []
    if crowded:
        videos.append({"id": 30, "height": h, "width": w, "length": 1})
        anns.append({"id": 4, "video_id": 30, "category_id": 9, "iscrowd": 0, "segmentations": [enc(masks[4][0])], "areas": [24]})
        rng = np.random.default_rng(5)
        for k in range(130):
            cat, base = (4, masks[1]) if k < 80 else (9, masks[2])
            segs = []
            for m in base:
                dy, dx = rng.integers(-2, 3, 2)
                segs.append(None if m is None or rng.random() < .2 else enc(np.roll(np.roll(m, dy, axis=0), dx, axis=1)))
            res.append({"video_id": 10, "score": float(rng.integers(1, 9)) / 10, "category_id": cat, "segmentations": segs})
    gt = {"videos": videos, "categories": [{"id": 4, "name": "cat"}, {"id": 9, "name": "dog"}], "annotations": anns}
    gp, rp = tmp_path / "gt.json", tmp_path / ("perfect.json" if perfect else "empty.json")
    gp.write_text(json.dumps(gt))
    rp.write_text(json.dumps(res))
    return str(rp), str(gp)
