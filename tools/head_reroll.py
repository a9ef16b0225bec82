"""Does a change of summation order in the head re-roll which query one of the masked decoder's hard decisions sends the other way - or degrade the
head?  The full-size head on the ORACLE's backbone features (tests/fullsize.py, picture 0) under four arithmetic-equivalent configurations of the
library: fused / two-kernel MSDeformAttn x GroupNorm statistics in 2 / 8 chunks per CU.  Per configuration: worst query, queries beyond 2.5e-2 of
max|logit|, the 99.9 % pixel quantile, the same quantile over the regular queries only, mask_embed error.          (GPU; ~3 min of host oracle time)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fullsize import build_models, export_state, reference  # noqa: E402
from odise_amd.pipeline import HipCategoryODISE  # noqa: E402
from odise_amd.runtime import Context  # noqa: E402

torch.set_num_threads(min(32, torch.get_num_threads()))
ctx = Context(0)
ext, bb, head = build_models()
img, heads, r = reference(bb, head, ext, 1024, 133, 254)
hip = HipCategoryODISE(ctx, export_state(ext, bb, head, heads), overlap_threshold=0.8)
feats = {k: r[k].numpy() for k in ("s2", "s3", "s4", "s5")}
ref = r["pred_masks"][0].numpy()
scale = np.abs(ref).max()
for msda_unfused in (0, 1):
    for chunks in (2, 8):
        ctx.lib.odise_hip_msda_unfused(msda_unfused)
        ctx.lib.odise_hip_gn_tuning(chunks)
        got = hip.head(feats)
        err = np.abs(got["pred_masks"][0] - ref) / scale
        q = err.reshape(100, -1).max(1)
        reg = q < 2.5e-2
        me = np.abs(got["mask_embed"] - r["mask_embed"].numpy()).max() / np.abs(r["mask_embed"].numpy()).max()
        print(f"MSDeformAttn {'two kernels' if msda_unfused else 'fused      '} | GroupNorm chunks/CU {chunks}: worst query {q.max():.2e} (query {int(q.argmax())}), beyond 2.5e-2: {int((~reg).sum())}, "
              f"median query {np.median(q):.2e}, p99.9 of all pixels {np.quantile(err.reshape(-1)[::7], 0.999):.2e}, of the regular queries {np.quantile(err[reg].reshape(-1)[::7], 0.999):.2e}, "
              f"mask_embed {me:.2e}", flush=True)
ctx.lib.odise_hip_msda_unfused(0)
ctx.lib.odise_hip_gn_tuning(2)
