"""The small synthetic CategoryODISE of the device tests (the graph of the full model at narrow widths: UNet / VAE width divided,
a two-layer CLIP, the small mask head with 20 queries) and its seeded test pictures.  Shared by tests/test_gpu_instance_rle.py and
tools/rle_bench.py; tests/test_gpu_model.py builds the same model inline."""
import torch

from odise_amd.pipeline import HipCategoryODISE
from oracle import odise_model as om
from oracle.backbone import FeatureExtractorBackbone
from oracle.ldm_extractor import ImplicitCaptionerExtractor
from oracle.m2f import SemSegHead, init_synthetic_

SMALL = dict(unet_div=5, vae_div=4, clip_kw=dict(image_size=336, patch_size=14, width=128, layers=2, heads=2, output_dim=64))
GROUPS = [1, 2, 1, 3, 1, 1, 2, 1, 1, 2, 1]
THINGS = {0, 2, 3, 5, 8}


def build_small(ctx, **kwargs) -> HipCategoryODISE:
    """The device model with its vocabulary set; kwargs go to HipCategoryODISE (default overlap_threshold 0)."""
    ext = ImplicitCaptionerExtractor(**SMALL)
    bb = FeatureExtractorBackbone(ext, [128, 128, 512, 384, 192, 128, 128, 128])
    head = init_synthetic_(SemSegHead(small=True, num_classes=len(GROUPS)))
    heads = om.OpenVocabHeads(ext.clip, GROUPS, projection_dim=64)
    state = ext.export_state()
    state.update({"backbone.feature_projections." + k: v for k, v in bb.feature_projections.state_dict().items()})
    state.update({"sem_seg_head." + k: v for k, v in head.state_dict().items()})
    state["category_head.text_proj.weight"] = heads.text_proj.weight.detach()
    state["category_head.text_proj.bias"] = heads.text_proj.bias.detach()
    state["category_head.null_embed"] = heads.null_embed.detach()
    hip = HipCategoryODISE(ctx, state, **{"overlap_threshold": 0.0, **kwargs})
    hip.set_vocabulary(heads.text_embed.numpy(), heads.clip_text_embed.numpy(), GROUPS, heads.category_overlapping_mask.numpy(), THINGS,
                       heads.alpha, heads.beta)
    return hip


def image_u8(h, w, seed=0):
    """Seeded, box-filtered uint8 CHW picture."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, h, w, generator=g)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(x, (4, 4, 4, 4), mode="reflect"), 9, stride=1)
    x = (x - x.amin()) / (x.amax() - x.amin())
    return (x[0] * 255).round().to(torch.uint8)
