// post_sample.h — the mask-logit resampling of the post-processing stage (odise.py:326-331 + sem_seg_postprocess), shared by the kernels that
// threshold it: classify_ops.hip (per-pixel pass, instance masks) and rle.hip (COCO RLE of the instance masks).  One definition, so every
// consumer sees the same bits.
#pragma once
#include "engine.h"

namespace odise {

__device__ __forceinline__ void bil_setup(int o, int in, int out, int& i0, int& i1, float& t) {
    float s = ((float)o + 0.5f) * ((float)in / (float)out) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    t = s - (float)i0;
}

__device__ __forceinline__ float sample_stage1(const f16* lr, int w4, int h4, int y, int x, int ph, int pw) {
    int y0, y1, x0, x1;
    float ty, tx;
    bil_setup(y, h4, ph, y0, y1, ty);
    bil_setup(x, w4, pw, x0, x1, tx);
    const float v00 = (float)lr[y0 * w4 + x0], v01 = (float)lr[y0 * w4 + x1], v10 = (float)lr[y1 * w4 + x0], v11 = (float)lr[y1 * w4 + x1];
    const float top = v00 + tx * (v01 - v00), bot = v10 + tx * (v11 - v10);
    return top + ty * (bot - top);
}

// logit of query q at output pixel (oy, ox): bilinear(crop(bilinear(logits -> padded size)) -> output size)
__device__ __forceinline__ float sample_mask(const f16* lr, const PostGeom& g, int oy, int ox) {
    if (g.oh == g.ih && g.ow == g.iw) return sample_stage1(lr, g.w4, g.h4, oy, ox, g.ph, g.pw);
    int y0, y1, x0, x1;
    float ty, tx;
    bil_setup(oy, g.ih, g.oh, y0, y1, ty);
    bil_setup(ox, g.iw, g.ow, x0, x1, tx);
    const float v00 = sample_stage1(lr, g.w4, g.h4, y0, x0, g.ph, g.pw), v01 = sample_stage1(lr, g.w4, g.h4, y0, x1, g.ph, g.pw);
    const float v10 = sample_stage1(lr, g.w4, g.h4, y1, x0, g.ph, g.pw), v11 = sample_stage1(lr, g.w4, g.h4, y1, x1, g.ph, g.pw);
    const float top = v00 + tx * (v01 - v00), bot = v10 + tx * (v11 - v10);
    return top + ty * (bot - top);
}

// The exact 4x upsampling (output = image size, padded size = 4 x logits) in the tap form of instance_masks_x4_kernel: output row oy = 4 cy + ky
// blends logit rows ra / rb with weight ty, a cell column cx gives four pixels k = 0..3 from the columns (cl, cx) (k < 2) or (cx, cr) (k >= 2).
__device__ __forceinline__ void x4_rows(const PostGeom& g, int oy, int& ra, int& rb, float& ty) {
    const int cy = oy >> 2, ky = oy & 3;
    ra = max(ky < 2 ? cy - 1 : cy, 0);
    rb = min(ky < 2 ? cy : cy + 1, g.h4 - 1);
    ty = ky == 0 ? 0.625f : ky == 1 ? 0.875f : ky == 2 ? 0.125f : 0.375f;
}
// the neighbour columns of cell column cx (a lane past the row's last cell column passes the clamped one: every load stays in range)
__device__ __forceinline__ void x4_cols(const PostGeom& g, int cx, int& cl, int& cr) {
    cl = max(cx - 1, 0);
    cr = min(cx + 1, g.w4 - 1);
}
// pixel k of a cell column from its six taps (a* on row ra, b* on row rb; l / c / r = columns cl, cx, cr): the value every x4 consumer thresholds -
// both x4 forms of the per-pixel pass, instance_masks_x4_kernel and rle_pack_x4_kernel
__device__ __forceinline__ float x4_pixel(int k, float ty, float al, float ac, float ar, float bl, float bc, float br) {
    const float tx = k == 0 ? 0.625f : k == 1 ? 0.875f : k == 2 ? 0.125f : 0.375f;
    const float v00 = k < 2 ? al : ac, v01 = k < 2 ? ac : ar, v10 = k < 2 ? bl : bc, v11 = k < 2 ? bc : br;
    const float top = v00 + tx * (v01 - v00), bot = v10 + tx * (v11 - v10);
    return top + ty * (bot - top);
}

}  // namespace odise
