// post_sample.h — the mask-logit resampling of the post-processing stage (odise.py:326-331 + sem_seg_postprocess), shared by the kernels that
// threshold it: classify_ops.hip (per-pixel pass, instance masks), rle.hip (COCO RLE of the instance masks) and tta.hip (the views' sigmoid matrices).  One definition, so every
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

// sigmoid of the per-pixel pass: v_exp_f32 + v_rcp_f32 (1 ulp each) instead of the library expf and the IEEE division (~20 VALU
// instructions less per pixel and query, of ~70); the result is rounded to fp16 for S and compared against 0.5 for the panoptic flag, both far
// coarser.  All three forms of the pass (generic, x4, tiled) share it, so they stay bit-identical to each other.
__device__ __forceinline__ float post_sigmoid(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

// fp16 sigmoid for the pixel-major matrix S.  The instance head counts a pixel as inside the mask iff its LOGIT is positive
// (maskformer_model.py:371 `mask_pred > 0`) and averages sigmoid over exactly those pixels (:376-377); sigmoid(v) for |v| < ~1e-3 rounds to
// 0.5 in fp16 on either side of zero, so a non-positive logit never gets more than the last fp16 value below 0.5 (and a positive one never less
// than 0.5): `S >= 0.5` then reproduces `logit > 0` exactly, and no value moves by more than one fp16 step of its own size - the semantic
// scores, which read the same matrix, keep the 2^-11 relative error of a plain rounding.  (Lifting the positive side to the next value ABOVE
// 0.5 instead cost those pixels 2^-10: tests/test_gpu_postprocess.py, generic geometry.)
__device__ __forceinline__ f16 sig_f16(float sg, float v) {
    const f16 h = (f16)sg;
    const f16 half = (f16)0.5f, below = (f16)0.499755859375f;
    return v > 0.f ? (h < half ? half : h) : (h > below ? below : h);   // selects, no branch
}

// F.softmax over one query's K + 1 log-probabilities (maskformer_model.py:287) by one wavefront: the row's maximum and the sum of the
// exponentials in every lane, then softmax_prob per entry.  post_decide_kernel (semT, the A operand of the semantic product) and
// tta_view_kernel (a view's columns of PT_cat) share it, so both hold the same fp16 bits.
__device__ __forceinline__ void wave_softmax_stats(const float* __restrict__ row, int K, int lane, float& m, float& ssum) {
    m = -INFINITY;
    for (int k = lane; k <= K; k += 64) m = fmaxf(m, row[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    ssum = 0.f;
    for (int k = lane; k <= K; k += 64) ssum += expf(row[k] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o);
}
__device__ __forceinline__ float softmax_prob(float x, float m, float ssum) { return expf(x - m) / ssum; }

}  // namespace odise
