// tta.hip — multi-scale / flip test-time augmentation of the semantic head (Mask2Former's SemanticSegmentorWithTTA: the picture at several
// short-edge sizes, each also mirrored, `sem_seg` averaged at the original size) without ever holding [K, h, w] per view.
//
// sem_seg = P^T sigmoid(masks) is linear in the (query, pixel) probabilities, so the sum over A views is ONE product over the views' query sets
// laid end to end:  sum_a sum_q P_a[q, k] S_a[q, pixel]  - depth A * Qpad.  A handle (odise_tta) keeps the operands of the views added so far:
//   S_cat  [oh*ow, max_views*Qpad] f16   view a in columns [a*Qpad, (a+1)*Qpad): fp16 sigmoid of the view's mask logits resampled to the output
//                                        size (sample_mask + post_sigmoid + sig_f16: the bits postprocess_pixels writes), at the mirrored
//                                        output column for a mirrored view
//   PT_cat [K, max_views*Qpad] f16       softmax(mask_cls)[:, :K]^T of the view in the same columns (post_decide_kernel's semT bits)
// tta_finish_kernel is semantic_argmax_kernel's MFMA form (class tile = row operand: classes along the registers, the pixel on the lane) with
// the depth walked in k-steps of 16 from memory instead of held in registers, and CT class tiles of accumulators per pass over a wave's S rows.
#include "post_sample.h"

struct odise_tta {
    int oh = 0, ow = 0, K = 0, Q = 0, Qpad = 0, max_views = 0, views = 0;
    int64_t ld = 0;              // max_views * Qpad: row pitch of both matrices
    odise::f16* S = nullptr;
    odise::f16* PT = nullptr;
};

namespace odise {

// One launch per view.  Blocks [0, pix_blocks): a thread per output pixel writes the view's Qpad columns of its S row (zeros past Q).  The
// blocks after them: a wavefront per query, post_decide_kernel's softmax (wave_softmax_stats / softmax_prob of post_sample.h: one definition,
// the same fp16 bits) into the view's columns of PT; its padding columns stay zero from odise_hip_tta_create.
__global__ void __launch_bounds__(256) tta_view_kernel(const f16* __restrict__ logits, const float* __restrict__ mask_cls, f16* __restrict__ S,
                                                      f16* __restrict__ PT, PostGeom g, int K, int64_t ld, int col0, int hflip, int pix_blocks) {
    const int Q = g.Q;
    if ((int)blockIdx.x < pix_blocks) {
        const int npix = g.oh * g.ow;
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= npix) return;
        const int oy = p / g.ow, ox = p - oy * g.ow;
        const int sx = hflip ? g.ow - 1 - ox : ox;
        const int plane = g.h4 * g.w4;
        f16* row = S + (int64_t)p * ld + col0;
        for (int q0 = 0; q0 < g.Qpad; q0 += 4) {   // 4 queries a step: 8 would hold 128 taps in flight (one wave per SIMD)
            f16x4 sv = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = q0 + j;
                if (q < Q) {  // uniform branch
                    const float v = sample_mask(logits + (int64_t)q * plane, g, oy, sx);
                    sv[j] = sig_f16(post_sigmoid(v), v);
                }
            }
            *reinterpret_cast<f16x4*>(row + q0) = sv;
        }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = ((int)blockIdx.x - pix_blocks) * 4 + wave;
    if (q >= Q) return;   // the whole wavefront
    const float* row = mask_cls + (int64_t)q * (K + 1);
    float m, ssum;
    wave_softmax_stats(row, K, lane, m, ssum);
    for (int k = lane; k < K; k += 64) PT[(int64_t)k * ld + col0 + q] = (f16)softmax_prob(row[k], m, ssum);
}

// A wave owns 32 pixels; a pass holds CT class tiles (32 classes each) of accumulators and walks the depth once: per k-step one 16-byte S
// fragment per lane and one PT fragment per class tile (PT_cat, <= 1.4 MB at K = 847 and 8 views, streams from L2).  ceil(K / (32 CT)) passes.
// The register footprint does not depend on the depth.  At one view the products and their order are semantic_argmax_kernel's (steps past the
// depth add 0 * 0 there), so the sums, and the first maximum, are bit-identical to it.
//   sem [K, npix] f32 = sums / views (a true fp32 division in the epilogue: one rounding);  out [npix] int32 = first maximum of the sums
template <int CT, bool SEM, bool AMAX>
__global__ void __launch_bounds__(256) tta_finish_kernel(const f16* __restrict__ S, const f16* __restrict__ PT, float* __restrict__ sem,
                                                        int* __restrict__ out, int npix, int64_t ld, int depth, int K, float views) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int64_t p = ((int64_t)blockIdx.x * 4 + wave) * 32 + l31;
    const bool pok = p < npix;
    const f16* srow = S + (pok ? p : 0) * ld + hi * 8;
    const int nks = (depth + 15) >> 4;
    float best = -INFINITY;
    int best_k = 0;
    for (int c0 = 0; c0 < K; c0 += 32 * CT) {
        f32x16 acc[CT];
        const f16* prow[CT];
#pragma unroll
        for (int t = 0; t < CT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
            const int c = c0 + 32 * t + l31;
            prow[t] = PT + (int64_t)(c < K ? c : K - 1) * ld + hi * 8;
        }
        for (int ks = 0; ks < nks; ++ks) {
            const int ko = ks * 16;
            const bool inr = ko + hi * 8 + 8 <= depth;
            f16x8 pf = {0, 0, 0, 0, 0, 0, 0, 0};
            if (pok && inr) pf = *reinterpret_cast<const f16x8*>(srow + ko);
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                if (c0 + 32 * t < K) {   // uniform
                    f16x8 cf = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (c0 + 32 * t + l31 < K && inr) cf = *reinterpret_cast<const f16x8*>(prow[t] + ko);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cf, pf, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            if (c0 + 32 * t < K) {   // uniform
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int cls = c0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hi;   // ascending in t, r: `>` keeps the first maximum
                    if (cls < K) {
                        if (SEM && pok) sem[(int64_t)cls * npix + p] = acc[t][r] / views;
                        if (AMAX && acc[t][r] > best) { best = acc[t][r]; best_k = cls; }
                    }
                }
            }
        }
    }
    if (AMAX) {
        const float ob = __shfl_xor(best, 32);
        const int ok = __shfl_xor(best_k, 32);
        if (ob > best || (ob == best && ok < best_k)) { best = ob; best_k = ok; }
        if (hi == 0 && pok) out[p] = best_k;
    }
}

// dst[y, x, :] = src[y, W - 1 - x, :] (HFlipTransform on the uint8 HWC picture): a thread per byte, coalesced on the store side
__global__ void __launch_bounds__(256) hflip_u8_hwc_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int C) {
    const int64_t n = (int64_t)H * W * C;
    const int64_t rowb = (int64_t)W * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t y = i / rowb, r = i - y * rowb;
        const int x = (int)(r / C), c = (int)(r - (int64_t)x * C);
        dst[i] = src[y * rowb + (int64_t)(W - 1 - x) * C + c];
    }
}

template <int CT>
static void launch_finish(odise_hip_ctx* ctx, const odise_tta* t, float* sem, int* amax) {
    const int npix = t->oh * t->ow, depth = t->views * t->Qpad;
    const dim3 grid((unsigned)ceil_div(npix, 128)), block(256);
    const float views = (float)t->views;
    if (sem && amax) hipLaunchKernelGGL((tta_finish_kernel<CT, true, true>), grid, block, 0, ctx->stream, t->S, t->PT, sem, amax, npix, t->ld, depth, t->K, views);
    else if (sem) hipLaunchKernelGGL((tta_finish_kernel<CT, true, false>), grid, block, 0, ctx->stream, t->S, t->PT, sem, amax, npix, t->ld, depth, t->K, views);
    else hipLaunchKernelGGL((tta_finish_kernel<CT, false, true>), grid, block, 0, ctx->stream, t->S, t->PT, sem, amax, npix, t->ld, depth, t->K, views);
}

static void tta_free(odise_tta* t) {
    if (t->S) (void)hipFree(t->S);
    if (t->PT) (void)hipFree(t->PT);
    delete t;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_tta_create(odise_hip_ctx* ctx, int out_h, int out_w, int K, int Q, int max_views, odise_tta** out) {
    ODISE_REQUIRE(ctx, "tta_create: null context");
    ODISE_REQUIRE(out, "tta_create: null pointer");
    ODISE_REQUIRE(out_h >= 1 && out_w >= 1 && (int64_t)out_h * out_w < (1ll << 30), "tta_create: bad output size %dx%d", out_h, out_w);
    ODISE_REQUIRE(K >= 1 && K <= 65536 && Q >= 1 && Q <= 304 && max_views >= 1 && max_views <= 64, "tta_create: K %d / Q %d / max_views %d out of range", K, Q,
                  max_views);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const int Qpad = (int)round_up(Q, 8);
    const int64_t ld = (int64_t)max_views * Qpad;
    const size_t s_bytes = (size_t)out_h * out_w * ld * sizeof(f16), pt_bytes = (size_t)K * ld * sizeof(f16);
    size_t free_b = 0, total_b = 0;
    ODISE_CHECK_HIP(hipMemGetInfo(&free_b, &total_b));
    ODISE_REQUIRE(s_bytes + pt_bytes <= free_b, "tta_create: %zu bytes for %d views of %d queries at %dx%d, %zu free", s_bytes + pt_bytes, max_views, Q, out_h,
                  out_w, free_b);
    odise_tta* t = new odise_tta();
    t->oh = out_h; t->ow = out_w; t->K = K; t->Q = Q; t->Qpad = Qpad; t->max_views = max_views; t->ld = ld;
    if (hipMalloc((void**)&t->S, s_bytes) != hipSuccess || hipMalloc((void**)&t->PT, pt_bytes) != hipSuccess) {
        (void)hipGetLastError();
        tta_free(t);
        set_error("tta_create: could not allocate %zu bytes", s_bytes + pt_bytes);
        return ODISE_ERR_NOMEM;
    }
    if (hipMemsetAsync(t->PT, 0, pt_bytes, ctx->stream) != hipSuccess) {   // the padding columns [Q, Qpad) of every view: never written again
        (void)hipGetLastError();
        tta_free(t);
        set_error("tta_create: clearing the class matrix failed");
        return ODISE_ERR_HIP;
    }
    *out = t;
    return ODISE_OK;
}

extern "C" int odise_hip_tta_reset(odise_hip_ctx* ctx, odise_tta* tta) {
    ODISE_REQUIRE(ctx, "tta_reset: null context");
    ODISE_REQUIRE(tta, "tta_reset: null handle");
    tta->views = 0;   // the next views overwrite the columns in stream order
    return ODISE_OK;
}

extern "C" int odise_hip_tta_destroy(odise_hip_ctx* ctx, odise_tta* tta) {
    ODISE_REQUIRE(ctx, "tta_destroy: null context");
    ODISE_REQUIRE(tta, "tta_destroy: null handle");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    ODISE_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // views / a finish in flight use its memory
    tta_free(tta);
    return ODISE_OK;
}

extern "C" int odise_hip_tta_add_view(odise_hip_ctx* ctx, odise_tta* tta, int b, const float* mask_cls_b, int pad_h, int pad_w, int img_h, int img_w,
                                      int hflip) {
    ODISE_REQUIRE(ctx, "tta_add_view: null context");
    ODISE_REQUIRE(tta && mask_cls_b, "tta_add_view: null pointer");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    ModelStore* ms = store_of(ctx);
    HeadOutputs ho;
    ODISE_TRY(head_outputs(ms, &ho));
    const int K = classify_num_classes(ms);
    if (K <= 0) {
        set_error("tta_add_view: call odise_hip_classify_build and odise_hip_set_vocabulary first");
        return ODISE_ERR_STATE;
    }
    ODISE_REQUIRE(tta->views < tta->max_views, "tta_add_view: the handle holds its %d views already", tta->max_views);
    ODISE_REQUIRE(K == tta->K && ho.Q == tta->Q, "tta_add_view: %d classes / %d queries for a handle of %d / %d", K, ho.Q, tta->K, tta->Q);
    ODISE_REQUIRE(b >= 0 && b < ho.B, "tta_add_view: image index %d out of range", b);
    // the padded size the logits were produced at, as odise_hip_postprocess_batch asks: a stale geometry (another view's) is refused, not resampled
    ODISE_REQUIRE(pad_h == 4 * ho.h4 && pad_w == 4 * ho.w4, "tta_add_view: padded size %dx%d does not match the mask logits (%dx%d x 4)", pad_h, pad_w,
                  ho.h4, ho.w4);
    ODISE_REQUIRE(img_h >= 1 && img_w >= 1 && img_h <= pad_h && img_w <= pad_w, "tta_add_view: bad geometry (image %dx%d, padded %dx%d)", img_h, img_w, pad_h,
                  pad_w);
    PostGeom g;
    g.h4 = ho.h4; g.w4 = ho.w4; g.ph = pad_h; g.pw = pad_w; g.ih = img_h; g.iw = img_w; g.oh = tta->oh; g.ow = tta->ow;
    g.Q = tta->Q; g.Qpad = tta->Qpad;
    const int pix_blocks = (int)ceil_div((int64_t)g.oh * g.ow, 256);
    const f16* logits = ho.pred_masks + (size_t)b * ho.Q * ho.h4 * ho.w4;
    hipLaunchKernelGGL(tta_view_kernel, dim3((unsigned)(pix_blocks + ceil_div(g.Q, 4))), dim3(256), 0, ctx->stream, logits, mask_cls_b, tta->S, tta->PT, g, K,
                       tta->ld, tta->views * tta->Qpad, hflip ? 1 : 0, pix_blocks);
    ODISE_CHECK_HIP(hipGetLastError());
    ++tta->views;
    return ODISE_OK;
}

extern "C" int odise_hip_tta_finish(odise_hip_ctx* ctx, odise_tta* tta, float* sem_seg, int* sem_argmax) {
    ODISE_REQUIRE(ctx, "tta_finish: null context");
    ODISE_REQUIRE(tta, "tta_finish: null handle");
    ODISE_REQUIRE(sem_seg || sem_argmax, "tta_finish: neither sem_seg nor sem_argmax");
    ODISE_REQUIRE(tta->views >= 1, "tta_finish: no view added");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    store_of(ctx)->macs += (double)tta->K * tta->oh * tta->ow * tta->views * tta->Qpad;
    if (tta->K <= 160) launch_finish<5>(ctx, tta, sem_seg, sem_argmax);   // every class in one pass over S
    else launch_finish<6>(ctx, tta, sem_seg, sem_argmax);   // two waves per SIMD still (8 tiles: one)
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

#ifdef ODISE_TOOLS
// Measurement build only (include/odise_hip_lab.h, tools/tta_bench.py): semantic_argmax_kernel on the operands of a ONE-view handle (row pitch
// Qpad: the layout that kernel takes), so both kernels are timed on the same bits.
extern "C" int odise_hip_lab_tta_single_argmax(odise_hip_ctx* ctx, odise_tta* tta, int* sem_argmax) {
    ODISE_REQUIRE(ctx && tta && sem_argmax, "lab_tta_single_argmax: null pointer");
    ODISE_REQUIRE(tta->max_views == 1 && tta->views == 1, "lab_tta_single_argmax: a handle of one view, added");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    return launch_semantic_argmax(ctx, tta->S, tta->PT, sem_argmax, tta->oh * tta->ow, tta->Qpad, tta->K);
}
#endif

extern "C" int odise_hip_hflip_u8_hwc(odise_hip_ctx* ctx, const void* src, void* dst, int H, int W, int C) {
    ODISE_REQUIRE(ctx, "hflip_u8_hwc: null context");
    ODISE_REQUIRE(src && dst && src != dst, "hflip_u8_hwc: null or aliased pointer");
    ODISE_REQUIRE(H >= 1 && W >= 1 && C >= 1 && (int64_t)H * W * C < (1ll << 31), "hflip_u8_hwc: bad shape %dx%dx%d", H, W, C);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(hflip_u8_hwc_kernel, dim3((unsigned)grid_blocks(ctx, (int64_t)H * W * C, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)src,
                       (uint8_t*)dst, H, W, C);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
