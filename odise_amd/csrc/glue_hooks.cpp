// glue_hooks.cpp — test hooks (include/odise_hip_tools.h) of the small kernels between the GEMM stages: decoder_ops.hip, misc.hip and the head of
// classify_ops.hip, one extern "C" function per launch_* of engine.h.  Each validates what the host can see (pointers, sizes, the 8-channel and
// 16-byte rules of the kernels), launches on the context's stream and returns the usual code; nothing on the product path calls them
// (tests/test_gpu_glue_ops.py does).  The fp32 mask_binarize hook lives beside its kernel in elementwise.hip.
#include "engine.h"
#include "../../include/odise_hip_tools.h"

using namespace odise;

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int odise_hip_crop_extract(odise_hip_ctx* ctx, const float* img, float* crops, int B, int C, int H, int W, int S, int K, const int* boxes_dev) {
    ODISE_REQUIRE(ctx && img && crops && boxes_dev && B >= 1 && C >= 1 && K >= 1 && S >= 1 && S <= H && S <= W, "crop_extract: bad argument");
    return launch_crop_extract(ctx, img, crops, B, C, H, W, S, K, boxes_dev);
}

extern "C" int odise_hip_crop_resize_bicubic(odise_hip_ctx* ctx, const float* img, float* crops, int B, int C, int H, int W, int s, int S, int K,
                                             const int* boxes_dev) {
    ODISE_REQUIRE(ctx && img && crops && boxes_dev && B >= 1 && C >= 1 && K >= 1 && S >= 1 && s >= 1 && s <= H && s <= W,
                  "crop_resize_bicubic: bad argument");
    return launch_crop_resize_bicubic(ctx, img, crops, B, C, H, W, s, S, K, boxes_dev);
}

extern "C" int odise_hip_clip_preprocess(odise_hip_ctx* ctx, const float* image01, void* out_f16, int N, int H, int W, int S) {
    ODISE_REQUIRE(ctx && image01 && out_f16 && al16(out_f16) && N >= 1 && H >= 1 && W >= 1 && S >= 1, "clip_preprocess: bad argument");
    return launch_clip_preprocess(ctx, image01, (f16*)out_f16, N, H, W, S);
}

extern "C" int odise_hip_resize_bilinear_norm(odise_hip_ctx* ctx, const float* image01, void* out_f16, int B, int H, int W, int S) {
    ODISE_REQUIRE(ctx && image01 && out_f16 && al16(out_f16) && B >= 1 && H >= 1 && W >= 1 && S >= 1, "resize_bilinear_norm: bad argument");
    return launch_resize_bilinear_norm(ctx, image01, (f16*)out_f16, B, H, W, S);
}

extern "C" int odise_hip_upsample_nearest(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int N, int H, int W, int OH, int OW, int C) {
    ODISE_REQUIRE(ctx && x_f16 && y_f16 && al16(x_f16) && al16(y_f16) && N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && C >= 8 && C % 8 == 0,
                  "upsample_nearest: bad argument");
    return launch_upsample_nearest(ctx, (const f16*)x_f16, (f16*)y_f16, N, H, W, OH, OW, C);
}

extern "C" int odise_hip_stitch(odise_hip_ctx* ctx, const void* feat_f16, void* out_f16, float* out_nchw, int B, int K, const int* boxes_dev, int ch, int cw,
                                int OH, int OW, int C) {
    ODISE_REQUIRE(ctx && feat_f16 && (out_f16 || out_nchw) && boxes_dev && al16(feat_f16) && al16(out_f16) && B >= 1 && K >= 1 && ch >= 1 && cw >= 1 &&
                      OH >= 1 && OW >= 1 && C >= 8 && C % 8 == 0,
                  "stitch: bad argument");
    return launch_stitch(ctx, (const f16*)feat_f16, (f16*)out_f16, out_nchw, B, K, boxes_dev, ch, cw, OH, OW, C);
}

extern "C" int odise_hip_add_vec_table(odise_hip_ctx* ctx, const void* x_f16, const float* vec, const float* table, void* y_f16, int64_t N, int P, int C) {
    ODISE_REQUIRE(ctx && x_f16 && y_f16 && al16(x_f16) && al16(y_f16) && N >= 1 && P >= 1 && C >= 8 && C % 8 == 0, "add_vec_table: bad argument");
    return launch_add_vec_table(ctx, (const f16*)x_f16, vec, table, (f16*)y_f16, N, P, C);
}

extern "C" int odise_hip_broadcast_rows(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int64_t n, int B) {
    ODISE_REQUIRE(ctx && x_f16 && y_f16 && al16(x_f16) && al16(y_f16) && n >= 8 && n % 8 == 0 && B >= 1, "broadcast_rows: bad argument");
    return launch_broadcast_rows(ctx, (const f16*)x_f16, (f16*)y_f16, n, B);
}

extern "C" int odise_hip_bilinear_add(odise_hip_ctx* ctx, const void* a_f16, const void* b_f16, void* y_f16, int N, int H, int W, int OH, int OW, int C) {
    ODISE_REQUIRE(ctx && b_f16 && y_f16 && al16(a_f16) && al16(b_f16) && al16(y_f16) && N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1 && C >= 8 &&
                      C % 8 == 0,
                  "bilinear_add: bad argument");
    return launch_bilinear_add(ctx, (const f16*)a_f16, (const f16*)b_f16, (f16*)y_f16, N, H, W, OH, OW, C);
}

extern "C" int odise_hip_mask_binarize_f16(odise_hip_ctx* ctx, const void* mask_f16, void* m01_f16, float* inv, int64_t rows, int HW) {
    ODISE_REQUIRE(ctx && mask_f16 && m01_f16 && inv && al16(mask_f16) && al16(m01_f16) && rows >= 1 && rows < (1ll << 31) && HW >= 8,
                  "mask_binarize_f16: bad argument");
    return launch_mask_binarize_f16(ctx, (const f16*)mask_f16, (f16*)m01_f16, inv, rows, HW);
}

extern "C" int odise_hip_attn_mask(odise_hip_ctx* ctx, const void* logits, int dtype, void* out_u8, int64_t rows, int H, int W, int oh, int ow, int64_t ldm) {
    ODISE_REQUIRE(ctx && logits && out_u8 && (dtype == ODISE_F16 || dtype == ODISE_F32) && rows >= 1 && rows < (1ll << 31) && H >= 1 && W >= 1 && oh >= 1 &&
                      ow >= 1 && ldm >= (int64_t)oh * ow,
                  "attn_mask: bad argument");
    if (dtype == ODISE_F16) return launch_attn_mask(ctx, (const f16*)logits, (uint8_t*)out_u8, rows, H, W, oh, ow, ldm);
    return launch_attn_mask_f32(ctx, (const float*)logits, (uint8_t*)out_u8, rows, H, W, oh, ow, ldm);
}

extern "C" int odise_hip_softmax_rows(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int64_t rows, int cols, int64_t ld, float scale) {
    ODISE_REQUIRE(ctx && x_f16 && y_f16 && al16(x_f16) && al16(y_f16) && rows >= 1 && rows < (1ll << 31) && cols >= 1 && ld >= cols,
                  "softmax_rows: bad argument");
    return launch_softmax_rows(ctx, (const f16*)x_f16, (f16*)y_f16, rows, cols, ld, scale);
}

extern "C" int odise_hip_clip_assemble(odise_hip_ctx* ctx, const void* patches_f16, const float* cls, const float* pos, void* tok_f16, int B, int T, int extra,
                                       int TP, int Cw) {
    ODISE_REQUIRE(ctx && patches_f16 && cls && pos && tok_f16 && al16(patches_f16) && al16(tok_f16) && B >= 1 && T >= 2 && extra >= 0 && Cw >= 8 &&
                      Cw % 8 == 0,
                  "clip_assemble: bad argument");
    return launch_clip_assemble(ctx, (const f16*)patches_f16, cls, pos, (f16*)tok_f16, B, T, extra, TP, Cw);
}

extern "C" int odise_hip_cond_inputs(odise_hip_ctx* ctx, const float* proj, const float* A1, const float* A2, float* out, int B, int T, int Cw) {
    ODISE_REQUIRE(ctx && proj && A1 && A2 && out && B >= 1 && T >= 1 && Cw >= 1, "cond_inputs: bad argument");
    return launch_cond_inputs(ctx, proj, A1, A2, out, B, T, Cw);
}

extern "C" int odise_hip_latent_heads(odise_hip_ctx* ctx, const void* h_f16, const float* noise, void* xt_f16, void* zdec_f16, float* latent, int B, int P,
                                      const float* wq_4x8, const float* bq_4, const float* wp_4x4, const float* bp_4, float scale, float qa, float qb) {
    ODISE_REQUIRE(ctx && h_f16 && noise && xt_f16 && zdec_f16 && al16(h_f16) && al16(xt_f16) && al16(zdec_f16) && B >= 1 && P >= 1 && wq_4x8 && bq_4 &&
                      wp_4x4 && bp_4 && scale != 0.f,
                  "latent_heads: bad argument");
    LatentW w;
    for (int c = 0; c < 4; ++c) {
        for (int k = 0; k < 8; ++k) w.wq[c][k] = wq_4x8[c * 8 + k];
        for (int k = 0; k < 4; ++k) w.wp[c][k] = wp_4x4[c * 4 + k];
        w.bq[c] = bq_4[c];
        w.bp[c] = bp_4[c];
    }
    w.scale = scale; w.qa = qa; w.qb = qb;
    return launch_latent_heads(ctx, (const f16*)h_f16, noise, (f16*)xt_f16, (f16*)zdec_f16, latent, B, P, w);
}

extern "C" int odise_hip_l2_normalize(odise_hip_ctx* ctx, const void* x, int dtype, void* y_f16, int64_t rows, int C) {
    ODISE_REQUIRE(ctx && x && y_f16 && (dtype == ODISE_F16 || dtype == ODISE_F32) && rows >= 1 && rows < (1ll << 32) && C >= 1, "l2_normalize: bad argument");
    if (dtype == ODISE_F16) return launch_l2_normalize_f16(ctx, (const f16*)x, (f16*)y_f16, rows, C);
    return launch_l2_normalize_f32(ctx, (const float*)x, (f16*)y_f16, rows, C);
}

extern "C" int odise_hip_classify_rows(odise_hip_ctx* ctx, const float* L1, const float* L2, const int* seg_dev, const int* ovl_dev, const float* binary,
                                       float* out, int64_t rows, int K, int Ktot, float ls1, float ls2, float alpha, float beta) {
    ODISE_REQUIRE(ctx && L1 && L2 && seg_dev && ovl_dev && out && rows >= 1 && rows < (1ll << 31) && K >= 1 && Ktot >= K && K <= 4000,
                  "classify_rows: bad argument");
    return launch_classify_rows(ctx, L1, L2, seg_dev, ovl_dev, binary, out, rows, K, Ktot, ls1, ls2, alpha, beta);
}
