/*
 * odise_hip_tools.h — developer / measurement hooks of libodise_hip.so.  NOT part of the drop-in boundary (include/odise_hip.h):
 * nothing on the product path calls these; tools/ (tile calibration, A/B runs of kernel generations, the MFMA and LDS rate probes)
 * the ABI self-check of tests/test_lib_abi.py and the op-level tests of the small kernels (tests/test_gpu_glue_ops.py) do.
 */
#ifndef ODISE_HIP_TOOLS_H
#define ODISE_HIP_TOOLS_H

#include "odise_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sizeof of the descriptor structs as the library was compiled (tests validate the ctypes mirrors against them) */
int odise_hip_sizeof_gemm_desc(void);
int odise_hip_sizeof_conv_desc(void);
int odise_hip_sizeof_attn_desc(void);
int odise_hip_sizeof_post_desc(void);
int odise_hip_sizeof_infer_desc(void);
int odise_hip_sizeof_pq_desc(void);
int odise_hip_sizeof_pq_stat(void);
int odise_hip_sizeof_pq_boundary_task(void);
int odise_hip_sizeof_semseg_pq_task(void);
int odise_hip_sizeof_inst_eval_desc(void);
int odise_hip_sizeof_inst_eval_row(void);
int odise_hip_sizeof_inst_poly_gt(void);
int odise_hip_sizeof_inst_accum_desc(void);
int odise_hip_sizeof_inst_boxes_desc(void);
int odise_hip_sizeof_inst_bbox_task(void);
int odise_hip_sizeof_inst_boundary_task(void);
int odise_hip_sizeof_box_track_desc(void);
int odise_hip_sizeof_inst_box_draw(void);

/* odise_hip_gemm / odise_hip_conv2d with the tile shape and the split-K factor forced instead of chosen by the cost model
 * (tile ids: gemm.hip kTileBM / kTileBN; -1 / 0 = automatic) */
int odise_hip_gemm_forced(odise_hip_ctx* ctx, const odise_gemm_desc* d, int tile, int splitk);
int odise_hip_conv2d_forced(odise_hip_ctx* ctx, const odise_conv_desc* d, int tile, int splitk);
/* tile id | split-K factor << 8 that the calling thread's last odise_hip_gemm / odise_hip_conv2d launch ran with (-1: none yet) */
int odise_hip_last_tile(void);
/* kernel | DPAD << 8 | nsplit << 16 of the calling thread's last odise_hip_attention launch (-1: none yet).  kernel: 0 = tiled (attn_kernel),
 * 1 = K / V^T-resident (attn_kvres_kernel), 2 = pipelined self-attention (attn_sa_kernel); DPAD = the padded head dim of the instance that
 * ran; nsplit = blocks the keys were split over (1: no split, no combine pass).  tests/test_gpu_attention_ref.py asserts which kernel a case reached */
int odise_hip_last_attention(void);
/* a GEMM with a LayerNorm folded into its epilogue, as the CLIP towers chain them (csrc/common.h LnEpi; any pointer may be NULL):
 *   producer  stats_out [M][N/64][2]: partial (sum, sum of squares) of every output row, per 64 columns
 *   consumer  part [M][parts][2] + colsum [N]: C = act(rstd_m (A W'^T - mean_m colsum) + bias_n) (+ residual), the row statistics finished from
 *             the partials with 1/inv_c channels and eps; final_out [M][2] receives (-mean rstd, rstd)
 *   swapped   fin [N][2] + rowsum [M]: the normalised operand is W (its rows are the tokens), statistics per output column */
int odise_hip_gemm_ln(odise_hip_ctx* ctx, const odise_gemm_desc* d, const float* part, int parts, float inv_c, float eps, const float* colsum,
                      float* final_out, const float* fin, const float* rowsum, float* stats_out);
/* the conv -> GroupNorm pair of the ResBlocks with the conv's tile forced: the conv epilogue reduces the GroupNorm statistics (per channel and
 * row block) into stats_scratch [N * ceil(OH*OW/64) * Cout * 2] and the GroupNorm only finalises + applies; y_norm = act(gn(conv(x))) (f16).
 * *stats_blocks = row blocks per image (0: this kernel declined the fusion, the stand-alone GroupNorm ran) */
int odise_hip_conv2d_gn_forced(odise_hip_ctx* ctx, const odise_conv_desc* d, int tile, int splitk, const float* gamma, const float* beta,
                               int groups, float eps, int act, void* y_norm, float* stats_scratch, int* stats_blocks);
/* process-wide kernel-selection switches for A/B measurements (bits 0-3: timing ablations of the tools build; bits 4-23: gemm.hip g_conv_flags << 4).
 * Bits of retired kernel generations and switches (1, 4, 8, 4096, 8192, 16384 << 4; 1 << 24 and up) are accepted and ignored. */
int odise_hip_gemm_debug(int flags);

/* 1: the post-processing kernels never take their exact-x4-upsampling specialisations (tests assert both forms are bit-identical);
 * 2: the specialisations, but the per-pixel pass in its thread-per-cell-column form instead of the tiled one */
int odise_hip_post_generic(int on);
/* force the tile of the semantic GEMM [K, pixels] = P^T S^T (A/B of the 256-row rule in odise_hip_postprocess_batch); -1 = the rule */
int odise_hip_sem_tile(int tile);
/* GroupNorm (csrc/norm.hip): chunks of the statistics pass per image = compute units * chunk_factor / images (default 2).  A value >= 1 sets the
 * factor, anything else leaves it.  Another factor is another summation order of the same statistics (tools/head_reroll.py asks what that moves) */
int odise_hip_gn_tuning(int chunk_factor);
/* odise_hip_layer_norm with the second output the pixel decoder and the masked decoder take from the same kernel: y2 [rows,C] f16 =
 * y + table[row % P] (table f32 [P,C]) from the rounded y, the bits odise_hip_add_vec_table(y, NULL, table) writes.  y2 = NULL: no second output;
 * otherwise C <= 256, a table and P >= 1 are required (ODISE_ERR_ARG and nothing launched).  tests/test_gpu_norm_bits.py holds the identity */
int odise_hip_layer_norm_table(odise_hip_ctx* ctx, const void* x, void* y, const float* gamma, const float* beta, int rows, int C, float eps, void* y2,
                               const float* table, int P);
/* 1: the pixel decoder's MSDeformAttn layers as msda_prepare_kernel + the native-op kernel (the round 1-5 form) instead of the fused gather (A/B, bit-compare) */
int odise_hip_msda_unfused(int on);
/* the pixel decoder's MSDeformAttn on raw projections: value f16 [B, Lq, M, 32], off f32 [B*Lq, M*12*2], aw f32 [B*Lq, M*12] (3 levels hs3 x ws3, 4 points),
 * out f16 [B*Lq, M*32].  fused = 2 (or any other non-zero value): msda_fused_kernel as the pixel decoder runs it, 1: its 8-lanes-per-pair variant; 0: msda_prepare_kernel (into loc_scratch [B*Lq*M*24] / w_scratch [B*Lq*M*12]) + the native-op kernel */
int odise_hip_msda_fused_forward(odise_hip_ctx* ctx, const void* value, const float* off, const float* aw, const int* hs3, const int* ws3, int B, int M, int fused,
                                 void* out, float* loc_scratch, float* w_scratch);

/* stage boundaries of the model calls made while the timeline is on: at each boundary (csrc: stage_mark) an event on the stream the stage
 * enqueues to and the host clock.  _read synchronises the device and writes, relative to the first mark: gpu_ms[i] = when the device reached mark
 * i, host_ms[i] = when the host had enqueued everything before it; names = '\n'-separated.  tools/stage_timeline.py prints both columns. */
int odise_hip_stage_timeline(odise_hip_ctx* ctx, int on);
int odise_hip_stage_timeline_read(odise_hip_ctx* ctx, char* names, int names_cap, float* gpu_ms, double* host_ms, int cap, int* n);

/* encoder prefetch (odise_hip_infer_prefetch), what happened so far on this context: encoders enqueued ahead of their batch, prefetched results the
 * next odise_hip_infer consumed (hits), prepared results that were dropped because another batch came next, registrations that could not be
 * enqueued (the call in progress is unaffected).  Any pointer may be NULL.  tests/test_gpu_fullsize_batch.py asserts hit / drop per call. */
int odise_hip_prefetch_stats(odise_hip_ctx* ctx, int* enqueued, int* hits, int* dropped, int* failed);

/* per-context log of every GEMM / convolution launch the cost model decided (tests print which choices differ between two batch sizes):
 * odise_hip_launch_log(ctx, 1) starts / clears it, (ctx, 0) drops it; _read copies records of 6 ints (conv, M, N, K, tile id, split-K factor) */
int odise_hip_launch_log(odise_hip_ctx* ctx, int on);
int odise_hip_launch_log_read(odise_hip_ctx* ctx, int* out6, int cap, int* n);

/* 1: the feature extractor enqueues everything on one stream; 2 (default): its CLIP -> UNet branch runs on a second stream beside the VAE */
int odise_hip_set_lanes(odise_hip_ctx* ctx, int lanes);

/* the s2..s5 backbone maps still resident in the context's arena after odise_hip_backbone_forward / odise_hip_infer, converted to fp32 NCHW
 * [B,C,h,w] device arrays out4[i] (NULL entries are skipped); shape_bchw4x4 (optional, host) receives the four (B, C, h, w).  What the
 * parity tests feed to the fp32 oracle head to attribute a re-decided query (tests/fullsize.py ideal_on_device_features) */
int odise_hip_backbone_maps(odise_hip_ctx* ctx, float** out4, int* shape_bchw4x4);

/* Mask logits chosen by the caller in place of the head's (tests of the post-processing kernels: tests/test_gpu_postprocess.py).  pred_masks
 * fp32 device [B,Q,h4,w4], 1 <= Q <= 304, is rounded to fp16 into storage the context owns (released with it; no arena reset or growth
 * of a later call touches it) and becomes "the mask logits of the last head forward" with this B / Q / h4 / w4 for odise_hip_postprocess_batch / _postprocess_pixels /
 * _instance_masks / _instance_rle.  No head weights are needed.  There are no mask embeddings behind these logits: odise_hip_classify
 * returns ODISE_ERR_STATE until a real odise_hip_head_forward / odise_hip_predictor_forward has run, which takes over again.  The call
 * also brings up the context's second lane and a small arena if the backbone stage has not done so yet. */
int odise_hip_set_head_masks(odise_hip_ctx* ctx, const float* pred_masks, int B, int Q, int h4, int w4);

/* probe (probe.hip): MFMA output layout (tests/test_gpu_probe.py).  The rate probes and yardstick kernels live in odise_hip_lab.h and only
 * in the measurement build of the library. */
int odise_hip_mfma_probe(odise_hip_ctx* ctx, float* host_out);

/* MaskCLIP's visibility rows (clip.py:288-318: bilinear resize of the mask probabilities to the CLIP input, max over each patch, >= 0.5):
 * out [B][T + Q][ldm] u8 (1 = hidden; rows < T are the image tokens' all-visible rows) from logits [B,Q,h,w] f16; T = (S / patch)^2 + 1.
 * plain = 1 runs the form that interpolates both source rows of every sample row anew (the two forms must agree to the bit). */
int odise_hip_maskclip_token_mask(odise_hip_ctx* ctx, const void* logits_f16, void* out_u8, int B, int Q, int h, int w, int S, int patch, int T,
                                  int64_t ldm, int plain);

/* ---- the small kernels between the GEMM stages, one hook per kernel (tests/test_gpu_glue_ops.py holds each to the float64 restatement of
 * tests/glue_reference.py).  All pointers are device pointers unless named host; f16 maps are NHWC with C a multiple of 8 and 16-byte aligned;
 * every call is enqueued on the context's stream.  A bad size or pointer is ODISE_ERR_ARG and nothing is launched; window boxes live on the
 * device and are the caller's to keep inside the image. */
/* slide-window crops (feature_extractor.py:216-224): crops [B*K,C,S,S] f32 = img [B,C,H,W] f32 [:, :, y1:y1+S, x1:x1+S], boxes [K][2] int (y1, x1) */
int odise_hip_crop_extract(odise_hip_ctx* ctx, const float* img, float* crops, int B, int C, int H, int W, int S, int K, const int* boxes_dev);
/* the same with windows of s x s resized to S x S (feature_extractor.py:197-215, 69-77: T.Resize(BICUBIC) of the cropped tensor =
 * F.interpolate(mode="bicubic", align_corners=False), A = -0.75, taps clamped to the window) */
int odise_hip_crop_resize_bicubic(odise_hip_ctx* ctx, const float* img, float* crops, int B, int C, int H, int W, int s, int S, int K,
                                  const int* boxes_dev);
/* CLIP preprocess (clip.py:94: T.Resize(S, BICUBIC) of the short side + T.CenterCrop(S) + T.Normalize): out [N,S,S,8] f16, channels 3..7 zero,
 * from image01 [N,3,H,W] f32 */
int odise_hip_clip_preprocess(odise_hip_ctx* ctx, const float* image01, void* out_f16, int N, int H, int W, int S);
/* MaskCLIP's image resize (clip.py:327-332: F.interpolate(image, (S, S), mode="bilinear", align_corners=False)) + CLIP normalise: out [B,S,S,8] f16 */
int odise_hip_resize_bilinear_norm(odise_hip_ctx* ctx, const float* image01, void* out_f16, int B, int H, int W, int S);
/* F.interpolate(x, size=(OH, OW)) in its default nearest mode (feature_extractor.py:165-168): y [N,OH,OW,C] from x [N,H,W,C] */
int odise_hip_upsample_nearest(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int N, int H, int W, int OH, int OW, int C);
/* overlap-add of the per-window features over count_mat (feature_extractor.py:229-248): feat [B*K,ch,cw,C] f16, boxes [K][2] int in feature
 * pixels -> out_f16 [B,OH,OW,C] and / or out_nchw [B,C,OH,OW] f32 (either may be NULL); a pixel no window covers is 0 */
int odise_hip_stitch(odise_hip_ctx* ctx, const void* feat_f16, void* out_f16, float* out_nchw, int B, int K, const int* boxes_dev, int ch, int cw, int OH,
                     int OW, int C);
/* src + level_embed (+ positional table) (msdeformattn.py:71-75, odise.py:657-660): y [N,P,C] = x [N,P,C] + vec [C] + table [P,C]; vec / table f32, may be NULL */
int odise_hip_add_vec_table(odise_hip_ctx* ctx, const void* x_f16, const float* vec, const float* table, void* y_f16, int64_t N, int P, int C);
/* query_feat.weight.unsqueeze(0).repeat(B, 1, 1) (odise.py:663-664): y [B][n] = x [n] f16, n a multiple of 8 */
int odise_hip_broadcast_rows(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int64_t n, int B);
/* cur_fpn + F.interpolate(out[-1], size=cur_fpn.shape[-2:], mode="bilinear", align_corners=False) (msdeformattn.py:347):
 * y [N,OH,OW,C] = a [N,OH,OW,C] + resize(b [N,H,W,C]); a = NULL: the resized map alone */
int odise_hip_bilinear_add(odise_hip_ctx* ctx, const void* a_f16, const void* b_f16, void* y_f16, int N, int H, int W, int OH, int OW, int C);
/* MaskPooling's prologue (odise.py:949-955: mask = (mask.sigmoid() > 0.5); denorm = mask.sum(-1) + 1e-8): m01 [rows,HW] f16, inv [rows] f32 = 1 / denorm;
 * _f16 takes fp16 logits (HW a multiple of 8), _f32 the fp32 ones of odise_hip_mask_pooling */
int odise_hip_mask_binarize_f16(odise_hip_ctx* ctx, const void* mask_f16, void* m01_f16, float* inv, int64_t rows, int HW);
int odise_hip_mask_binarize_f32(odise_hip_ctx* ctx, const float* mask, void* m01_f16, float* inv, int64_t rows, int HW);
/* the masked-attention rows (odise.py:760-774: F.interpolate(outputs_mask, size, mode="bilinear").sigmoid() < 0.5, and :683: a row that masks every
 * key is cleared): out [rows][ldm] u8 (1 = masked; columns oh*ow..ldm-1 are 1) from logits [rows,H,W] of dtype ODISE_F16 / ODISE_F32 */
int odise_hip_attn_mask(odise_hip_ctx* ctx, const void* logits, int dtype, void* out_u8, int64_t rows, int H, int W, int oh, int ow, int64_t ldm);
/* the VAE AttnBlock's torch.softmax(scale * x, dim=-1) on fp16 rows of `cols` <= 8192 values, row stride ld (a multiple of 8); y may be x */
int odise_hip_softmax_rows(odise_hip_ctx* ctx, const void* x_f16, void* y_f16, int64_t rows, int cols, int64_t ld, float scale);
/* torch.cat([class_embedding, patches]) + positional_embedding (clip.py:179-190) with `extra` copies of the class token appended (clip.py:268-270):
 * tok [B,TP,Cw] f16 from patches [B,T-1,Cw] f16, cls [Cw] f32, pos [T,Cw] f32; rows T+extra..TP-1 are zero */
int odise_hip_clip_assemble(odise_hip_ctx* ctx, const void* patches_f16, const float* cls, const float* pos, void* tok_f16, int B, int T, int extra, int TP,
                            int Cw);
/* uncond + tanh(alpha) * (proj + pos) (ldm.py:706-709) folded to out [B,T,Cw] = A1 [T,Cw] + A2 [T,Cw] * proj [B,Cw] (all f32) */
int odise_hip_cond_inputs(odise_hip_ctx* ctx, const float* proj, const float* A1, const float* A2, float* out, int B, int T, int Cw);
/* quant_conv mean * scale_factor -> q_sample (gaussian_diffusion.py:275-292) and post_quant_conv (ldm.py:459-467, 535-538, 577-598): h [B,P,8] f16,
 * noise [4,P] f32 -> xt, zdec [B,P,8] f16 (channels 4..7 zero), latent [B,4,P] f32 (may be NULL).  The weights are HOST arrays: wq [4][8], bq [4],
 * wp [4][4], bp [4]; qa = sqrt(alpha_bar_t), qb = sqrt(1 - alpha_bar_t) */
int odise_hip_latent_heads(odise_hip_ctx* ctx, const void* h_f16, const float* noise, void* xt_f16, void* zdec_f16, float* latent, int B, int P,
                           const float* wq_4x8, const float* bq_4, const float* wp_4x4, const float* bp_4, float scale, float qa, float qb);
/* F.normalize(x, dim=-1) (eps 1e-12): y [rows,C] f16 from x of dtype ODISE_F16 / ODISE_F32 */
int odise_hip_l2_normalize(odise_hip_ctx* ctx, const void* x, int dtype, void* y_f16, int64_t rows, int C);
/* the open-vocabulary class scores (helper.py:79-109 max over synonyms; odise.py:1506-1536 geometric ensemble; odise.py:300-323 null merge and
 * log): L1 [rows,Ktot+1] (null last) / L2 [rows,Ktot] f32 cosines, seg [K+1] / ovl [K] int, binary [rows,2] f32 or NULL (odise.py:559-565) ->
 * out [rows,K+1] f32 log-probabilities */
int odise_hip_classify_rows(odise_hip_ctx* ctx, const float* L1, const float* L2, const int* seg_dev, const int* ovl_dev, const float* binary, float* out,
                            int64_t rows, int K, int Ktot, float ls1, float ls2, float alpha, float beta);
#ifdef __cplusplus
}
#endif
#endif /* ODISE_HIP_TOOLS_H */
