/*
 * odise_hip.h — C ABI of libodise_hip.so, the MI355X (gfx950) device side of the
 * ODISE panoptic-inference hot path.
 *
 * Every entry point takes plain pointers and sizes (no torch types).  Device pointers
 * are raw HIP device addresses (hipMalloc'ed by odise_hip_malloc or borrowed from a
 * torch-ROCm tensor's data_ptr()).  All functions return 0 on success and a negative
 * code on failure; odise_hip_last_error() returns a human readable message.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   - odise_hip_ms_deform_attn_forward  <->  MSDA.ms_deform_attn_forward
 *       third_party/Mask2Former/mask2former/modeling/pixel_decoder/ops/src/ms_deform_attn.h:25-44
 *       third_party/Mask2Former/mask2former/modeling/pixel_decoder/ops/src/cuda/ms_deform_attn_cuda.cu:25-85
 *   - odise_hip_unet_features           <->  LdmExtractor.unet_forward
 *       odise/modeling/meta_arch/ldm.py:469-491 (taps = concat-inputs of output blocks 2,5,8,11)
 *   - odise_hip_mask_pooling            <->  MaskPooling.forward  odise/modeling/meta_arch/odise.py:937-963
 *   - op-level entry points (gemm / conv / group-norm / layer-norm / attention) are the
 *     building blocks the stage-level calls are made of; they are exported so every
 *     stage can be parity-tested in isolation (SURVEY.md §8b last row).
 */
#ifndef ODISE_HIP_H
#define ODISE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct odise_hip_ctx odise_hip_ctx;

enum { ODISE_F16 = 0, ODISE_F32 = 1, ODISE_U8 = 2 };   /* ODISE_U8: uint8 / bool masks (odise_hip_rle_encode) */
enum { ODISE_ACT_NONE = 0, ODISE_ACT_SILU = 1, ODISE_ACT_RELU = 2, ODISE_ACT_GELU = 3, ODISE_ACT_QUICKGELU = 4 };

/* error codes */
enum {
    ODISE_OK = 0,
    ODISE_ERR_ARG = -1,      /* bad argument (shape/alignment/dtype) */
    ODISE_ERR_HIP = -2,      /* a HIP runtime call failed           */
    ODISE_ERR_STATE = -3,    /* missing weights / wrong call order  */
    ODISE_ERR_NOMEM = -4,    /* workspace / arena exhausted         */
    ODISE_ERR_UNSUPPORTED = -5 /* a valid input this library does not handle (e.g. an arithmetic-coded JPEG) */
};

/* ---- context / plumbing ------------------------------------------------------------ */
int odise_hip_create(int device, odise_hip_ctx** out);
int odise_hip_destroy(odise_hip_ctx* ctx);
const char* odise_hip_last_error(void);
int odise_hip_version(void);
/* adopt an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int odise_hip_set_stream(odise_hip_ctx* ctx, void* hip_stream);
int odise_hip_malloc(odise_hip_ctx* ctx, size_t bytes, void** dptr);
int odise_hip_free(odise_hip_ctx* ctx, void* dptr);
int odise_hip_memcpy_h2d(odise_hip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int odise_hip_memcpy_d2h(odise_hip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int odise_hip_memset(odise_hip_ctx* ctx, void* dst_dev, int value, size_t bytes);
int odise_hip_sync(odise_hip_ctx* ctx);
/* HIP-event timing on the context's stream (what bench.py uses around the timed region) */
int odise_hip_timer_start(odise_hip_ctx* ctx);
int odise_hip_timer_stop(odise_hip_ctx* ctx, float* elapsed_ms);
int odise_hip_device_info(odise_hip_ctx* ctx, char* name_buf, int buf_len, int* cu_count, size_t* hbm_bytes);
/* Per-context execution options.  They choose between arithmetic-equivalent forms of a stage, never between results and no results:
 *   ODISE_OPT_CLIP_LN_FOLD     how the CLIP towers (clip.py:177-206, 252-323) take their LayerNorms: 0 = folded into the neighbouring GEMMs from
 *                              8192 token rows per call (default; below that as kernels), 1 = always folded, 2 = never.  The two forms differ by
 *                              fp16 rounding, so a caller that needs results independent of how many crops share a call pins 1 or 2.
 *   ODISE_OPT_VAE_CHUNK_BYTES  > 0: the AutoencoderKL levels (ldm.py:493-533, 585-606) run over as many crops per launch as keep one activation
 *                              tensor below this many bytes (a smaller working set and arena); 0 (default) = all crops of a call at once, which
 *                              measured faster on MI355X (profiles/r04_vae_chunking_experiment.txt).  Per-crop arithmetic is unchanged.
 *   ODISE_OPT_PREFETCH_CU_EIGHTHS  1..7: the encoder-prefetch stream (odise_hip_infer_prefetch) is created with a CU mask of that many of every 8
 *                              compute units, so the batch in progress always finds free CUs for its small dependent launches - a CU-masked stream
 *                              has NORMAL priority and default flags (HIP offers neither with a mask); 0 / 8 (default 0) = no mask, lowest
 *                              priority, non-blocking.  Read when the stream is first created.
 *   ODISE_OPT_PREFETCH_START   where the next batch's encoder is enqueued: 0 = behind the current batch's VAE lane, 1 (default) = behind its
 *                              backbone, i.e. beside the serial tail of small launches (pixel decoder .. post-processing)
 *   ODISE_OPT_ATTN_KV_RESIDENT 0 (default) = attention with d_head 64 and at most 608 keys runs the K / V^T-resident kernel where (head, image)
 *                              pairs fill the chip in whole rounds (the CLIP tower of 16 / 32 crops), unmasked self-attention over whole
 *                              128-query / 64-key tiles (the SD UNet's 64^2 and 32^2 levels) the software-pipelined kernel, the tiled kernel
 *                              elsewhere; 2 = never the K / V^T-resident kernel, 4 = never the pipelined one, 6 = always the tiled kernel.  The
 *                              resident form steps the running softmax maximum per 32 instead of 64 keys (results agree to fp32 rounding);
 *                              the pipelined form is bit-identical to the tiled one.
 *   ODISE_OPT_MASKCLIP_PASSES  MaskCLIP (clip.py:252-323) hides the mask tokens from every query (clip.py:314-315), so the 577 image tokens of a
 *                              picture run the plain tower whatever the masks are and the Q mask tokens only read its keys and values.
 *                              0 (default) = two passes: the image tokens leave q|k and V^T of every block, the mask tokens follow as B x Q
 *                              rows; in odise_hip_infer the pictures' image tokens RIDE IN THE CROPS' CLIP TOWER of the implicit captioner (the
 *                              same frozen ViT-L/14@336: pictures + crops are one batch of token rows on the second lane), so only the
 *                              mask-token pass is left on the serial tail behind the mask head.  1 = two passes, both where the reference runs
 *                              the tower (after the mask head).  2 = one pass over [577 image | Q mask] token rows (the reference's layout).
 *                              3 = as 0 with the first pass as a tower of its own on the second lane behind the UNet.  The forms run the same
 *                              arithmetic per row on different GEMM tiles and LayerNorm forms (CLIP_LN_FOLD counts the rows of the tower the
 *                              tokens are in): results agree to fp16 rounding.  odise_hip_classify / odise_hip_maskclip_embed called on their
 *                              own run 0 and 3 as 1. */
enum { ODISE_OPT_CLIP_LN_FOLD = 1, ODISE_OPT_VAE_CHUNK_BYTES = 2, ODISE_OPT_ATTN_KV_RESIDENT = 3, ODISE_OPT_PREFETCH_CU_EIGHTHS = 4, ODISE_OPT_PREFETCH_START = 5,
       ODISE_OPT_MASKCLIP_PASSES = 6 };
int odise_hip_set_option(odise_hip_ctx* ctx, int option, int64_t value);
int odise_hip_get_option(odise_hip_ctx* ctx, int option, int64_t* value);
/* Launch probe (measurement, bench.py's `roofline`): HIP events around every launch of ONE shape - conv != 0: the implicit GEMM of a convolution
 * with M = N*OH*OW output pixels, N = Cout, K = KH*KW*Cin (convolutions with the fused 2x upsample are not matched); conv = 0: odise_hip_gemm's M, N, K - recorded on whichever stream the library
 * launches it on, for the next max_launches matching launches.  odise_hip_probe_read waits for the recorded launches, writes their durations
 * in microseconds (at most cap) and the number recorded, and disarms the probe. */
int odise_hip_probe_arm(odise_hip_ctx* ctx, int conv, int M, int N, int K, int max_launches);
int odise_hip_probe_read(odise_hip_ctx* ctx, float* us_out, int cap, int* n_launches);

/* ---- MSDeformAttn forward ------------------------------ */
/* value        [B, S, M, D]      dtype value_dtype (device)
 * spatial_shapes [L, 2] int64 (HOST)   (H_l, W_l)
 * level_start_index [L] int64 (HOST)
 * sampling_loc [B, Lq, M, L, P, 2] f32 (device), normalised to [0,1]
 * attn_weight  [B, Lq, M, L, P]   f32 (device)
 * out          [B, Lq, M*D]       dtype value_dtype (device)
 * im2col_step is accepted for signature parity and validated like the reference
 * (B % min(B, im2col_step) == 0, ms_deform_attn_cuda.cu:52) but the kernel is one launch. */
int odise_hip_ms_deform_attn_forward(odise_hip_ctx* ctx, const void* value, const int64_t* spatial_shapes,
                                     const int64_t* level_start_index, const float* sampling_loc,
                                     const float* attn_weight, int B, int S, int M, int D, int Lq, int L, int P,
                                     int im2col_step, int value_dtype, void* out);

/* ---- GEMM: C[M,N] = epilogue(alpha * A[M,K] * W[N,K]^T) -----------------------------
 * Replaces every nn.Linear / projection of the path (W in PyTorch's [out, in] layout, bias_n = bias): the q/k/v/out projections and
 * FFNs of M2F/modeling/transformer_decoder/mask2former_transformer_decoder.py:17-204 and of MSDeformAttn (ops/modules/ms_deform_attn.py:98-125),
 * PooledMaskEmbed's pool_proj / mask_embed MLPs (odise/modeling/meta_arch/odise.py:975-1009), PositionalLinear (ldm.py:624-635), the
 * CLIP and SD-UNet transformer blocks driven from clip.py:252-280 / ldm.py:469-491 (GEGLU, per-row terms and row-group adds are their
 * fused tails), text_proj and the cosine logits of odise.py:181-207. */
typedef struct {
    int M, N, K;              /* K % 8 == 0 */
    const void* A; int64_t lda;   /* f16, row-major, lda % 8 == 0, 16-byte aligned */
    const void* W; int64_t ldw;   /* f16, row-major [N,K] ("B^T" form) */
    void* C; int64_t ldc;
    int c_dtype;              /* ODISE_F16 | ODISE_F32 */
    const float* bias_n;      /* [N] or NULL */
    const float* bias_m;      /* [M] or NULL */
    const float* scale_m;     /* [M] or NULL: per-row multiplier applied to the accumulator first */
    const void* residual;     /* f16 [M, ldr] or NULL (added after activation) */
    int64_t ldr;
    const float* rowgroup_add;/* [ceil(M/rows_per_group), N] f32 or NULL (added before activation) */
    int rows_per_group;
    int64_t ldg;              /* row stride of rowgroup_add (0 -> N) */
    int act;                  /* ODISE_ACT_* */
    int geglu;                /* 1: columns are interleaved (a,gate) pairs -> out[M,N/2] = a*gelu(gate) */
    float alpha;
    int batch;                /* >=1; batched over grid.z with element strides below */
    int64_t strideA, strideW, strideC, strideR;
} odise_gemm_desc;
int odise_hip_gemm(odise_hip_ctx* ctx, const odise_gemm_desc* d);

/* ---- implicit-GEMM convolution, NHWC f16 --------------------------------------------
 * Replaces nn.Conv2d / detectron2.layers.Conv2d wherever the path convolves: the SD UNet and VAE blocks walked by ldm.py:424-533
 * (incl. Upsample = nearest 2x + 3x3 conv -> upsample2x, the time-embedding broadcast -> per_image_add), the BottleneckBlock projections
 * of feature_extractor.py:53-66, the pixel decoder's input_proj / lateral / output / mask_features convs
 * (M2F/modeling/pixel_decoder/msdeformattn.py:206-286) and CLIP's patch embedding (clip.py:253). */
typedef struct {
    int N, H, W, Cin;         /* input  X [N,H,W,Cin] f16, Cin % 8 == 0 */
    int Cout, KH, KW, stride, pad_t, pad_l, OH, OW;
    int upsample2x;           /* 1: conv runs on nearest-2x upsampled X (fused gather) */
    const void* X;
    const void* Wt;           /* [Cout, KH, KW, Cin] f16 */
    void* Y; int y_dtype;     /* [N,OH,OW,Cout] */
    const float* bias;        /* [Cout] or NULL */
    const void* residual;     /* f16 [N,OH,OW,Cout] or NULL */
    const float* per_image_add;/* [N, Cout] f32 or NULL (time-embedding broadcast) */
    int64_t per_image_add_ld; /* row stride of per_image_add (0 -> Cout) */
    int act;
} odise_conv_desc;
int odise_hip_conv2d(odise_hip_ctx* ctx, const odise_conv_desc* d);

/* ---- normalisation -------------------------------------------------------------------
 * GroupNorm: nn.GroupNorm(32, C) of msdeformattn.py:218-225 / get_norm("GN") of the detectron2 Conv2d wrappers and BottleneckBlocks,
 * ldm's Normalize in every ResnetBlock / ResBlock (+ fused SiLU).  LayerNorm: decoder norms (mask2former_transformer_decoder.py:26, 84,
 * 149), decoder_norm, PooledMaskEmbed (odise.py:975-977), CLIP ln_pre / ln_1 / ln_2 / ln_post (clip.py:264-276). */
/* GroupNorm over NHWC f16 x[N,HW,C]; stats in fp32; y = act(gn(x)*gamma+beta) (f16) */
int odise_hip_group_norm(odise_hip_ctx* ctx, const void* x, void* y, const float* gamma, const float* beta,
                         int N, int HW, int C, int groups, float eps, int act);
/* y = act(GroupNorm(x) + residual) + accum; residual / accum optional f16 tensors shaped like x
 * (detectron2 BottleneckBlock tail and the per-stride sum of feature_extractor.py:171-176) */
int odise_hip_group_norm_ex(odise_hip_ctx* ctx, const void* x, void* y, const float* gamma, const float* beta,
                            int N, int HW, int C, int groups, float eps, int act, const void* residual, const void* accum);
/* LayerNorm over the last dim of x[rows, C] f16 -> y f16 */
int odise_hip_layer_norm(odise_hip_ctx* ctx, const void* x, void* y, const float* gamma, const float* beta,
                         int rows, int C, float eps);

/* ---- fused attention -------------------------------------------------------------------
 * Replaces nn.MultiheadAttention of the masked decoder (mask2former_transformer_decoder.py:22, 80: self-attention and cross-attention
 * with the boolean attn_mask of odise.py:763-775), CLIP's transformer with the mask-token attention mask (clip.py:271, 300-323) and the
 * SD UNet's CrossAttention (self and text-conditioned, d_head 40..160) reached through ldm.py:469-491. */
/* O[b,q,h*D+d] = softmax_k(scale * Q[b,q,h*D+:] . K[b,k,h*D+:] + mask) V
 * Q  [B, Lq, ldq] f16, K [B, Lk, ldk] f16, Vt [B, H*D, ldvt] f16 (V TRANSPOSED: row h*D+d, col key),
 * O  [B, Lq, ldo] f16.  mask: optional u8 [B, Lq, ldmask] (1 = key not visible), shared by heads.
 * D in {32,40,64,80,160}; ldvt % 8 == 0, ldmask % 4 == 0. */
typedef struct {
    int B, H, Lq, Lk, D;
    const void* Q; int64_t ldq, strideQ;
    const void* K; int64_t ldk, strideK;
    const void* Vt; int64_t ldvt, strideVt;
    void* O; int64_t ldo, strideO;
    const uint8_t* mask; int64_t ldmask, strideMask;
    float scale;
} odise_attn_desc;
int odise_hip_attention(odise_hip_ctx* ctx, const odise_attn_desc* d);

/* ---- layout / elementwise helpers ---------------------------------------------------- */
int odise_hip_nchw_f32_to_nhwc_f16(odise_hip_ctx* ctx, const float* x, void* y, int N, int C, int H, int W, int Cpad);
int odise_hip_nhwc_f16_to_nchw_f32(odise_hip_ctx* ctx, const void* x, float* y, int N, int C, int H, int W);
int odise_hip_cast_f32_to_f16(odise_hip_ctx* ctx, const float* x, void* y, size_t n);
int odise_hip_cast_f16_to_f32(odise_hip_ctx* ctx, const void* x, float* y, size_t n);
/* y[n,p,:] = cat(a[n,p,:Ca], b[n,p,:Cb]) (f16, channels-last) */
int odise_hip_concat_channels(odise_hip_ctx* ctx, const void* a, const void* b, void* y, size_t pixels, int Ca, int Cb);

/* ---- MaskPooling (odise.py:937-963) --------------------------------------------------- */
/* x [B,C,H,W] f32 NCHW, mask logits [B,Q,H,W] f32 -> pooled [B,Q,C] f32
 * pooled = einsum(x, sigmoid(mask)>0.5) / (sum(mask>0) + 1e-8) */
int odise_hip_mask_pooling(odise_hip_ctx* ctx, const float* x, const float* mask, float* pooled,
                           int B, int C, int Q, int HW);

/* ---- SD v1 UNet single-step feature extraction (ldm.py:469-491) ----------------------- */
/* Weights are registered by their checkpoint key (model.diffusion_model.* stripped of that prefix),
 * host fp32, any rank<=4; the library converts to its packed fp16 layouts.  */
int odise_hip_load_weight(odise_hip_ctx* ctx, const char* name, const float* host_data, const int64_t* shape, int ndim);
int odise_hip_unet_build(odise_hip_ctx* ctx);     /* after all weights are loaded; packs + uploads */
int odise_hip_clear_host_weights(odise_hip_ctx* ctx);  /* drop the host fp32 staging copies after build */
/* x_t [B,4,h,w] f32 NCHW (device), context [B,77,768] f32 (device), cond_emb [B,1280] f32 or NULL (device).
 * taps: u2 [B,2560,h/8,w/8], u5 [B,1920,h/4,w/4], u8 [B,960,h/2,w/2], u11 [B,640,h,w] f32 NCHW (device), any may be NULL.
 * timestep t (the reference uses t=0).  */
int odise_hip_unet_features(odise_hip_ctx* ctx, const float* x_t, const float* context, const float* cond_emb,
                            int B, int h, int w, int t, float* tap_u2, float* tap_u5, float* tap_u8, float* tap_u11);
/* same, but keeps taps as fp16 NHWC inside the context (bench / fused pipeline path); returns device pointers */
int odise_hip_unet_features_nhwc(odise_hip_ctx* ctx, const float* x_t, const float* context, const float* cond_emb,
                                 int B, int h, int w, int t, void** taps4);
/* analytic MACs of the last unet call (per the layer shapes actually launched) */
int odise_hip_unet_last_macs(odise_hip_ctx* ctx, double* macs);
/* capture the unet forward for (B,h,w) into a hipGraph and replay it on subsequent calls (0 disables) */
int odise_hip_unet_use_graph(odise_hip_ctx* ctx, int enable);

/* ---- LdmImplicitCaptionerExtractor.forward (ldm.py:697-718 -> 543-621) ------------------------------ */
/* Weights (host fp32, checkpoint keys): first_stage_model.* and model.diffusion_model.* (SD v1 ckpt "state_dict"),
 * clip.visual.* (OpenAI ViT-L-14-336px archive, prefixed with "clip."), backbone.feature_extractor.{clip_project.*,
 * alpha_cond, time_embed_project.*, alpha_cond_time_embed} (ODISE ckpt "model"), plus the two frozen buffers
 * backbone.feature_extractor.ldm_extractor.{ldm.uncond_inputs [1,77,768], shared_noise [1,4,64,64]}. */
int odise_hip_extractor_build(odise_hip_ctx* ctx);
/* image [B,3,H,W] f32 device in [0,1] (H,W multiples of 64; reference crops are 512x512).  taps8: 8 device pointers
 * (fp32 NCHW, any may be NULL) in the reference's order enc5, enc7, u2, u5, u8, u11, dec2, dec5 (ldm.py:608). */
int odise_hip_extractor_forward(odise_hip_ctx* ctx, const float* image, int B, int H, int W, float** taps8);
/* hot-path variant: taps stay fp16 NHWC inside the library arena; returns pointers and [n,c,h,w] per tap */
int odise_hip_extractor_forward_nhwc(odise_hip_ctx* ctx, const float* image, int B, int H, int W, void** taps8, int* shapes8x4);
int odise_hip_extractor_last_macs(odise_hip_ctx* ctx, double* macs);

/* ---- FeatureExtractorBackbone (feature_extractor.py:139-250): slide-window crops -> extractor -> projections -> stitch ---- */
/* extra weights: backbone.feature_projections.{0..7}.0.{conv1,conv2,conv3[,shortcut]}.{weight,norm.weight,norm.bias} */
int odise_hip_backbone_build(odise_hip_ctx* ctx);
/* image [B,3,H,W] f32 device in [0,1], H,W >= 512 and multiples of 64.  out4: s2,s3,s4,s5 fp32 NCHW [B,512,H/4..H/32,..]
 * device pointers (array or entries may be NULL); fp16 NHWC copies stay inside the library for odise_hip_head_forward. */
int odise_hip_backbone_forward(odise_hip_ctx* ctx, const float* image, int B, int H, int W, float** out4);

/* ---- MaskFormerHead: MSDeformAttn pixel decoder + ODISE masked transformer decoder (msdeformattn.py:314-358, odise.py:642-776) */
/* weights: sem_seg_head.pixel_decoder.*, sem_seg_head.predictor.* */
int odise_hip_head_build(odise_hip_ctx* ctx);
/* feats4: s2..s5 fp32 NCHW device pointers [B,Cin,H4>>i,W4>>i], or NULL to consume the last backbone_forward.
 * outputs (device fp32, any may be NULL): pred_masks [B,Q,H4,W4] logits, mask_embed [B,Q,C], mask_pooled_features [B,Q,C];
 * logit_scale (host) = clamp(exp(logit_scale), max=100). */
int odise_hip_head_forward(odise_hip_ctx* ctx, const float* const* feats4, int B, int Cin, int H4, int W4, float* pred_masks,
                           float* mask_embed, float* mask_pooled, float* logit_scale);
int odise_hip_maskgen_info(odise_hip_ctx* ctx, int* num_queries, int* hidden_dim, double* last_macs);
/* the two halves of the head on their own (the reference's modules are callable one by one):
 * MSDeformAttnPixelDecoder.forward_features (msdeformattn.py:314-358): feats4 = s2..s5 fp32 NCHW -> mask_features [B,C,H4,W4] and the three
 * multi-scale maps [B,C,H4/8,W4/8], [B,C,H4/4,W4/4], [B,C,H4/2,W4/2] (fp32 NCHW device, any may be NULL) */
int odise_hip_pixel_decoder_forward(odise_hip_ctx* ctx, const float* const* feats4, int B, int Cin, int H4, int W4, float* mask_features,
                                    float* const* multi_scale3);
/* ODISEMultiScaleMaskedTransformerDecoder.forward (odise.py:642-727): multi_scale3 = 3 fp32 NCHW maps of sizes hw3 [3][2] (HOST),
 * mask_features [B,C,H4,W4]; outputs as odise_hip_head_forward (and kept inside for odise_hip_classify / postprocess) */
int odise_hip_predictor_forward(odise_hip_ctx* ctx, const float* const* multi_scale3, const int* hw3, const float* mask_features, int B, int H4, int W4,
                                float* pred_masks, float* mask_embed, float* mask_pooled, float* logit_scale);

/* ---- open-vocabulary classification (odise.py:285-323; clip.py:252-361; helper.py:79-109) ---------------------------- */
/* weights: category_head.text_proj.{weight,bias}, category_head.null_embed (ODISE ckpt) + the CLIP tower of the extractor */
int odise_hip_classify_build(odise_hip_ctx* ctx);
/* vocabulary = CLIP text embeddings (HOST fp32) of the two prompt sets the reference builds per label tuple
 * (category_head: plain labels; clip_head: "a photo of a {}."), K synonym groups of group_sizes[k] strings each,
 * overlap[k] = 1 if the class overlaps a training class (category_overlapping_mask, odise.py:1479-1491), alpha/beta of clip_head */
int odise_hip_set_vocabulary(odise_hip_ctx* ctx, const float* cat_text, const float* clip_text, int K_tot, int dim,
                             const int* group_sizes, const int* overlap, int K, float alpha, float beta);
/* image [B,3,H,W] fp32 device in [0,1]; uses the last head_forward; mask_cls [B,Q,K+1] fp32 device (log-probabilities);
 * clip_embed (optional) [B,Q,dim] fp32 device = MaskCLIP.get_mask_embed */
int odise_hip_classify(odise_hip_ctx* ctx, const float* image, int B, int H, int W, float* mask_cls, float* clip_embed);
/* MaskCLIP.get_mask_embed stand-alone (clip.py:325-338; the arithmetic of PoolingCLIPHead.forward, odise.py:1469-1542): image [B,3,H,W] fp32 in
 * [0,1], pred_masks [B,Q,h,w] fp32 logits (device) -> clip_embed [B,Q,dim] fp32.  Needs the CLIP tower (odise_hip_extractor_build). */
int odise_hip_maskclip_embed(odise_hip_ctx* ctx, const float* image, int B, int H, int W, const float* pred_masks, int Q, int h, int w, float* clip_embed);

/* ---- post-processing (odise.py:326-370; maskformer_model.py:280-380) ------------------------------------------------- */
/* fused mask upsample (x4 bilinear to pad_h x pad_w, crop img_h x img_w, bilinear to out_h x out_w) + sigmoid +
 * semantic einsum + panoptic argmax and area counters for image b of the last head_forward.
 *   kscore [Q] fp32 device: score of kept queries (label != null, score > object_mask_threshold), < 0 for dropped queries
 *   semT   [K,Q] fp32 device = softmax(mask_cls)[:, :-1]^T, or NULL
 *   sem_seg [K,out_h,out_w] fp32 / ids [out_h*out_w] int32 (kept-query index | 1<<16 if inside the mask, -1 if none) /
 *   counts [3*Q] int32 (mask_area, original_area, intersection) / inst_stats [2*Qpad] fp32 (sum of prob over positive pixels,
 *   positive pixel count; Qpad = Q rounded up to 8): device pointers, each optional */
int odise_hip_postprocess_pixels(odise_hip_ctx* ctx, int b, const float* kscore, const float* semT, int K, int pad_h, int pad_w,
                                 int img_h, int img_w, int out_h, int out_w, float* sem_seg, int* ids, int* counts, float* inst_stats);
/* seg[p] = map[q] for pixels whose argmax query q is inside its own mask, else 0 (maskformer_model.py:321-333) */
int odise_hip_panoptic_write(odise_hip_ctx* ctx, const int* ids, const int* map, int* seg, int npix);
/* out [n,out_h,out_w] fp32 = (upsampled mask logit of query idx[i] > 0)  (maskformer_model.py:371) */
int odise_hip_instance_masks(odise_hip_ctx* ctx, int b, const int* idx, int n, int pad_h, int pad_w, int img_h, int img_w, int out_h,
                             int out_w, float* out);

/* ---- the three inference heads for a whole batch, decisions on the device (odise.py:336-370; maskformer_model.py:280-380) --------
 * Consumes the mask logits of the last odise_hip_head_forward and mask_cls of odise_hip_classify.  Everything the reference decides
 * on the host from device tensors - kept queries, the per-segment loop with its `.item()` round trips (maskformer_model.py:312-340),
 * the top-k of the instance head (:349-369) - is decided by kernels, so a call enqueues work and never synchronises; the caller reads
 * the small tables back when it needs them.  Per image b the outputs are (HOST arrays of B device pointers; an array or an entry may
 * be NULL to skip that output):
 *   sem_seg[b]     fp32 [K, oh, ow]                    semantic_inference (:280-284)
 *   sem_argmax[b]  int32 [oh*ow]                       argmax over classes of the same scores WITHOUT materialising [K, oh, ow]
 *                                                      (what detectron2's SemSegEvaluator keeps; A-847 at 1280x1280 is 5.5 GB otherwise)
 *   panoptic[b]    int32 record [oh*ow | 1 | 3*ODISE_MAX_SEGMENTS]: panoptic ids, n_segments, (id, isthing, category_id) rows -
 *                  the per-image record of the multi-GPU exchange (odise_hip_allgather_predictions).  The reference's list of segments
 *                  is unbounded, the record is not: of more than ODISE_MAX_SEGMENTS surviving segments the first ODISE_MAX_SEGMENTS in
 *                  query order are kept; a later one gets no id and consumes none (its pixels are 0 in the map), a later query of a
 *                  stuff class that was emitted before the cap still merges into that segment.  Every non-zero id of the map has a
 *                  row, rows past n_segments are zero.
 *   inst_masks[b]  fp32 [topk, oh, ow] (first n valid) ; inst_table (device, [B][1 + 2*topk] int32: n | query index | class) ;
 *                  inst_scores (device, [B][topk] fp32), sorted by class score descending (instance_inference, :344-380) */
#define ODISE_MAX_SEGMENTS 100
typedef struct {
    int B;                        /* batch of the last head_forward */
    int pad_h, pad_w;             /* padded network input size (ImageList.from_tensors(images, size_divisibility), odise.py:240) */
    const int* img_hw;            /* HOST [B][2] true image sizes (the crop of sem_seg_postprocess) */
    const int* out_hw;            /* HOST [B][2] requested output sizes ("height" / "width" of the input dicts) */
    const float* mask_cls;        /* device [B,Q,K+1] log-probabilities (output of odise_hip_classify) */
    const uint8_t* isthing;       /* HOST [K]: 1 for "thing" classes (metadata.thing_dataset_id_to_contiguous_id) */
    int semantic_on, panoptic_on, instance_on;
    float object_mask_threshold;  /* maskformer_model.py:290 */
    double overlap_threshold;     /* :318 (double: compared against an integer ratio exactly like the reference's Python float) */
    int topk;                     /* test_topk_per_image */
    float* const* sem_seg;
    int32_t* const* sem_argmax;
    int32_t* const* panoptic;
    float* const* inst_masks;
    int32_t* inst_table;
    float* inst_scores;
} odise_post_desc;
int odise_hip_postprocess_batch(odise_hip_ctx* ctx, const odise_post_desc* d);

/* ---- CategoryODISE.forward / CaptionODISE.forward, eval branch, as ONE call (odise.py:236-246, 282-372; the call
 * `self.model(batched_inputs)` of OpenPanopticInference.forward, odise/modeling/wrapper/pano_wrapper.py:64) ------------------------
 * images[b]: device pointer to image b, uint8 [h_b, w_b, 3] (image_layout 0: HWC, the DatasetMapper's decoded picture),
 * uint8 [3, h_b, w_b] (1: CHW, the "image" tensor of the reference's input dicts) or fp32 [3, h_b, w_b] with values 0..255 (2).
 * The library normalises ((x - 0) / 255), pads to the batch maximum rounded up to 64 (backbone input) and to the batch maximum
 * (MaskCLIP input, odise.py:242-244), runs backbone -> head -> classification -> the three heads.  post.B / pad_h / pad_w / img_hw /
 * mask_cls are filled in by the library (post.out_hw NULL = image sizes).  mask_cls_out (optional): device [B,Q,K+1] fp32. */
typedef struct {
    int B;
    const void* const* images;    /* HOST [B] device pointers */
    int image_layout;
    const int* img_hw;            /* HOST [B][2] */
    float* mask_cls_out;
    odise_post_desc post;
} odise_infer_desc;
int odise_hip_infer(odise_hip_ctx* ctx, const odise_infer_desc* d);
/* Encoder prefetch for a stream of batches (the reference's evaluation loop consumes a prefetching loader: odise/evaluation/evaluator.py:
 * 87-126, odise/data/build.py:138-151).  Registers the NEXT batch (only B / images / image_layout / img_hw of `next` are read; the image
 * buffers must stay valid and unchanged until that batch's own odise_hip_infer returns): the following odise_hip_infer call, once the VAE
 * lane of ITS batch is done, enqueues the next batch's normalise / pad, window extraction, VAE encoder and latent on a lowest-priority
 * stream into a side arena, and the odise_hip_infer of exactly that batch (same pointers, layout and sizes) starts from the stored latent
 * and encoder taps.  Same kernels on the same shapes: every output is bit-identical to the call without prefetch.  A prefetched batch that
 * is not the next one inferred is dropped.  next == NULL cancels a registration. */
int odise_hip_infer_prefetch(odise_hip_ctx* ctx, const odise_infer_desc* next);

/* ---- input resize and evaluator reductions of the eval loop --------------------------------------------
 * Replaces, on device buffers: detectron2 T.ResizeShortestEdge -> PIL.Image.resize(BILINEAR) of the DatasetMapper
 * (configs/common/data/pano_open_d2_eval.py:74-107) and the per-pixel parts of the evaluators configured there
 * (odise/evaluation/d2_evaluator.py:49 COCOPanopticEvaluator -> panopticapi pq_compute_single_core, :63 SemSegEvaluator.process).
 * Per picture each evaluator is one asynchronous call that adds into a small accumulator: odise_hip_semantic_confusion /
 * odise_hip_semantic_boundary_confusion (SemSegEvaluator), odise_hip_panoptic_quality (COCOPanopticEvaluator, straight from the panoptic
 * record), odise_hip_instance_eval (InstanceSegEvaluator / COCOEvaluator with tasks=("segm",), d2_evaluator.py:29,104: COCOeval.evaluateImg
 * of a picture, straight from the mask logits; one fixed-size row per detection, reduced on the host by odise_amd/instance_eval.py).
 * odise_hip_pair_histogram is the bare per-pixel part of the panoptic one, odise_hip_mask_iou that of the segm one; odise_hip_instance_rle
 * writes the RLE strings of coco_instances_results.json, which the metric no longer needs. */
/* src uint8 [H,W,C] -> dst uint8 [OH,OW,C], bit-identical to Pillow's 8-bit bilinear resampler (horizontal pass, then vertical) */
int odise_hip_resize_bilinear_u8(odise_hip_ctx* ctx, const void* src, int H, int W, int C, void* dst, int OH, int OW);
/* dst fp32 [C,H,W] = scale * src uint8 [H,W,C] */
int odise_hip_u8_hwc_to_f32_chw(odise_hip_ctx* ctx, const void* src, float* dst, int H, int W, int C, float scale);
/* dst fp32 [C,Hp,Wp] = the same, zero padded at the bottom / right (detectron2 ImageList.from_tensors(images, size_divisibility),
 * odise.py:240) */
int odise_hip_u8_hwc_to_f32_chw_padded(odise_hip_ctx* ctx, const void* src, float* dst, int H, int W, int C, int Hp, int Wp, float scale);
/* conf int64 [(K+1)*(K+1)] += count of (argmax_k sem_seg[k,p], gt[p]); gt outside [0,K] (ignore label) counts in column K.
 * The caller zeroes conf before the first image and sums it across ranks (all-gather / all-reduce of (K+1)^2 int64). */
int odise_hip_semantic_confusion(odise_hip_ctx* ctx, const float* sem_seg, const int* gt, int K, int npix, int64_t* conf);
/* The evaluator's second matrix (_b_conf_matrix, Boundary IoU; detectron2 fills it when OpenCV is importable and K < 255).
 * _mask_to_boundary(m) = m - erode(m): a 3x3 minimum behind a one-pixel ring of zeros, `radius` times; equivalently e = 0 within
 * `radius` of an edge and the (2 radius + 1)^2 window minimum elsewhere.  m - e is a LABEL DIFFERENCE in 0..K, as in the evaluator.
 * radius of an H x W picture: max(1, int(round(0.02 * sqrt(H*H + W*W)))), Python's round; negative error for H or W < 1.  No context. */
int odise_hip_boundary_radius(int H, int W);
/* boundary int32 [H,W] = _mask_to_boundary(labels int32 [H,W] (device), values outside [0,K] taken as K); radius <= 0: the formula.
 * 1 <= K <= 254.  Scratch comes from the context.  Asynchronous on the context's stream. */
int odise_hip_label_boundary(odise_hip_ctx* ctx, const int* labels, int K, int H, int W, int radius, int* boundary);
/* One SemSegEvaluator.process step of a picture: sem_seg fp32 [K,H,W], gt int32 [H,W].  conf (optional) += exactly what
 * odise_hip_semantic_confusion adds; b_conf int64 [(K+1)*(K+1)] += count of (boundary(argmax)[p], boundary(gt)[p]), rows = prediction.
 * Neither is cleared.  radius <= 0: the formula.  K > 254 is ODISE_ERR_ARG (the evaluator computes no Boundary IoU there) and writes nothing. */
int odise_hip_semantic_boundary_confusion(odise_hip_ctx* ctx, const float* sem_seg, const int* gt, int K, int H, int W, int radius,
                                          int64_t* conf, int64_t* b_conf);
/* One WHOLE SemSegEvaluator.process step of a picture (d2_evaluator.py:63 -> detectron2 SemSegEvaluator.process), from the prediction as
 * it lies in HBM: the counters above and the per-class COCO RLE strings of sem_seg_predictions.json (encode_json_sem_seg: for every label
 * of np.unique(pred), mask.encode of (pred == label)).  Host restatement: odise_amd/semseg_eval.py.
 * Prediction, exactly one of: labels int32 [H,W] (the fused arg-max map, sem_argmax of odise_post_desc), or sem_seg fp32 [K,H,W], whose
 * first-maximum arg-max (ties to the lower class, as odise_hip_semantic_confusion takes it) is taken ONCE into scratch; every later
 * stage reads labels.
 * Counting (conf and / or b_conf non-NULL; needs gt int32 [H,W], a gt outside [0,K] counts in column K): conf int64 [(K+1)^2] += exactly
 * what odise_hip_semantic_confusion adds, b_conf += exactly what odise_hip_semantic_boundary_confusion adds (radius <= 0: the formula);
 * rows are the prediction.  A non-NULL b_conf with K > 254 is ODISE_ERR_ARG.
 * Per-class RLE (offsets non-NULL; then classes and n_classes are required): classes int32 [max_classes] = the classes present in
 * ASCENDING order (np.unique's), -1 past the count; n_classes int32 [1] = how many are present, also when that exceeds max_classes (then
 * the first max_classes are encoded); rle / capacity / offsets int64 [max_classes+1] / area int64 [max_classes] (optional) as
 * odise_hip_rle_encode: offsets always complete, nothing written past capacity, strings written only when offsets[max_classes] <=
 * capacity, entries past the count are empty strings of area 0.  String i is byte-identical to
 * mask.encode(np.asfortranarray((pred == classes[i]).astype(np.uint8)))["counts"].
 * flags int32 [1], OR-ed: 1 = a label outside [0,K) in `labels`; that pixel is counted in neither matrix's class rows (in the boundary
 * maps it stands as K, as odise_hip_label_boundary takes it) and is a zero in every class mask.
 * ODISE_ERR_ARG and nothing written: a null or doubled prediction, null flags, counting outputs without gt, neither counting nor RLE
 * asked for, H or W < 1, H * W > 2^29 - 1, K outside 1..12288, max_classes outside 1..65535 (with RLE), a negative capacity or one
 * without a buffer.  Scratch comes from the context's growable buffers.  Asynchronous on the context's stream. */
typedef struct {
    int K, H, W;
    const int32_t* labels;        /* device [H,W], or NULL */
    const float* sem_seg;         /* device [K,H,W], or NULL */
    const int32_t* gt;            /* device [H,W]; NULL = no counting */
    int radius;
    int64_t* conf;                /* device [(K+1)^2], optional */
    int64_t* b_conf;              /* device [(K+1)^2], optional */
    int max_classes;              /* 1..65535 */
    int32_t* classes;             /* device [max_classes] */
    int32_t* n_classes;           /* device [1] */
    void* rle; int64_t capacity;  /* device bytes */
    int64_t* offsets;             /* device [max_classes + 1]; NULL = no RLE */
    int64_t* area;                /* device [max_classes], optional */
    int32_t* flags;               /* device [1] */
} odise_semseg_eval_desc;
int odise_hip_semantic_eval(odise_hip_ctx* ctx, const odise_semseg_eval_desc* d);
/* hist int32 [na*nb] += count of (a[p], b[p]) pairs with 0 <= a < na, 0 <= b < nb (segment-index co-occurrence of PQ matching) */
int odise_hip_pair_histogram(odise_hip_ctx* ctx, const int* a, const int* b, int npix, int na, int nb, int* hist);
/* One picture of COCOPanopticEvaluator's metric (d2_evaluator.py:49 -> panopticapi pq_compute_single_core) without the PNG round trip:
 * the prediction is the panoptic record of odise_post_desc as it lies in HBM, the ground truth the annotation PNG as decoded plus its
 * segments_info table.  `stats` is ADDED to and never cleared: the caller zeroes it before the first picture, sums it across ranks once
 * (odise_amd.distributed.sum_pq_stats) and turns it into PQ / SQ / RQ on the host (odise_amd/panoptic_quality.py, which also restates
 * the rules below in numpy).  Ids are 24-bit values (the PNG format), 0 = VOID on both sides; in a table the first row of an id counts.
 *   pred area of a segment = its pixels in pred_ids; inter[g][p] = pixels with gt id g and pred id p; gt ids that are not in gt_segments
 *   take part in nothing except as "not VOID".
 *   matching   pairs (g, p) with both ids in their tables, inter > 0, iscrowd[g] == 0 and equal categories:
 *              union = area_pred[p] + area_gt[g] - inter[g][p] - inter[VOID][p]  (area_gt from the table, i.e. the annotation JSON);
 *              iou = inter / union as a double division of the two integers (a union <= 0 matches nothing); iou > 0.5: tp[cat] += 1,
 *              iou[cat] += iou, g and p are matched.  The pairs are added one by one in ascending (g, p) order onto the value already in
 *              `stats`, so the sums of a stream of pictures are bit-identical to the single-process evaluator and from run to run.
 *   fn         unmatched gt rows in table order: a crowd row sets crowd_of[cat] (the last one wins) and counts nothing, every other row
 *              - with or without pixels in the map - counts fn[cat] += 1.
 *   fp         unmatched pred rows: ign = inter[VOID][p] (+ inter[crowd_of[cat_p]][p]); ign / area_pred[p] > 0.5 skips the row, otherwise
 *              fp[cat_p] += 1.  Both thresholds are strict.
 * flags (OR-ed in; a picture that raises one adds nothing to stats; the reference raises KeyError for the first two):
 *   1 = a non-zero id of pred_ids is missing from pred_segments, 2 = a pred_segments row has no pixel, 4 = a predicted category outside
 *   [0, num_categories).
 * ODISE_ERR_ARG and nothing written: a null pointer, H * W > 2^29 - 1, n_gt > 254, a ground-truth category outside [0, num_categories), iscrowd not 0 / 1.
 * Asynchronous on the context's stream.  Scratch belongs to the context: it is allocated once, at the first call, at the caps (a matrix of
 * 256 x (ODISE_MAX_SEGMENTS + 2) int32, the second matrix of odise_hip_panoptic_quality_boundary, the device table, 8 pinned table slots;
 * about 250 KB), never resized, and released with the context.  The pixel pass sizes its LDS histogram to the real n_gt but, since n is read on the device, to ODISE_MAX_SEGMENTS on the
 * predicted side (at most 48 KiB); tables beyond that count in the matrix directly. */
typedef struct { double iou; int64_t tp, fp, fn; } odise_pq_stat;      /* one per category, 32 bytes */
typedef struct {
    int H, W;
    const int32_t* pred_ids;      /* device [H*W] panoptic ids: the first H*W ints of the panoptic record */
    const int32_t* pred_segments; /* device: n | n rows (id, isthing, category_id) - the tail of the same record; n is read on the device,
                                     n <= ODISE_MAX_SEGMENTS */
    const void* gt;               /* device: gt_layout 0 = uint8 [H,W,3] RGB as Pillow decodes the annotation PNG (id = R + 256 G + 65536 B,
                                     converted on the device), 1 = int32 [H*W] ids */
    int gt_layout;
    const int32_t* gt_segments;   /* HOST [n_gt][4] rows (id, category_id, iscrowd, area); copied before the call returns */
    int n_gt;                     /* 0 .. 254 */
    int num_categories;           /* both tables carry categories 0 .. num_categories - 1 (the caller maps dataset ids) */
    odise_pq_stat* stats;         /* device [num_categories] */
    int32_t* flags;               /* device [1] */
} odise_pq_desc;
int odise_hip_panoptic_quality(odise_hip_ctx* ctx, const odise_pq_desc* d);
/* The same picture with Boundary PQ beside PQ (Cheng et al., "Boundary IoU", CVPR 2021: PQ with min(mask IoU, boundary IoU) in place of
 * the mask IoU).  d->stats += exactly what odise_hip_panoptic_quality adds, bit for bit; b->stats += the Boundary PQ statistics; both
 * come from one translation of the two id maps.  This is the project's restatement of the paper's rule on pq_compute_single_core; parity
 * with the published boundary-iou package is UNPINNED (the package was never run beside it).  Host restatement:
 * odise_amd/panoptic_quality.py image_boundary_stats.
 *   radius     b->radius > 0, else odise_hip_boundary_radius(H, W), as the other two boundary measures.
 *   B(s)       the boundary of segment s = its pixels minus their erosion (`radius` 3x3 erosions behind a ring of zeros: the binary
 *              odise_hip_mask_boundary of its mask).  Equivalently a pixel of s lies in B(s) when its (2 radius + 1)^2 window leaves the
 *              picture or holds a pixel that is not of s; VOID and ids missing from a table are neighbours like any other.  With
 *              2 radius + 1 > min(H, W) every pixel is a boundary pixel.
 *   b_iou      of a candidate pair (g, p) - the candidates are those of PQ -: inter_b = |B(g) & B(p)|,
 *              union_b = |B(p)| + |B(g)| - inter_b - |B(p) over ground-truth VOID|  (|B(g)| counted from the map: the JSON holds none),
 *              b_iou = inter_b / union_b as the double division of the two integers, 0 when union_b <= 0.
 *   matching   iou_b = fmin(iou, b_iou) with iou exactly that of odise_hip_panoptic_quality (JSON area included); iou_b > 0.5:
 *              tp[cat] += 1, iou[cat] += iou_b, in ascending (g, p) order onto the value already in b->stats.
 *   fn, fp     follow from this matching by the unchanged rules; the fp skip test uses mask areas, VOID and the crowd row.
 *   flags      the same three; a flagged picture adds nothing to either accumulator.
 * ODISE_ERR_ARG and nothing enqueued: what odise_hip_panoptic_quality refuses, a null b or b->stats, b->stats overlapping d->stats.
 * Asynchronous on the context's stream.  Scratch: the context's second matrix ((254 + 3) x (ODISE_MAX_SEGMENTS + 3) int32, allocated with
 * the first) and its growable boundary scratch (four byte maps - both slot maps and their complements - their erosions and a spare). */
typedef struct { odise_pq_stat* stats; int radius; } odise_pq_boundary_task;   /* device [num_categories]; radius <= 0: the formula */
int odise_hip_panoptic_quality_boundary(odise_hip_ctx* ctx, const odise_pq_desc* d, const odise_pq_boundary_task* b);
/* Panoptic quality of a SEMANTIC segmentation (Mask2Former tools/evaluate_pq_for_semantic_segmentation.py: the PQ number of the
 * semantic-only evaluation sets), one picture.  Every class of the picture is one stuff segment on either side, pictures accumulate in
 * one odise_pq_stat per class.  Host restatement: odise_amd/semseg_pq.py.
 * Prediction, exactly one of: labels int32 [H,W], or sem_seg fp32 [K,H,W] whose first-maximum arg-max (ties to the lower class, as
 * odise_hip_semantic_confusion takes it) is taken per pixel.  gt int32 [H,W] follows the contract of odise_hip_semantic_eval: the
 * ignore label already mapped to K, any value outside [0,K] counts as K = VOID.  (A ground-truth value that is neither a class nor the
 * ignore label would be a segment of an unknown category in the tool; here it is VOID.)
 *   counts     area_pred[c] = pixels with pred == c, area_gt[c] = pixels with gt == c, inter[c] = pixels with both,
 *              void_pred[c] = pixels with pred == c on VOID.  A class is present on a side when its area there is > 0.
 *   matching   only a class with itself, when inter[c] > 0: union = area_pred[c] + area_gt[c] - inter[c] - void_pred[c],
 *              iou = inter / union as the double division of the two integers; iou > 0.5 (strict): tp[c] += 1, iou[c] += iou.
 *   fn, fp     a ground-truth class present and unmatched: fn[c] += 1.  A predicted class present and unmatched: skipped when
 *              void_pred[c] / area_pred[c] > 0.5 (strict), otherwise fp[c] += 1.
 * `stats` [K] is ADDED to and never cleared.  One adder per class and the pictures of a stream in order: the iou sums grow by one addend
 * per picture, bit-identical to the tool's in picture order and from run to run.  PQ / SQ / RQ follow on the host with every class a
 * stuff class (odise_amd/panoptic_quality.py pq_average).
 * flags int32 [1], OR-ed: 1 = a label outside [0,K) in `labels` (the flag of odise_hip_semantic_eval); a picture that raises it adds
 * nothing to `stats`, and the next picture counts as if it had not been there.
 * ODISE_ERR_ARG and nothing written: a null pointer, both or neither prediction, H or W < 1, H * W > 2^29 - 1, K outside 1..12288.
 * Scratch (4 K int32 counters, in LDS while the pixels are swept for K <= 3072) comes from the context and grows with K.
 * Asynchronous on the context's stream. */
int odise_hip_semantic_pq(odise_hip_ctx* ctx, const int32_t* labels, const float* sem_seg, const int32_t* gt, int K, int H, int W,
                          odise_pq_stat* stats, int32_t* flags);
/* odise_hip_semantic_eval(ctx, d) with these statistics beside it: conf, b_conf, classes, the RLE strings and flags exactly as that call
 * leaves them, bit for bit, and t->stats [d->K] += what odise_hip_semantic_pq adds, from the same label map (the arg-max of a score
 * tensor is taken once for all of it).  Needs d->gt; the statistics alone (no conf, no b_conf, no offsets) are allowed.  A caller that
 * enqueues a picture again for its strings (capacity, max_classes) uses odise_hip_semantic_eval for that, as for the matrices.
 * ODISE_ERR_ARG and nothing enqueued: what odise_hip_semantic_eval refuses, a null t, t->stats or d->gt, statistics not 8-byte aligned. */
typedef struct { odise_pq_stat* stats; } odise_semseg_pq_task;   /* device [K] */
int odise_hip_semantic_eval_pq(odise_hip_ctx* ctx, const odise_semseg_eval_desc* d, const odise_semseg_pq_task* t);
/* The erosion stage of the call above on one id map: boundary uint8 [H,W] = 1 where the pixel lies on the boundary B(s) of its own
 * segment; ids int32 [H,W] (device); table device int32 [n] ids, n <= 254 (the first row of an id counts).  Pixels of id 0 and of ids
 * absent from the table: 0.  area int64 [n] (optional) = the pixels of each row's boundary.  radius <= 0: the formula.  Same slot and
 * erosion code as the evaluator call.  Asynchronous on the context's stream. */
int odise_hip_segment_boundaries(odise_hip_ctx* ctx, const int32_t* ids, int H, int W, const int32_t* table, int n, int radius,
                                 uint8_t* boundary, int64_t* area);
/* COCO compressed RLE (pycocotools mask.encode of the Fortran-ordered mask, counts as text) of n masks: the per-mask part of the segm
 * evaluators (COCOEvaluator / InstanceSegEvaluator(tasks=("segm",)) -> detectron2 instances_to_coco_json), byte-identical to
 * `mask.encode(np.asfortranarray(m.astype(np.uint8)))["counts"].decode("utf-8")` (maskApi.c rleEncode + rleToString).
 * masks: device row-major [n, h, w] (the layout of pred_masks), dtype ODISE_F32 or ODISE_U8 (bool); any nonzero value is 1.
 * rle: device bytes, all strings packed back to back, no terminators; bytes past `capacity` are never written.
 * offsets: device int64 [n+1], exclusive scan of string lengths (always complete; offsets[n] > capacity => strings not written,
 * call again with capacity >= offsets[n]).  area: device int64 [n] (optional), the pixels of each mask.  Scratch comes from the context.
 * h * w <= 2^30, n <= 65535.  Asynchronous on the context's stream. */
int odise_hip_rle_encode(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w,
                         void* rle, int64_t capacity, int64_t* offsets, int64_t* area);
/* the same for the instance head's selection of image b of the last head forward, straight from the mask logits (the pixels of
 * odise_hip_instance_masks, with the taps of its x4 form where that form applies; no [topk,oh,ow] tensor): inst_table = device row
 * [1 + 2*topk] of that image (inst_table of odise_post_desc; the count is read on the device); pad_h / pad_w = 4 x the mask-logit size,
 * as in odise_hip_postprocess_batch.  offsets [topk+1], area [topk]: entries
 * past the count are empty strings of area 0.  Enqueue it after odise_hip_postprocess_batch / odise_hip_infer of the same batch. */
int odise_hip_instance_rle(odise_hip_ctx* ctx, int b, const int* inst_table, int topk, int pad_h, int pad_w, int img_h, int img_w,
                           int out_h, int out_w, void* rle, int64_t capacity, int64_t* offsets, int64_t* area);
/* pycocotools' mask.iou of n dense masks (layout / dtype as odise_hip_rle_encode) against n_gt run-length masks of the same size.
 * gt_runs: device uint32, the UNCOMPRESSED counts of all masks back to back - runs over the column-major order j = x * h + y, starting
 * with the zeros and alternating (coco_rle.string_to_counts of a compressed string); zero-length runs are legal anywhere.
 * gt_offsets: device int64 [n_gt + 1], the first count of every mask.  iscrowd: device uint8 [n_gt] or NULL (none is).
 * iou: device double [n][n_gt] = rleIou: inter == 0 -> 0, crowd -> inter / area_d, else inter / (area_d + area_g - inter), the double
 * division of exact integers.  inter int32 [n][n_gt], area_d int64 [n], area_g int64 [n_gt]: optional.
 * flags: device int32 [1], OR-ed: 1 = the counts of a mask do not sum to h * w (its missing tail is zeros, what lies past the end is
 * dropped; no access leaves a buffer).  n == 0 or n_gt == 0 writes nothing and succeeds.  n, n_gt <= 65535, n * n_gt <= 2^26,
 * h * w <= 2^30.  Scratch comes from the context.  Asynchronous on the context's stream. */
int odise_hip_mask_iou(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, const uint32_t* gt_runs,
                       const int64_t* gt_offsets, int n_gt, const uint8_t* iscrowd, double* iou, int32_t* inter, int64_t* area_d,
                       int64_t* area_g, int32_t* flags);
/* One picture of COCOeval.evaluateImg for iouType "segm", useCats = 1, maxDets 100, in all four area ranges ([0, 1e10], [0, 32^2],
 * [32^2, 96^2], [96^2, 1e10], ends included) and at the ten IoU thresholds the caller passes (np.linspace(.5, .95, 10) as doubles).
 * Per (category, range a, threshold t): detections in descending score, ties in table order; a ground truth is ignored when it is a
 * crowd or its area lies outside range a (the caller computes these bits from the annotation's float area); non-ignored ground truths
 * come first, each group in annotation order.  A detection starts from best = min(t, 1 - 1e-10) and walks the ground truths: one already
 * matched at (a, t) that is no crowd is skipped; the walk stops at the first ignored one once a non-ignored match is held; iou < best is
 * skipped; otherwise best = iou and the match moves there (on equal values to the later one).  A matched detection takes the ignore bit of
 * its ground truth; an unmatched one is ignored when its own area (pixels of its mask) lies outside range a.
 * Row k is the detection of rank k by score: what COCOeval.accumulate needs of it (odise_amd/instance_eval.py accumulate / summarize).
 * ODISE_ERR_ARG and nothing written: a null pointer, topk outside 1..100, n_gt outside 0..1024, the geometry errors of
 * odise_hip_instance_rle.  Polygon ground truth goes through odise_hip_instance_eval_poly below.
 * The matching is one block: a wave per category, so a picture whose detections and ground truths all share one category is matched
 * by one wave.  Scratch comes from the context.  Asynchronous on the context's stream; no host synchronisation. */
typedef struct { float score; int32_t category; int32_t area; int32_t image; uint64_t matched, ignored; } odise_inst_eval_row; /* 32 bytes; bit 10*a + t */
typedef struct {
    int h, w;                       /* output size of the picture */
    /* detections, one of: */
    const void* masks; int dtype;   /* dense [topk,h,w] (ODISE_F32 / ODISE_U8), or NULL = from the mask logits of image b of the last head forward: */
    int b, pad_h, pad_w, img_h, img_w;   /* as odise_hip_instance_rle */
    const int32_t* inst_table;      /* device [1 + 2*topk]: n | query index | class  (n read on the device) */
    const float* inst_scores;       /* device [topk] */
    int topk;                       /* 1..100: the evaluator looks at no more than 100 detections per picture and category */
    /* ground truth, all device: */
    const uint32_t* gt_runs; const int64_t* gt_offsets;   /* as odise_hip_mask_iou */
    const int32_t* gt_rows;         /* [n_gt][3]: contiguous category, iscrowd, bits 0..3 = area outside range a */
    int n_gt;                       /* 0..1024 */
    int num_categories; int image;  /* `image` is copied into every row */
    const double* iou_thresholds;   /* HOST [10], copied by value into the launch */
    odise_inst_eval_row* rows;      /* device [topk]; rows past n are zeroed */
    int32_t* n_rows;                /* device [1] */
    int32_t* flags;                 /* device [1], OR-ed: 1 = a gt mask's runs do not sum to h*w, 2 = a detection's class outside [0,num_categories),
                                       4 = a gt category outside it / iscrowd not 0|1 (odise_hip_instance_eval_poly: or runs AND polygons on one gt; 8 = a bad
                                       polygon).  A picture that raises one writes n_rows = 0 and zeroed rows. */
} odise_inst_eval_desc;
int odise_hip_instance_eval(odise_hip_ctx* ctx, const odise_inst_eval_desc* d);
/* pycocotools' annToRLE of polygon annotations (mask.frPyObjects of every polygon + mask.merge as a union): maskApi.c rleFrPoly bit for
 * bit - vertices scaled by 5 and rounded as (int)(5 v + .5), every edge walked in max(dx, dy) + 1 points with separately rounded
 * multiply and add (no fused multiply-add), a crossing wherever two consecutive points differ in x; the mask is the running parity of the
 * crossings over the column-major order, and an annotation is the OR of its polygons.
 * xy: device double, the vertices x0 y0 x1 y1 .. of all polygons back to back.  poly_offsets: device int64 [n_poly + 1], the first VERTEX
 * of every polygon (poly_offsets[n_poly] vertices are read from xy).  ann_polys: device int32 [n_ann + 1], the first polygon of every
 * annotation; an annotation with no polygons is the empty mask.  rle / capacity / offsets / area: exactly as odise_hip_rle_encode.
 * flags: device int32 [1], OR-ed: 8 = a polygon has fewer than 3 vertices, or a coordinate is NaN or larger than 2^26 in magnitude (5 x
 * must fit an int); such a polygon contributes nothing.  Polygon ranges are clamped to [0, n_poly]: no access leaves a buffer.
 * n_ann <= 65535, n_poly >= 0, h * w <= 2^30.  Scratch comes from the context.  Asynchronous on the context's stream. */
int odise_hip_polygon_rle(odise_hip_ctx* ctx, const double* xy, const int64_t* poly_offsets, const int32_t* ann_polys, int n_ann, int n_poly,
                          int h, int w, void* rle, int64_t capacity, int64_t* offsets, int64_t* area, int32_t* flags);
/* odise_hip_instance_eval with ground truth that is polygons, run lengths, or both in one picture (COCO: polygons for every object, RLE
 * for the crowds).  p: the polygons as in odise_hip_polygon_rle, gt_polys [n_gt + 1] the polygon range of every ground truth.  A ground
 * truth with a non-empty polygon range must have an EMPTY run range in d->gt_offsets (flag 4 otherwise); its mask is rasterised into the
 * words the run-length decoder fills for the others, and intersections, IoU and matching are those of odise_hip_instance_eval.
 * Flag 8 (odise_hip_polygon_rle) joins the flags of the descriptor: the picture writes n_rows = 0 and zeroed rows.
 * p == NULL is odise_hip_instance_eval. */
typedef struct {
    const double* xy;               /* device: vertices of all polygons */
    const int64_t* poly_offsets;    /* device [n_poly + 1], in vertices */
    const int32_t* gt_polys;        /* device [n_gt + 1] */
    int n_poly;
} odise_inst_poly_gt;
int odise_hip_instance_eval_poly(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p);
/* The boxes of a picture's instance selection: detectron2 BitMasks.get_bounding_boxes of every mask, XYXY = [first column with a pixel,
 * first row with a pixel, last column + 1, last row + 1], a mask without a pixel [0, 0, 0, 0] - the line maskformer_model.py:372 leaves
 * commented out ("this is slow"), which is why the reference's pred_boxes are zeros.  The detections are those of odise_inst_eval_desc:
 * dense `masks` [topk,h,w] (inst_table optional: NULL = all topk), or masks == NULL = the selection inst_table of image b of the last
 * head forward, sampled from the mask logits.  Rows past the count of the table are zeros.  ODISE_ERR_ARG and nothing written: a null
 * required pointer, topk outside 1..100, h or w < 1, h * w > 2^30, a dtype other than ODISE_F32 / ODISE_U8, the geometry errors of
 * odise_hip_instance_rle.  Scratch comes from the context.  Asynchronous on the context's stream; no host synchronisation. */
typedef struct {
    int h, w;
    const void* masks; int dtype;
    int b, pad_h, pad_w, img_h, img_w;
    const int32_t* inst_table;
    const float* inst_scores;       /* unused, may be NULL */
    int topk;
    float* boxes;                   /* device [topk][4] XYXY; rows past the count are zeros */
} odise_inst_boxes_desc;
int odise_hip_instance_boxes(odise_hip_ctx* ctx, const odise_inst_boxes_desc* d);
/* pycocotools' mask.iou of boxes: maskApi.c bbIou of n XYWH boxes against n_gt XYWH boxes, all device doubles.  With D a box of dt and G
 * one of gt: da = D.w * D.h, ga = G.w * G.h, w = fmin(D.x + D.w, G.x + G.w) - fmax(D.x, G.x), h the same in y; w <= 0 or h <= 0 -> 0;
 * i = w * h; iou = i / (crowd ? da : da + ga - i), every operation rounded on its own (no fused multiply-add).  iscrowd: device uint8
 * [n_gt] or NULL.  iou: device double [n][n_gt].  n == 0 or n_gt == 0 writes nothing and succeeds.  n, n_gt <= 65535, n * n_gt <= 2^26.
 * Asynchronous on the context's stream. */
int odise_hip_box_iou(odise_hip_ctx* ctx, const double* dt, int n, const double* gt, int n_gt, const uint8_t* iscrowd, double* iou);
/* COCOeval.evaluateImg for iouType "bbox", optionally together with "segm", from ONE pack of the detections (sampling the mask logits is
 * the expensive part of either).  The detection boxes are those of odise_hip_instance_boxes as XYWH, the IoU is odise_hip_box_iou against
 * bb->gt_boxes, and the walk is the one of odise_hip_instance_eval.  A bbox row's `area` is its box's w * h (COCO.loadRes' bb[2] * bb[3]),
 * which is also what the ignore rule of an unmatched detection looks at; the ignore bits of the ground truth are d->gt_rows for both tasks
 * (COCO compares the annotation's `area` in both).
 * segm part: with d->rows and d->n_rows set it is exactly odise_hip_instance_eval_poly(d, p).  With both NULL it is skipped, and
 * d->gt_runs / d->gt_offsets / p are not read.
 * d->flags collects the flags of both tasks.  For bbox, 4 is also raised by a ground-truth box with a non-finite member, and 1 cannot
 * occur.  Flags 1 and 8 zero the segm rows only (n_rows = 0); flags 2 and 4 zero the rows of both tasks.
 * ODISE_ERR_ARG and nothing written: what odise_hip_instance_eval refuses, a null bb, bb->rows or bb->n_rows, a null bb->gt_boxes with
 * n_gt > 0, only one of d->rows / d->n_rows.  Scratch comes from the context.  Asynchronous on the context's stream; no host
 * synchronisation. */
typedef struct {
    const double* gt_boxes;         /* device [n_gt][4] XYWH */
    odise_inst_eval_row* rows;      /* device [topk] */
    int32_t* n_rows;                /* device [1] */
    float* boxes;                   /* device [topk][4] XYXY, optional */
} odise_inst_bbox_task;
int odise_hip_instance_eval_bbox(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p, const odise_inst_bbox_task* bb);
/* The boundaries of n dense masks (layout / dtype as odise_hip_rle_encode): boundary = mask & ~erode(mask), the rule of Boundary IoU (Cheng
 * et al., CVPR 2021) and of detectron2's _mask_to_boundary on a binary mask - erode is the (2 r + 1)^2 minimum that sees zeros outside the
 * picture (r 3x3 erosions behind a ring of zeros); with 2 r + 1 > min(h, w) everything erodes and the boundary is the mask.  radius <= 0:
 * r = odise_hip_boundary_radius(h, w).  boundary: device uint8 [n][h][w] of 0 / 1.  area: device int64 [n] (optional), the pixels of each
 * boundary.  The masks are packed into 64-bit words, eroded there in O(log r) passes whatever the radius, and unpacked.  n == 0 writes
 * nothing and succeeds.  h * w <= 2^30, n <= 65535.  Scratch comes from the context.  Asynchronous on the context's stream.
 * The rule is restated from the paper and from _mask_to_boundary and pinned to the literal repeated erosion and to hand-worked pictures;
 * parity with the published boundary-iou package is unpinned (no test compares against it). */
int odise_hip_mask_boundary(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, int radius, uint8_t* boundary,
                            int64_t* area);
/* odise_hip_mask_iou with the Boundary IoU beside it: boundary_iou = rleIou on the exact pixel counts of the two boundaries
 * (odise_hip_mask_boundary of the dense masks and of the decoded ground truth, same radius; inter == 0 -> 0, crowd -> inter / the area of
 * the detection's boundary), mask_iou = what odise_hip_mask_iou writes, iou = fmin(mask_iou, boundary_iou), the IoU Boundary AP matches
 * on.  iou: device double [n][n_gt]; mask_iou, boundary_iou: the same shape, optional.  inter, area_d, area_g: optional, the counts of the
 * MASKS as in odise_hip_mask_iou.  Everything else - arguments, flag 1, the empty cases, limits - as odise_hip_mask_iou. */
int odise_hip_mask_boundary_iou(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, const uint32_t* gt_runs,
                                const int64_t* gt_offsets, int n_gt, const uint8_t* iscrowd, int radius, double* iou, double* mask_iou,
                                double* boundary_iou, int32_t* inter, int64_t* area_d, int64_t* area_g, int32_t* flags);
/* COCOeval.evaluateImg with the IoU of Boundary AP (LVIS' "boundary" iouType), beside "segm" and, with bb != NULL, "bbox", all from ONE
 * pack of the detections and ONE decode of the ground truth.  The walk is the one of odise_hip_instance_eval over
 * iou = fmin(mask IoU, boundary IoU) as odise_hip_mask_boundary_iou defines them; a boundary row's `area`, and with it the ignore rule of
 * an unmatched detection, is the segm task's (the pixels of the mask, not of its boundary), and the ignore bits of the ground truth are
 * d->gt_rows, as for the other tasks.  Detections past the count of the table are not read.
 * bd == NULL is odise_hip_instance_eval_bbox (bb set) or odise_hip_instance_eval_poly (bb NULL).  With bd set, d->rows and d->n_rows may
 * both be NULL: the segm rows are skipped then, but d->gt_runs / d->gt_offsets / p are still read, since the minimum needs the masks'
 * counts.  Flags 1, 2, 4 and 8 zero the boundary rows (n_rows = 0) exactly as they zero the segm rows.
 * ODISE_ERR_ARG and nothing written: a null bd->rows or bd->n_rows, and what odise_hip_instance_eval_bbox refuses (a null bb is no error
 * here).  Scratch comes from the context: the words of the topk + n_gt masks three times over (masks, boundaries, one temporary).
 * Asynchronous on the context's stream; no host synchronisation. */
typedef struct {
    int radius;                     /* <= 0: odise_hip_boundary_radius(d->h, d->w) */
    odise_inst_eval_row* rows;      /* device [topk] */
    int32_t* n_rows;                /* device [1] */
} odise_inst_boundary_task;
int odise_hip_instance_eval_boundary(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p, const odise_inst_bbox_task* bb,
                                     const odise_inst_boundary_task* bd);
/* COCOeval.accumulate for iouType "segm" on the rows of odise_hip_instance_eval as they lie on the device: maxDets (1, 10, 100), the four
 * area ranges, the ten IoU thresholds and the caller's table of recall thresholds; byte for byte what odise_amd/instance_eval.py
 * accumulate returns for the same rows.
 * The rows come in blocks: block b is rows[b] = odise_inst_eval_row [slots[b] * topk] and counts[b] = int32 [slots[b]]; slot s holds one
 * picture's rows in descending score, only its first counts[b][s] (clamped to 0..topk) exist.  Arrival order is block, slot, position.
 *   rank      the position of a row among the rows of its category in its slot, in slot order; maxDet m keeps the rows with rank < m.
 *   order     per category: score descending (every finite value and +-inf as -score orders them, -0 ties with +0), then `image`
 *             ascending, then arrival order.  That is the host's stable sort on `image` followed by argsort(-score, kind="mergesort")
 *             as long as no two slots share an image number (the host function merges such slots into one picture; this call does not).
 *   cells     per category k with npig[k][a] > 0, maxDet m, range a, threshold t, over the kept rows in that order: tp / fp = the inclusive
 *             counts of matched & ~ignored / ~matched & ~ignored at bit 10 a + t; rc = tp / npig[k][a], pr = tp / (fp + tp + 2^-52), IEEE
 *             double divisions; pr is replaced by its right-to-left running maximum; precision[t][r][k][a][m] = pr at the first row with
 *             rc >= rec_thrs[r], 0 without one; recall[t][k][a][m] = the last rc, 0 without rows.  Where npig[k][a] <= 0 every cell of
 *             (k, a) is -1.  Both outputs are written completely.  rec_thrs must ascend (COCO's np.linspace(0, 1, 101) does; pass that
 *             table, i / 100.0 is not the same numbers).
 * flags (OR-ed in): 1 = a row's category outside [0, num_categories), 2 = a NaN score.  A call that raises one fills both outputs with
 * -1; such rows are set aside before anything is indexed by them, no access leaves a buffer.
 * Limits (ODISE_ERR_ARG and nothing written otherwise): sum of slots[b] * topk <= 2^24, num_categories 1..65535, topk 1..100,
 * n_rec 1..101, no null pointer.  n_blocks = 0, slots[b] = 0 and counts of 0 are valid.
 * The sort is a stable LSD radix sort of the library's own (csrc/radix_sort.h); counts are integers and the maximum is exact, so the
 * bytes are the same from run to run.  Scratch comes from the context (56 bytes per row of capacity).  Asynchronous on the context's
 * stream; the host arrays are read before the call returns. */
typedef struct {
    int n_blocks;
    const odise_inst_eval_row* const* rows;   /* HOST [n_blocks] of device pointers */
    const int32_t* const* counts;             /* HOST [n_blocks] of device pointers */
    const int32_t* slots;                     /* HOST [n_blocks] */
    int topk;                                 /* rows per slot */
    int num_categories;                       /* K */
    const int64_t* npig;                      /* device [K][4]: non-ignored ground truths per (category, range) */
    const double* rec_thrs;                   /* device [n_rec], ascending */
    int n_rec;                                /* R */
    double* precision;                        /* device [10][R][K][4][3] */
    double* recall;                           /* device [10][K][4][3] */
    int32_t* flags;                           /* device [1] */
} odise_inst_accum_desc;
int odise_hip_instance_accumulate(odise_hip_ctx* ctx, const odise_inst_accum_desc* d);
/* LVIS AP for iouType "segm" (lvis-api LVISEval / LVISResults as detectron2's LVISEvaluator drives them): the walk of
 * odise_hip_instance_eval with LVIS' federated rules, at up to 300 detections of a picture over ALL categories.  Host restatement, which
 * is the specification: odise_amd/lvis_eval.py.  The rule is restated from lvis-api and pinned to hand-worked pictures
 * (tests/test_lvis_eval_cpu.py); parity with the lvis package is UNPINNED: it is no dependency of this project and no test runs the two
 * side by side.  "bbox" and "boundary" for LVIS are not part of this.
 *   cut          the caller's table holds the picture's detections cut at 300 by score (d->topk 1..300; lvis_eval.limit_dets).
 *   federation   pos = the categories with a ground truth in the picture (taken from d->gt_rows on the device); lv->neg_bits = those known
 *                to be absent, lv->not_exhaustive_bits = those annotated incompletely: device uint32 [ceil(K / 32)] each, bit k % 32 of
 *                word k / 32 = category k; bits at K and above are not looked at.  A detection whose category is in neither pos nor neg is
 *                DROPPED: it gives no row and is counted nowhere.
 *   walk         odise_hip_instance_eval's, with no crowd: LVIS has none, and iscrowd != 0 raises flag 4.  A ground truth with the
 *                annotation's `ignore` set comes as outside bits 0b1111: it is matched like any other, once, and hands its ignore bit on.
 *   unmatched    a detection without a match is ignored in range a when its area lies outside a OR its category is not exhaustive.
 * d->rows: the kept detections in descending score (ties in table order), row k = rank k among the KEPT; *d->n_rows = their count; rows
 * past it up to topk are zeroed.  Flags 1 / 2 / 4 / 8 as for odise_hip_instance_eval_poly; a picture that raises one writes n_rows = 0
 * and zeroed rows.  p: polygon ground truth, NULL = run lengths only.
 * With detections taken from the mask logits (d->masks NULL) the table holds (query, class) pairs, and every distinct query is sampled,
 * counted and intersected ONCE, however many classes it stands with; the rows are those of the same call on the dense masks of the pairs.
 * ODISE_ERR_ARG and nothing written: a null pointer (lv and both bitsets included), topk outside 1..300, n_gt outside 0..1024,
 * num_categories outside 1..65535, the geometry errors of odise_hip_instance_rle.  Scratch comes from the context.  Asynchronous on the
 * context's stream; no host synchronisation. */
typedef struct {
    const uint32_t* neg_bits;             /* device [ceil(K / 32)] */
    const uint32_t* not_exhaustive_bits;  /* device [ceil(K / 32)] */
} odise_lvis_task;
int odise_hip_lvis_eval(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p, const odise_lvis_task* lv);
/* LVISEval.accumulate on the rows of odise_hip_lvis_eval: odise_hip_instance_accumulate (blocks, slots, order, flags, limits, scratch) with
 * topk 1..300 and ONE cut, the 300 per picture that the rows already respect, so there is no maxDets axis: precision [10][R][K][4],
 * recall [10][K][4].  Byte for byte what odise_amd/lvis_eval.py accumulate returns for the same rows. */
typedef struct {
    int n_blocks;
    const odise_inst_eval_row* const* rows;   /* HOST [n_blocks] of device pointers */
    const int32_t* const* counts;             /* HOST [n_blocks] of device pointers */
    const int32_t* slots;                     /* HOST [n_blocks] */
    int topk;                                 /* rows per slot, 1..300 */
    int num_categories;                       /* K */
    const int64_t* npig;                      /* device [K][4] */
    const double* rec_thrs;                   /* device [n_rec], ascending */
    int n_rec;                                /* R */
    double* precision;                        /* device [10][R][K][4] */
    double* recall;                           /* device [10][K][4] */
    int32_t* flags;                           /* device [1] */
} odise_lvis_accum_desc;
int odise_hip_lvis_accumulate(odise_hip_ctx* ctx, const odise_lvis_accum_desc* d);
/* Video instance segmentation AP (YouTube-VIS: mask2former_video/data_video/ytvis_eval.py over datasets/ytvis_api/ytvoseval.py), which is
 * COCOeval with two changes: the IoU of a predicted track and a ground-truth track is taken over the whole sequence, and areas are
 * per-track means with ranges of their own.  Three calls: reset, one frame (any number of times), the end of a video.  Host restatement:
 * odise_amd/video_eval.py.  The rule is restated from ytvoseval.py and pinned to hand-worked videos (tests/test_video_eval_cpu.py); parity
 * with the reference evaluator is UNPINNED: pycocotools is no dependency of this project and no test runs the two side by side.
 *   sums      over the frames of a video, for predicted track s and ground-truth track s': inter[s][s'] = sum of |d & g|, area_d[s] and
 *             area_g[s'] = the sums of the pixel counts, frames_d[s] = the frames in which the track had a pixel.  A frame in which a
 *             track has no mask adds nothing for it.  All exact integers in 64 bits: the same bytes from run to run.
 *   iou       (computeIoU -> iou_seq) inter / (area_d + area_g - inter), one double division of exact integers; 0 when the denominator
 *             is 0.  iscrowd does NOT enter the IoU (the reference builds the list and never uses it).
 *   avg_area  of a predicted track (ytvos.py loadRes): area_d / frames_d, one double division; 0 without a frame.  Of a ground-truth
 *             track: the same mean over the annotation's own `areas`, which the HOST takes (they are the file's floats, not pixel counts).
 *   ranges    [0, 1e10], [0, 128^2], [128^2, 256^2], [256^2, 1e10], ends included.
 *   walk      evaluateVid is evaluateImg (odise_hip_instance_eval) with a track where a detection stands: maxDet 100, descending score
 *             with ties in table order, the crowd bit acting in the walk only, an unmatched track ignored when its avg_area lies outside
 *             the range.  Accumulate and summarize are COCOeval's: the rows go into odise_hip_instance_accumulate unchanged, topk =
 *             max_tracks, a video where a picture stands.
 * The accumulators belong to the caller, so the library keeps no state between the calls: */
typedef struct {
    int64_t* inter;      /* device [max_tracks][max_gt] */
    int64_t* area_d;     /* device [max_tracks]  sum of pixel counts */
    int64_t* area_g;     /* device [max_gt] */
    int32_t* frames_d;   /* device [max_tracks]  frames in which the track had a pixel */
    int max_tracks;      /* 1..100 */
    int max_gt;          /* 0..1024 */
} odise_video_eval_state;
/* Zeroes the four accumulators on the context's stream.  ODISE_ERR_ARG and nothing enqueued: a null pointer (inter and area_g may be
 * NULL with max_gt = 0), max_tracks outside 1..100, max_gt outside 0..1024, a buffer not aligned to its element. */
int odise_hip_video_eval_reset(odise_hip_ctx* ctx, const odise_video_eval_state* st);
/* One frame.  The detections are those of odise_inst_eval_desc (dense masks [topk,h,w], inst_table optional then: NULL = all topk; or
 * masks == NULL = the selection of image b of the last head forward, sampled from the mask logits); detections past the count of the
 * table are not read.  det_slot[i] is the track of table index i, gt_slot[j] the ground-truth track of annotation j; a value outside
 * [0, max_tracks) / [0, max_gt) belongs to no track and is skipped.  The ground truth is this frame's, as in odise_hip_instance_eval_poly:
 * runs, polygons (p, may be NULL) or both.  The call packs the detections, decodes or rasterises the ground truth into the same words and
 * adds to the sums above:
 *   inter[det_slot[i]][gt_slot[j]] += popcount(d_i & g_j)      area_d[s] += |d_i|      frames_d[s] += (|d_i| > 0)      area_g[s'] += |g_j|
 * The intersection is the tile loop of odise_hip_instance_eval (64 x 32 masks, 32 words, the word axis split over the grid) whose epilogue
 * adds its partial counts through the two slot tables with 64-bit integer atomics: no [topk][n_gt] matrix is written and read again.
 * flags (OR-ed): 1, 4 and 8 as in odise_hip_instance_eval_poly, read on the device: a frame that raises one adds nothing.  16 = two
 * detections below the count share a slot, or two annotations share a gt slot: both are still added (the sums are those of the two masks,
 * not of their union).
 * ODISE_ERR_ARG and nothing enqueued: a null required pointer (d, st and its buffers, flags, det_slot; gt_slot, gt_runs and gt_offsets
 * with n_gt > 0), topk outside 1..100, n_gt outside 0..1024, the limits of the state, h or w < 1, h * w > 2^30, a dtype other than
 * ODISE_F32 / ODISE_U8, the polygon errors of odise_hip_instance_eval_poly, the geometry errors of odise_hip_instance_rle.  Scratch comes
 * from the context.  Asynchronous on the context's stream: the host synchronises nowhere and reads no count. */
typedef struct {
    int h, w;
    const void* masks; int dtype;
    int b, pad_h, pad_w, img_h, img_w;
    const int32_t* inst_table;
    const float* inst_scores;       /* unused with dense masks, may be NULL then */
    int topk;                       /* 1..100 */
    const int32_t* det_slot;        /* device [topk] */
    const uint32_t* gt_runs; const int64_t* gt_offsets;   /* as odise_hip_mask_iou */
    const odise_inst_poly_gt* polys;                      /* HOST, or NULL: no polygon ground truth */
    int n_gt;                       /* 0..1024: the annotations of this frame */
    const int32_t* gt_slot;         /* device [n_gt] */
    const odise_video_eval_state* st;
    int32_t* flags;                 /* device [1] */
} odise_video_frame_desc;
int odise_hip_video_eval_frame(odise_hip_ctx* ctx, const odise_video_frame_desc* d);
/* The end of a video: evaluateVid on the sums.  Track s (s < n_tracks) has score track_scores[s] and contiguous category
 * track_category[s]; ground-truth track s' (s' < n_gt) is gt_rows[s'] = category, iscrowd, bits 0..3 = avg_area outside range a (the
 * host computes these from the annotation, as for odise_hip_instance_eval).  rows / n_rows: odise_inst_eval_row [max_tracks] in descending
 * score and their count, rows past it zeroed; a row's `area` is the track's avg_area truncated and clamped to int32, its `image` is
 * `video`, its bits are 10 a + t as everywhere.  iou (double [n_tracks][n_gt]) and avg_area (double [n_tracks]) are optional dumps.
 * flags (OR-ed): 2 = a track category outside [0, num_categories), 4 = a ground-truth category outside it / iscrowd not 0|1; a video
 * that raises one writes n_rows = 0 and zeroed rows.  The sums are left as they are: reset starts the next video.
 * ODISE_ERR_ARG and nothing enqueued: a null required pointer (d, st and its buffers, iou_thresholds, flags; track_scores and
 * track_category with n_tracks > 0; gt_rows with n_gt > 0), n_tracks outside 0..max_tracks, n_gt outside 0..max_gt, the limits of the
 * state, num_categories < 1, only one of rows / n_rows, neither rows nor a dump.  Asynchronous on the context's stream. */
typedef struct {
    const odise_video_eval_state* st;
    int n_tracks;                   /* 0..st->max_tracks */
    const float* track_scores;      /* device [n_tracks] */
    const int32_t* track_category;  /* device [n_tracks] */
    const int32_t* gt_rows;         /* device [n_gt][3] */
    int n_gt;                       /* 0..st->max_gt */
    int num_categories; int video;
    const double* iou_thresholds;   /* HOST [10] */
    odise_inst_eval_row* rows;      /* device [max_tracks] */
    int32_t* n_rows;                /* device [1] */
    int32_t* flags;                 /* device [1] */
    double* iou;                    /* device [n_tracks][n_gt], optional */
    double* avg_area;               /* device [n_tracks], optional */
} odise_video_finish_desc;
int odise_hip_video_eval_finish(odise_hip_ctx* ctx, const odise_video_finish_desc* d);

/* ---- drawing a panoptic result (demo/demo.py:173-199 VisualizationDemo.run_on_image -> detectron2 Visualizer.draw_panoptic_seg) ----
 * The per-pixel work of that call on the panoptic record as it lies in HBM: the pieces of a segment, where its label goes, and the
 * coloured picture.  Glyphs and file encoding stay on the host (odise_amd/visualize.py, which also restates the rules below in numpy). */
/* Connected components of a label map, 8-connectivity.  labels int32 [H,W] (device) -> roots int32 [H,W] (device, must not overlap
 * labels): roots[p] = the smallest row-major pixel index among the pixels joined to p by 8-neighbour steps over EQUAL labels;
 * roots[p] = -1 where labels[p] <= 0 (VOID).  A function of the input alone: the same bytes from run to run.  Tiles of 32 x 32 are
 * labelled in LDS, their borders joined by integer atomic minima in `roots` itself, and a last pass points every pixel at its root; no
 * scratch.  ODISE_ERR_ARG and nothing written: a null pointer, H or W < 1, H * W > 2^29 - 1.  Asynchronous on the context's stream. */
int odise_hip_connected_components(odise_hip_ctx* ctx, const int32_t* labels, int H, int W, int32_t* roots);
/* Where detectron2 puts the labels of a panoptic result (Visualizer.draw_panoptic_seg -> draw_binary_mask / _draw_text_in_mask).
 * pred_ids / pred_segments are the two parts of the panoptic record, as in odise_pq_desc; in the table the first row of an id counts,
 * isthing != 0 is a thing, and ids <= 0 of the map are VOID.  Rows of 32 bytes {segment_row, area, x2, y2, x0, y0, x1, y1}: x2 / y2 are
 * TWICE the median column / row of the pixels the row stands for (np.median(mask.nonzero(), axis=1): the .5 of an even count is exact),
 * x0..y1 their inclusive bounding box, area their number.
 *   thing row whose id has a pixel   one anchor over ALL pixels of the segment, in however many pieces it lies.
 *   stuff row                        nothing if its largest 8-connected component has fewer than small_area pixels; otherwise one anchor
 *                                    for the largest component (equal areas: the one with the smaller root, i.e. met first in row-major
 *                                    order) and one for every other component with MORE than large_area pixels.
 *   a table row without a pixel, a map id without a row: nothing.
 * Anchors are written in ascending (segment_row, root) order; n_anchors is the total found, at most `cap` rows are written and nothing
 * is written past them.  detectron2's constants are small_area = 1000, large_area = 120000.  Medians come from per-anchor column and
 * row histograms and a scan (nothing is sorted); all counting is integer atomics, so the output is the same from run to run.  The
 * order is found by comparing the anchors of a call with each other: they are few (at most n + H * W / (large_area + 1)).
 * ODISE_ERR_ARG and nothing written: a null pointer, H or W < 1, H * W > 2^29 - 1, cap < 0.  Scratch comes from the context.
 * Asynchronous on the context's stream. */
typedef struct { int32_t segment_row, area, x2, y2, x0, y0, x1, y1; } odise_anchor_row;   /* 32 bytes */
typedef struct {
    int H, W;
    const int32_t* pred_ids;      /* device [H*W] */
    const int32_t* pred_segments; /* device: n | n rows (id, isthing, category_id); n is read on the device, n <= ODISE_MAX_SEGMENTS */
    int small_area, large_area;
    odise_anchor_row* anchors;    /* device [cap] */
    int cap;
    int32_t* n_anchors;           /* device [1] */
} odise_anchor_desc;
int odise_hip_segment_anchors(odise_hip_ctx* ctx, const odise_anchor_desc* d);
/* The coloured picture.  image / out uint8 [H,W,3] (device; out == image is allowed, any other overlap is not), colors uint8 [n][3]
 * (device), one per table row.  Per pixel, in this order of precedence:
 *   its id is <= 0 or has no row                                          out = image
 *   a 4-neighbour INSIDE the picture has a different id                    out = edge_rgb
 *   otherwise, per channel                                                out = (image * (256 - alpha256) + color * alpha256 + 128) >> 8
 * Integer arithmetic, one pass; buffers of any byte alignment (four pixels per lane as three dwords where image and out are 4-byte
 * aligned, pixel by pixel otherwise).  ODISE_ERR_ARG and nothing written: a null pointer, H or W < 1, H * W > 2^29 - 1, alpha256
 * outside 0..256.  Asynchronous on the context's stream. */
typedef struct {
    int H, W;
    const uint8_t* image;
    const int32_t* pred_ids;      /* as odise_anchor_desc */
    const int32_t* pred_segments;
    const uint8_t* colors;
    int alpha256;                 /* 0 (the picture) .. 256 (the colour) */
    uint8_t edge_rgb[3];
    uint8_t* out;
} odise_overlay_desc;
int odise_hip_panoptic_overlay(odise_hip_ctx* ctx, const odise_overlay_desc* d);
/* ---- drawing instance and semantic results (the else branch of run_on_image: draw_sem_seg, then draw_instance_predictions) ----
 * Instance masks overlap, so they are drawn from the bit-packed words the segm evaluators use (exactly the pixels of
 * odise_hip_instance_rle), not from a label map.  The descriptor follows odise_inst_eval_desc: the detections are the selection of image
 * b of the last head forward (inst_table / inst_scores / pad / img as there; masks sampled from the mask logits, n read on the device),
 * or dense `masks` [topk,h,w], for which inst_table (NULL: n = topk) and inst_scores (NULL: no score test) are optional.
 *   kept       instance i < n is kept iff inst_scores[i] >= min_score and its mask has a pixel.
 *   anchors    (optional) [topk] rows, one per table index: segment_row = i, area, x2 / y2 = TWICE np.median of the mask's columns / rows
 *              (detectron2 centres the label there when the instance has no box; the reference's pred_boxes are zeros), x0..y1 the
 *              bounding box.  A row that is not kept (or i >= n) is {-1, 0, 0, 0, 0, 0, 0, 0}.
 *   order      (optional) int32 [topk]: the position of instance i in the draw order, -1 when it is not kept.  detectron2 draws the
 *              largest area first; here: descending area, ties by ascending table index.
 *   out        (optional) the picture.  Per pixel, starting from c = image and walking the kept instances in draw order, for each
 *              instance i whose mask holds the pixel: c = edge_colors[i] if a 4-neighbour INSIDE the picture is outside mask i, else per
 *              channel c = (c * (256 - alpha256) + colors[i] * alpha256 + 128) >> 8.  Pixels in no kept mask keep the image; n = 0
 *              copies it.  colors / edge_colors uint8 [topk][3] (device), by table index.  out == image is allowed, any other overlap
 *              is not; buffers of any byte alignment (four pixels of a row as three dwords where they are 4-byte aligned in both).
 * Column and row histograms come from popcounts and bit tests of the packed words, the order from counting, the picture from tiles of
 * 64 x 64 pixels whose mask and edge bits are transposed through LDS: integer work without atomics, the same bytes from run to run.
 * ODISE_ERR_ARG and nothing written: a null required pointer (out needs image, colors and edge_colors; without masks inst_table and
 * inst_scores; at least one output), h or w < 1, h * w > 2^29 - 1, topk outside 1..100, alpha256 outside 0..256, an out that overlaps
 * image without being equal to it, the geometry errors of odise_hip_instance_rle.  Scratch comes from the context.  Asynchronous on
 * the context's stream. */
typedef struct {
    int h, w;                       /* size of the picture = output size of the masks */
    const void* masks; int dtype;   /* dense [topk,h,w] (ODISE_F32 / ODISE_U8), or NULL = from the mask logits of image b of the last head forward: */
    int b, pad_h, pad_w, img_h, img_w;   /* as odise_hip_instance_rle */
    const int32_t* inst_table;      /* device [1 + 2*topk]: n | query index | class  (n read on the device) */
    const float* inst_scores;       /* device [topk] */
    int topk;                       /* 1..100 */
    float min_score;
    const uint8_t* image;           /* device [h,w,3] */
    const uint8_t* colors;          /* device [topk][3] */
    const uint8_t* edge_colors;     /* device [topk][3] */
    int alpha256;                   /* 0 (the picture) .. 256 (the colour) */
    uint8_t* out;                   /* device [h,w,3], optional */
    odise_anchor_row* anchors;      /* device [topk], optional */
    int32_t* order;                 /* device [topk], optional */
} odise_inst_draw_desc;
int odise_hip_instance_draw(odise_hip_ctx* ctx, const odise_inst_draw_desc* d);
/* odise_hip_instance_draw for instances that carry boxes: detectron2 Visualizer.overlay_instances(boxes=..., masks=...), which draws a
 * rectangle frame per box, orders the instances by BOX area and puts the label on the box corner.  d is read as above; bx adds the boxes
 * (as odise_hip_instance_boxes writes them, or any other).  What differs:
 *   kept       additionally the box is finite and has a positive width and height (x1 > x0 and y1 > y0).
 *   order      descending box area, the float product (x1 - x0) * (y1 - y0); ties by ascending table index.
 *   anchors    x0..y1 = the box, the floats truncated toward zero (clamped to +-2^29); the label position (x2 / 2, y2 / 2) is (x0, y0);
 *              when the box area (that float product) < small_area or y1 - y0 < 40 (floats) it is (x1, y0) if y1 >= h - 5, else
 *              (x0, y1).  `area` stays the mask's pixel count.  detectron2's small_area is _SMALL_OBJECT_AREA_THRESH = 1000.
 *   out        walking the kept instances in the new order, instance i first lays its frame: with bx0 = max(x0, 0), by0 = max(y0, 0),
 *              bx1 = min(x1, w), by1 = min(y1, h) of the truncated members (the box clipped to the picture), a pixel with
 *              bx0 <= x < bx1, by0 <= y < by1 and x < bx0 + box_width or x >= bx1 - box_width or y < by0 + box_width or
 *              y >= by1 - box_width takes c = (c * (256 - box_alpha256) + colors[i] * box_alpha256 + 128) >> 8 per channel; then the
 *              mask step of odise_hip_instance_draw, unchanged.  A box narrower than 2 * box_width is all frame.
 * The same tiles as odise_hip_instance_draw; the bounds of the boxes lie in LDS and a tile that no kept mask touches still gets its frames.
 * With box_alpha256 = 0 and a box order equal to the mask order the picture is odise_hip_instance_draw's.
 * ODISE_ERR_ARG and nothing written: what odise_hip_instance_draw refuses, a null bx or bx->boxes, boxes not 4-byte aligned,
 * box_width < 1, box_alpha256 outside 0..256.  Scratch comes from the context.  Asynchronous on the context's stream. */
typedef struct {
    const float* boxes;             /* device [topk][4] XYXY */
    int box_width;                  /* >= 1, pixels */
    int box_alpha256;               /* 0 (no frame) .. 256 (the colour) */
    int small_area;                 /* the label of a box below this area moves off the corner */
} odise_inst_box_draw;
int odise_hip_instance_draw_boxes(odise_hip_ctx* ctx, const odise_inst_draw_desc* d, const odise_inst_box_draw* bx);
/* A semantic result as a panoptic record that odise_hip_segment_anchors and odise_hip_panoptic_overlay draw unchanged (draw_sem_seg).
 * Input: labels int32 [H,W] (the fused arg-max map) or sem_seg fp32 [K,H,W] (arg-max over the planes, ties to the lower class, as
 * odise_hip_semantic_confusion takes it); exactly one of the two.  record int32 [H*W | 1 | 3*ODISE_MAX_SEGMENTS] (device, must not
 * overlap the input): ids, n, n rows (id, 0, category) with id = category + 1, the rest of the table zero.  Rows in descending pixel
 * count, ties by the smaller category (the order draw_sem_seg draws in); of more than ODISE_MAX_SEGMENTS present classes the first
 * ODISE_MAX_SEGMENTS are kept.  A label outside [0, K) and a class without a row get id 0.  Every row is stuff, so
 * odise_hip_segment_anchors applies draw_sem_seg's rule: a label at the largest component and at every component above large_area, none
 * if the largest is below small_area.  Counting is a per-block LDS histogram added with integer atomics, the order is found by counting.
 * ODISE_ERR_ARG and nothing written: a null pointer or both inputs, H or W < 1, H * W > 2^29 - 1, K outside 1..12288.  Scratch comes
 * from the context.  Asynchronous on the context's stream. */
int odise_hip_semantic_record(odise_hip_ctx* ctx, const int32_t* labels, const float* sem_seg, int K, int H, int W, int32_t* record);
/* ---- a thing keeps its colour from frame to frame (demo/demo.py:201-243 run_on_video -> detectron2 VideoVisualizer._assign_colors) ----
 * The mask-IoU path of that rule on panoptic records as they lie in HBM (host restatement: odise_amd/video.py ColorTracker).
 *   instances   of a frame: the table rows with isthing != 0 that are the first row of their id, have an id > 0 and own a pixel of
 *               pred_ids, in table-row order; (label = category, mask, area, ttl = the tracker's ttl).
 *   live list   ordered, empty at the start; after a frame: that frame's instances in their order, then the surviving old ones in theirs.
 *   iou         of live row o and new instance j: inter / (area_o + area_j - inter) as the double division of the two integers, 0 where
 *               the categories differ.
 *   matching    every live row takes j = the FIRST maximum of its iou row.  If that iou > 0.5 (strict) and o is the smallest list position
 *               among the rows that chose j this way, j takes o's colour and o leaves the list; every other live row loses one ttl and
 *               stays iff ttl > 0 (also a row whose j went to an earlier row, whatever its second-best is).
 *   colours     new instances without a colour take pool[counter % n_pool], counter += 1, in instance order; the counter lives on.
 * colors is in/out: only the rows of this frame's instances are written.  The tracker keeps what it needs (a byte map per retained frame:
 * 0 = no instance, 1 + table row; a live row can only come from the last ttl <= 8 frames), so the record may be reused as soon as the call
 * has returned; all of its memory (8 byte maps, a pair-count matrix of 8 x 101 x 101 int32, 800 live rows) is allocated by
 * odise_hip_track_create and released by odise_hip_track_destroy.  Two launches per frame, no synchronisation: one sweep over the pixels
 * counts (old index, new index) pairs of every retained frame that still has a live row in the per-block LDS histogram (in the matrix
 * directly when the frames' tables together need more than 12288 cells) and writes the new byte map in place of the oldest; one block
 * matches, colours and compacts the list.  Integer atomics only: the same bytes from run to run.
 * ODISE_ERR_ARG and nothing written: a null required pointer, H or W < 1, H * W > 2^29 - 1, ttl outside 1..8, n_pool < 1, a negative cap,
 * live without n_live, a descriptor whose H / W are not the tracker's.  Asynchronous on the context's stream. */
typedef struct odise_track odise_track;
int odise_hip_track_create(odise_hip_ctx* ctx, int H, int W, int ttl, const uint8_t* pool_rgb /* HOST [n_pool][3] */, int n_pool, odise_track** out);
int odise_hip_track_reset(odise_hip_ctx* ctx, odise_track* track);     /* empties the live list and the counter */
int odise_hip_track_destroy(odise_hip_ctx* ctx, odise_track* track);   /* waits for the stream */
typedef struct { int32_t frame, id, category, area, ttl, rgb /* r | g << 8 | b << 16 */, pad0, pad1; } odise_track_row;   /* 32 bytes; pads are 0 */
typedef struct {
    odise_track* track;
    int H, W;                     /* must be the tracker's */
    const int32_t* pred_ids;      /* device [H*W], as odise_overlay_desc (read 16 bytes at a time when so aligned, pixel by pixel otherwise) */
    const int32_t* pred_segments; /* device: n | n rows (id, isthing, category_id); n is read on the device, n <= ODISE_MAX_SEGMENTS */
    uint8_t* colors;              /* device [ODISE_MAX_SEGMENTS][3], in/out */
    odise_track_row* live;        /* optional, device [live_cap]: the live list AFTER the frame, in list order; nothing past live_cap rows */
    int live_cap;
    int32_t* n_live;              /* device [1], required with live: the length of the list (not clipped to live_cap) */
    double* iou;                  /* optional, device [iou_cap][ODISE_MAX_SEGMENTS]: iou[o * ODISE_MAX_SEGMENTS + j] of live row o of the
                                     list BEFORE the frame and this frame's instance j; other cells are left alone */
    int iou_cap;
} odise_track_desc;
int odise_hip_track_frame(odise_hip_ctx* ctx, const odise_track_desc* d);
/* ---- overlapping instance masks keep their colours from frame to frame (run_on_video's instance branch) ----------------------------
 * For a box-less _DetectedInstance detectron2's _assign_colors matches on mask IoU; that path is what is built here (host restatement:
 * odise_amd/video.py InstanceColorTracker).  It is NOT what the reference's run_on_video produces on this model: there the instances
 * carry pred_boxes of all zeros, box IoU is 0 / 0 and every instance takes a fresh colour in every frame.
 * Instance masks overlap, so a frame is no label map: the tracker retains the bit-packed words of rle_pack.h (exactly the pixels of
 * odise_hip_instance_rle / odise_hip_instance_draw) and the IoU of two masks is the popcount of an AND.
 *   instances   of a frame: the table indices i < n with inst_scores[i] >= min_score whose mask has a pixel (the `kept` rule of
 *               odise_hip_instance_draw), in ascending table index; (label = class, mask, area, ttl = the tracker's ttl).
 *   live list   ordered, empty at the start; after a frame: that frame's instances in their order, then the surviving old ones in theirs.
 *   iou         of live row o and new instance j: inter / (area_o + area_j - inter) as the double division of the two integers, 0 where
 *               the classes differ.
 *   matching    every live row takes j = the FIRST maximum of its iou row.  If that iou > 0.5 (strict) and o is the smallest list position
 *               among the rows that chose j this way, j takes o's colour and o leaves the list; every other live row loses one ttl and
 *               stays iff ttl > 0 (also a row whose j went to an earlier row, whatever its second-best is).
 *   colours     new instances without a colour take pool[counter % n_pool], counter += 1, in instance order; the counter lives on.
 * ttl 1..8, topk 1..100, at most 800 live rows.  The detections are those of odise_inst_draw_desc: dense `masks` [topk,h,w] (inst_table
 * NULL: n = topk and every class is 0; inst_scores NULL: no score test), or masks == NULL = the selection of image b of the last head
 * forward, sampled from the mask logits (inst_table and inst_scores required).
 * colors is in/out and indexed by table index: only the rows of this frame's instances are written; edge_colors (optional) gets, in the
 * same rows, the outline colour odise_hip_instance_draw is given for them (3/10 of a colour whose channels sum to >= 384, else the
 * colour moved 7/10 of the way to white, per channel in integers).  live rows carry id = table index.
 * Memory: a row made in frame f with ttl T is still matched against in frame f + T, so the tracker owns a ring of ttl + 1 slots of
 * topk * h-word-rows * w words of 8 bytes ((ttl + 1) * topk * w * ceil(h / 64) * 8 bytes; at 1024 x 1024 and topk 100 a slot is 13.1 MB,
 * nine of them 118 MB), an 800 x topk int32 intersection matrix that is zero between calls and the 800 live rows; all of it is allocated
 * by odise_hip_inst_track_create and released by odise_hip_inst_track_destroy, so the masks may be reused as soon as the call has returned.
 * Per frame, on the context's stream, without a synchronisation or a count read by the host: the pack launch of rle_pack.h into the ring
 * slot frame mod (ttl + 1) (the frame number is counted on the host, so a call cannot be replayed from a captured graph); areas and the
 * kept test; the gathered intersection - tiles of 64 live rows x 32 new masks x 32 words in LDS, a live row's words found through its
 * (frame, id) in the device-resident list, the grid sized for 800 x topk with the word axis split over blockIdx.z, a tile past either
 * count or without a (live, new) pair of one class leaving before it loads a word; one block that matches, colours and compacts the
 * list.  Integer atomics only: the same bytes from run to run.
 * ODISE_ERR_ARG and nothing written: a null required pointer, h or w < 1, h * w > 2^29 - 1, topk outside 1..100, ttl outside 1..8,
 * n_pool outside 1..2^20, a descriptor whose h, w or topk are not the tracker's, a dtype other than ODISE_F32 / ODISE_U8, a negative
 * cap, live without n_live, the geometry errors of odise_hip_instance_rle.  ODISE_ERR_NOMEM: the ring could not be allocated. */
typedef struct odise_inst_track odise_inst_track;
int odise_hip_inst_track_create(odise_hip_ctx* ctx, int H, int W, int topk, int ttl, const uint8_t* pool_rgb /* HOST [n_pool][3] */, int n_pool,
                                odise_inst_track** out);
int odise_hip_inst_track_reset(odise_hip_ctx* ctx, odise_inst_track* track);     /* empties the live list, the counter and the frame number */
int odise_hip_inst_track_destroy(odise_hip_ctx* ctx, odise_inst_track* track);   /* waits for the stream */
typedef struct {
    odise_inst_track* track;
    int h, w;                       /* must be the tracker's */
    const void* masks; int dtype;   /* dense [topk,h,w] (ODISE_F32 / ODISE_U8), or NULL = from the mask logits of image b of the last head forward: */
    int b, pad_h, pad_w, img_h, img_w;   /* as odise_hip_instance_rle */
    const int32_t* inst_table;      /* device [1 + 2*topk]: n | query index | class  (n read on the device) */
    const float* inst_scores;       /* device [topk] */
    int topk;                       /* must be the tracker's */
    float min_score;
    uint8_t* colors;                /* device [topk][3], in/out */
    uint8_t* edge_colors;           /* optional, device [topk][3], in/out */
    odise_track_row* live;          /* optional, device [live_cap]: the live list AFTER the frame, in list order; nothing past live_cap rows */
    int live_cap;
    int32_t* n_live;                /* device [1], required with live: the length of the list (not clipped to live_cap) */
    double* iou;                    /* optional, device [iou_cap][100]: iou[o * 100 + j] of live row o of the list BEFORE the frame and this
                                       frame's instance j (its position among the instances); other cells are left alone */
    int iou_cap;
} odise_inst_track_desc;
int odise_hip_inst_track_frame(odise_hip_ctx* ctx, const odise_inst_track_desc* d);
/* ---- instances that carry boxes keep their colours from frame to frame (the FIRST path of _assign_colors) ----------------------------
 * For a _DetectedInstance with a box detectron2's _assign_colors matches on box IoU at 0.6; mask IoU at 0.5 (above) is only its path for
 * box-less instances.  Host restatement: odise_amd/video.py BoxColorTracker.  A box tracker needs neither pixels nor a ring: its state is
 * the 800 live rows and one float [4] per row.
 *   instances   of a frame: the table indices i < n with inst_scores[i] >= min_score whose box is finite and has x1 > x0 && y1 > y0 (for
 *               the tight boxes of odise_hip_instance_boxes the `kept` rule of odise_hip_instance_draw), in ascending table index;
 *               (label = class, box, ttl = the tracker's ttl).  A row with a non-finite box member is no instance.
 *   live list   ordered, empty at the start; after a frame: that frame's instances in their order, then the surviving old ones in theirs.
 *   iou         of live row o and new instance j: the arithmetic of odise_hip_box_iou (maskApi.c bbIou in doubles, every operation rounded
 *               on its own, crowd = 0) on the two boxes as XYWH = (x0, y0, x1 - x0, y1 - y0) computed in double from the floats; 0 where
 *               the classes differ.
 *   matching    every live row takes j = the FIRST maximum of its iou row.  If that iou > 0.6 (strict) and o is the smallest list position
 *               among the rows that chose j this way, j takes o's colour and o leaves the list; every other live row loses one ttl and
 *               stays iff ttl > 0 (also a row whose j went to an earlier row, whatever its second-best is).
 *   colours     new instances without a colour take pool[counter % n_pool], counter += 1, in instance order; the counter lives on.
 * Deviation, asked for by its own flag (demo --track-boxes) as the mask tracker is: as far as detectron2's source can be read without
 * the package at hand, _assign_colors hands its XYXY rows to pycocotools' iou, which reads them as XYWH; here the IoU is the geometric
 * one of the boxes.
 * ttl 1..8, topk 1..100, at most 800 live rows.  boxes: device float [topk][4] XYXY as odise_hip_instance_boxes writes them.  inst_table
 * NULL: n = topk and every class is 0; inst_scores NULL: no score test.  colors / edge_colors / live / n_live / iou as in
 * odise_inst_track_desc; a live row carries id = table index, area = (int32) of its box's w * h (the double product, at most 2^31 - 1)
 * and frame = frames since the reset.
 * One launch of one block per frame, no pixel memory, no synchronisation.  The frame number lives on the device with the list, so -
 * unlike odise_hip_inst_track_frame - the call can be replayed from a captured graph.  The same bytes from run to run.
 * ODISE_ERR_ARG and nothing written: a null required pointer (track, boxes, colors), topk outside 1..100, ttl outside 1..8, n_pool
 * outside 1..2^20, a descriptor whose topk is not the tracker's, a negative cap, live without n_live, a misaligned buffer.
 * ODISE_ERR_NOMEM: the state could not be allocated. */
typedef struct odise_box_track odise_box_track;
int odise_hip_box_track_create(odise_hip_ctx* ctx, int topk, int ttl, const uint8_t* pool_rgb /* HOST [n_pool][3] */, int n_pool, odise_box_track** out);
int odise_hip_box_track_reset(odise_hip_ctx* ctx, odise_box_track* track);     /* empties the live list, the counter and the frame number */
int odise_hip_box_track_destroy(odise_hip_ctx* ctx, odise_box_track* track);   /* waits for the stream */
typedef struct {
    odise_box_track* track;
    const float* boxes;             /* device [topk][4] XYXY */
    const int32_t* inst_table;      /* device [1 + 2*topk]: n | query index | class  (n read on the device), optional */
    const float* inst_scores;       /* device [topk], optional */
    int topk;                       /* must be the tracker's */
    float min_score;
    uint8_t* colors;                /* device [topk][3], in/out */
    uint8_t* edge_colors;           /* optional, device [topk][3], in/out */
    odise_track_row* live;          /* optional, device [live_cap]: the live list AFTER the frame, in list order; nothing past live_cap rows */
    int live_cap;
    int32_t* n_live;                /* device [1], required with live: the length of the list (not clipped to live_cap) */
    double* iou;                    /* optional, device [iou_cap][100]: iou[o * 100 + j] of live row o of the list BEFORE the frame and this
                                       frame's instance j (its position among the instances); other cells are left alone */
    int iou_cap;
} odise_box_track_desc;
int odise_hip_box_track_frame(odise_hip_ctx* ctx, const odise_box_track_desc* d);

/* ---- test-time augmentation of the semantic head (Mask2Former SemanticSegmentorWithTTA: several short-edge sizes, each also mirrored,
 * sem_seg averaged at the original size) ------------------------------------------------------------------------------------------
 * sem_seg = P^T sigmoid(masks) is linear in the (query, pixel) probabilities, so the mean over A views is one product over the views' query
 * sets laid end to end, and its arg-max never needs [K, h, w].  The handle owns S_cat f16 [out_h*out_w, max_views*Qpad] and PT_cat f16
 * [K, max_views*Qpad] (Qpad = Q rounded up to 8); they outlive the odise_hip_infer calls of the views.
 *   create    ODISE_ERR_ARG: a null pointer, out_h*out_w >= 2^30, K outside 1..65536, Q outside 1..304, max_views outside 1..64, or buffers
 *             larger than the free device memory; ODISE_ERR_NOMEM if the allocation fails all the same.
 *   add_view  image b of the context's current mask logits (odise_hip_head_forward / odise_hip_infer / odise_hip_set_head_masks) and that
 *             image's mask_cls_b (device fp32 [Q, K+1] log-probabilities) become the next view: its S bits are what the post-processing
 *             pixel pass writes for (pad, img, out = the handle's size), sampled at column out_w-1-x when hflip; its PT bits those of
 *             odise_hip_postprocess_batch.  One launch, asynchronous.  ODISE_ERR_ARG and the handle unchanged: a view beyond max_views, a
 *             vocabulary size or query count that is not the handle's, b out of range, img larger than pad, pad other than 4 x the logit grid.
 *   finish    sem_seg (optional, device fp32 [K, out_h, out_w]) = the sum over the views divided by their number in fp32; sem_argmax
 *             (optional, device int32 [out_h*out_w]) = first maximum of the sums.  With one unmirrored view sem_argmax is bit-identical to
 *             odise_post_desc's.  ODISE_ERR_ARG: no view added, or neither output.  The views stay; reset starts the next picture.
 *   destroy   waits for the stream. */
typedef struct odise_tta odise_tta;
int odise_hip_tta_create(odise_hip_ctx* ctx, int out_h, int out_w, int K, int Q, int max_views, odise_tta** out);
int odise_hip_tta_reset(odise_hip_ctx* ctx, odise_tta* tta);
int odise_hip_tta_destroy(odise_hip_ctx* ctx, odise_tta* tta);
int odise_hip_tta_add_view(odise_hip_ctx* ctx, odise_tta* tta, int b, const float* mask_cls_b, int pad_h, int pad_w, int img_h, int img_w, int hflip);
int odise_hip_tta_finish(odise_hip_ctx* ctx, odise_tta* tta, float* sem_seg, int32_t* sem_argmax);
/* dst uint8 [H,W,C] = src mirrored left to right (HFlipTransform on the resized picture); src != dst, H*W*C < 2^31.  Asynchronous. */
int odise_hip_hflip_u8_hwc(odise_hip_ctx* ctx, const void* src, void* dst, int H, int W, int C);

/* ---- JPEG input -------------------------------------------------------------------------------------------
 * Replaces detectron2 `read_image(file, "RGB")` = PIL.Image.open -> EXIF transpose -> convert("RGB") of the DatasetMapper
 * (configs/common/data/pano_open_d2_eval.py:74-107; demo/demo.py:399) for baseline JPEG files, bit-identical to Pillow /
 * libjpeg-turbo defaults (islow IDCT, fancy upsampling).  Huffman decoding runs on the host, everything per-sample on the device.
 * 8-bit Huffman files: baseline / extended sequential (SOF0 / SOF1) and progressive (SOF2), grey or YCbCr with luma sampling
 * 1x1 / 2x1 / 2x2; anything else (arithmetic coding, lossless, CMYK, RGB-coded): ODISE_ERR_UNSUPPORTED. */
typedef struct odise_jpeg_info {
    int32_t width, height;        /* coded size (before the EXIF orientation is applied) */
    int32_t components;           /* 1 (grey) or 3 (YCbCr) */
    int32_t h_samp, v_samp;       /* luma sampling factors */
    int32_t orientation;          /* EXIF tag 0x0112, 1..8 (1 when absent) */
    int32_t restart_interval;     /* MCUs, 0 = none */
    int32_t blocks_x[3], blocks_y[3]; /* 8x8-block grid of every component (padded to whole MCUs) */
    int64_t coef_count;           /* int16 coefficients of all components */
} odise_jpeg_info;
/* host only: parse the headers of a JPEG byte stream */
int odise_hip_jpeg_info(const void* data, int64_t len, odise_jpeg_info* info);
/* host only: entropy-decode into coefs int16 [coef_count] (component after component, [blocks_y][blocks_x][64], natural order,
 * not dequantised); qtables (optional) uint16 [components*64] receives every component's quantisation table in natural order */
int odise_hip_jpeg_entropy_decode(const void* data, int64_t len, int16_t* coefs, int64_t capacity, uint16_t* qtables);
/* data: host bytes of the file.  dst_rgb: device uint8 [out_h,out_w,3] (capacity in bytes); the decoded size is returned in
 * out_h / out_w (height and width swap for EXIF orientations 5..8 when apply_orientation != 0).  Asynchronous on the context's stream. */
int odise_hip_jpeg_decode(odise_hip_ctx* ctx, const void* data, int64_t len, void* dst_rgb, int64_t dst_capacity, int apply_orientation,
                          int* out_h, int* out_w);
/* the device half on its own: coefficients and tables as produced by odise_hip_jpeg_entropy_decode (which is thread-safe and can run
 * in loader threads while this context is busy with the previous image) */
int odise_hip_jpeg_decode_coefs(odise_hip_ctx* ctx, const odise_jpeg_info* info, const int16_t* coefs, const uint16_t* qtables, void* dst_rgb,
                                int64_t dst_capacity, int apply_orientation, int* out_h, int* out_w);

/* ---- multi-GPU exchange step ---------------------------------------------------------------------------------------
 * One process per GPU; images are independent units sharded across ranks, there is no collective inside the model forward, and
 * exactly one exchange: an RCCL all-gather (xGMI) of fixed-size int32 prediction records, replacing detectron2's pickled
 * `comm.gather` of per-image predictions reached from odise/evaluation/evaluator.py:144 (inference_on_dataset -> evaluator.evaluate)
 * and, for semantic evaluation, the gather behind SemSegEvaluator.evaluate (odise/evaluation/d2_evaluator.py:63) -> one all-reduce of
 * the (K+1)^2 int64 confusion counters.  The communicator belongs to the context; collectives run on a second HIP stream ordered after
 * the work queued on the compute stream so far, so the next batch's kernels overlap the exchange.  A world of one rank is valid. */
#define ODISE_COMM_ID_BYTES 128
/* rank 0: fill id128 (ODISE_COMM_ID_BYTES host bytes) - the launcher broadcasts it to the other ranks over its CPU rendezvous */
int odise_hip_comm_unique_id(void* id128);
int odise_hip_comm_init(odise_hip_ctx* ctx, const void* id128, int rank, int world);
int odise_hip_comm_destroy(odise_hip_ctx* ctx);
int odise_hip_comm_info(odise_hip_ctx* ctx, int* rank, int* world);   /* world = 0 when no communicator exists */
/* all [world * count] = concatenation over ranks of local [count] (device int32; count identical on every rank).  Record layout per
 * image (odise_amd/distributed.py): panoptic_seg [H*W] | n_segments | segments [100][3] = (id, isthing, category_id).  Asynchronous. */
int odise_hip_allgather_predictions(odise_hip_ctx* ctx, const int32_t* local, int64_t count, int32_t* all);
/* The same exchange for UNEVEN shards: this rank contributes n_records (0 .. max_records) records of record_len int32 each; max_records is
 * identical on every rank (the largest shard: ceil(images / world) per batch, known to every rank without communication).  all
 * [world * max_records * record_len]: rank r's records at row r * max_records, its missing rows filled with -1 (a valid record never starts
 * with -1: its first element is a panoptic id >= 0).  local may alias this rank's slice of `all`.  Asynchronous. */
int odise_hip_allgather_records(odise_hip_ctx* ctx, const int32_t* local, int n_records, int max_records, int64_t record_len, int32_t* all);
/* data [count] int64 device, summed in place over ranks (confusion matrices of odise_hip_semantic_confusion).  Asynchronous. */
int odise_hip_allreduce_sum_i64(odise_hip_ctx* ctx, int64_t* data, int64_t count);
/* join the last collective: block_host != 0 waits on the host, otherwise makes the compute stream wait for it */
int odise_hip_comm_wait(odise_hip_ctx* ctx, int block_host);

#ifdef __cplusplus
}
#endif
#endif /* ODISE_HIP_H */
