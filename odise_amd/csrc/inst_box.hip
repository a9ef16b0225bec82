// inst_box.hip — the boxes of instance masks on the device: odise_hip_instance_boxes (detectron2 BitMasks.get_bounding_boxes of a picture's
// instance selection, the line maskformer_model.py:372 leaves out as "slow") and odise_hip_box_iou (maskApi.c bbIou).  Host restatement:
// odise_amd/instance_eval.py mask_boxes / box_iou.
//
// A box is a reduction over the packed words of inst_words.h / rle_pack.h: word (x, r) of a mask holds rows 64 r .. 64 r + 63 of column x,
// so a non-zero word gives the column x and the rows 64 r + ctz(word) .. 64 r + 63 - clz(word), and the box is the minimum / maximum of
// those over the mask's words.  One block per mask reads the words in their stored order (consecutive threads, consecutive words), keeps
// four integers per thread and reduces them by shuffles and through LDS, as block_popcount does.
// Bits at or beyond row h: every producer of these words (rle_pack_dense_kernel, rle_pack_x4_kernel, rle_pack_generic_kernel of rle.hip)
// sets bit k of the last word of a column only for k < h - 64 r, so the tails are zero and nothing is masked out here.
#include <climits>

#include "inst_words.h"

namespace odise {

__global__ void __launch_bounds__(256) inst_box_kernel(const u64* __restrict__ words, RleGrid G, const int* __restrict__ inst_table, int topk,
                                                       float* __restrict__ boxes) {
    __shared__ int part[4][4];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* out = boxes + 4 * i;
    if (i >= inst_count(inst_table, topk)) {   // the logits pack leaves these words unwritten
        if (tid < 4) out[tid] = 0.f;
        return;
    }
    const u64* wd = words + (int64_t)i * G.nw;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    // word k = x * R + r; a step of 256 words is dx columns and dr words further on
    const int dx = 256 / G.R, dr = 256 - dx * G.R;
    int x = tid / G.R, r = tid - x * G.R;
    for (int64_t k = tid; k < G.nw; k += 256) {
        const u64 v = wd[k];
        if (v) {
            x0 = min(x0, x); x1 = max(x1, x);
            y0 = min(y0, 64 * r + __ffsll(v) - 1);
            y1 = max(y1, 64 * r + 63 - __clzll(v));
        }
        x += dx; r += dr;
        if (r >= G.R) { r -= G.R; ++x; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        x0 = min(x0, __shfl_down(x0, o)); y0 = min(y0, __shfl_down(y0, o));
        x1 = max(x1, __shfl_down(x1, o)); y1 = max(y1, __shfl_down(y1, o));
    }
    if ((tid & 63) == 0) {
        int* p = part[tid >> 6];
        p[0] = x0; p[1] = y0; p[2] = x1; p[3] = y1;
    }
    __syncthreads();
    if (tid < 4) {   // thread c writes member c: x0, y0 are minima, x1 + 1, y1 + 1 maxima
        const int a = part[0][tid], b = part[1][tid], c = part[2][tid], d = part[3][tid];
        const bool empty = max(max(part[0][2], part[1][2]), max(part[2][2], part[3][2])) < 0;
        const int v = tid < 2 ? min(min(a, b), min(c, d)) : max(max(a, b), max(c, d)) + 1;
        out[tid] = empty ? 0.f : (float)v;
    }
}

int inst_boxes_launch(odise_hip_ctx* ctx, const u64* words, const RleGrid& G, const int* inst_table, int topk, float* boxes) {
    hipLaunchKernelGGL(inst_box_kernel, dim3((unsigned)topk), dim3(256), 0, ctx->stream, words, G, inst_table, topk, boxes);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

__global__ void __launch_bounds__(256) box_iou_kernel(const double* __restrict__ dt, const double* __restrict__ gt, int n, int n_gt,
                                                      const uint8_t* __restrict__ iscrowd, double* __restrict__ iou) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * n_gt) return;
    const int d = (int)(i / n_gt), g = (int)(i - (int64_t)d * n_gt);
    const double *D = dt + 4 * d, *B = gt + 4 * g;
    iou[i] = bb_iou(D[0], D[1], D[2], D[3], B[0], B[1], B[2], B[3], iscrowd && iscrowd[g] != 0);
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_sizeof_inst_boxes_desc(void) { return (int)sizeof(odise_inst_boxes_desc); }
extern "C" int odise_hip_sizeof_inst_bbox_task(void) { return (int)sizeof(odise_inst_bbox_task); }

extern "C" int odise_hip_instance_boxes(odise_hip_ctx* ctx, const odise_inst_boxes_desc* d) {
    ODISE_REQUIRE(ctx && d && d->boxes, "instance_boxes: null argument");
    ODISE_REQUIRE(d->masks || d->inst_table, "instance_boxes: null inst_table (optional only with dense masks)");
    ODISE_REQUIRE(d->topk >= 1 && d->topk <= kInstMaxTopk, "instance_boxes: topk %d (1..%d)", d->topk, kInstMaxTopk);
    ODISE_REQUIRE(d->h >= 1 && d->w >= 1 && (int64_t)d->h * d->w <= kRleMaxPixels, "instance_boxes: mask size %dx%d out of range", d->h, d->w);
    ODISE_REQUIRE(!d->masks || d->dtype == ODISE_F32 || d->dtype == ODISE_U8, "instance_boxes: dtype %d (ODISE_F32 or ODISE_U8)", d->dtype);
    ODISE_REQUIRE((((uintptr_t)d->inst_table | (uintptr_t)d->boxes) & 3) == 0, "instance_boxes: inst_table / boxes must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const InstSource src = inst_source(*d);
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "instance_boxes", src, &ig));
    const RleGrid G = rle_grid(d->h, d->w);
    ODISE_TRY(scratch_reserve(ctx->rle, (size_t)d->topk * G.nw * 8, 8, drain_streams(ctx->stream), "rle"));
    u64* words = (u64*)ctx->rle.ptr;
    ODISE_TRY(inst_pack(ctx, src, ig, G, words));
    return inst_boxes_launch(ctx, words, G, src.inst_table, d->topk, d->boxes);
}

extern "C" int odise_hip_box_iou(odise_hip_ctx* ctx, const double* dt, int n, const double* gt, int n_gt, const uint8_t* iscrowd, double* iou) {
    ODISE_REQUIRE(ctx, "box_iou: null argument");
    ODISE_REQUIRE(n >= 0 && n <= 65535 && n_gt >= 0 && n_gt <= 65535 && (int64_t)n * n_gt <= (1 << 26), "box_iou: %d x %d boxes out of range", n, n_gt);
    if (n == 0 || n_gt == 0) return ODISE_OK;
    ODISE_REQUIRE(dt && gt && iou, "box_iou: null argument");
    ODISE_REQUIRE((((uintptr_t)dt | (uintptr_t)gt | (uintptr_t)iou) & 7) == 0, "box_iou: boxes and iou must be 8-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(box_iou_kernel, dim3((unsigned)ceil_div((int64_t)n * n_gt, 256)), dim3(256), 0, ctx->stream, dt, gt, n, n_gt, iscrowd, iou);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
