// sem_pq.hip — panoptic quality of a SEMANTIC segmentation on the device (odise_hip_semantic_pq, and the PQ half of
// odise_hip_semantic_eval_pq in eval_ops.hip): the metric of Mask2Former's tools/evaluate_pq_for_semantic_segmentation.py, the one PQ
// number of the semantic-only evaluation sets.  Every class of a picture is one stuff segment on either side, so a class can only match
// itself and a picture is a function of four integer vectors of length K (host restatement: odise_amd/semseg_pq.py):
//
//   area_pred[c]  pixels with pred == c            inter[c]      pixels with pred == c and gt == c
//   area_gt[c]    pixels with gt == c              void_pred[c]  pixels with pred == c on ground-truth VOID
//
// The ground truth follows HipSemSegEvaluator's contract: int32 with the ignore label mapped to K, and any value outside [0, K] counts as
// K.  (In the tool a ground-truth value that is neither a class nor the ignore label would be a segment of an unknown category; here it is
// VOID.)  Two launches per picture, no synchronisation:
//
//   sem_pq_pixel_kernel   one sweep over (labels, gt), four pixels per lane and step as two 16-byte loads when both maps are aligned.  The
//                         four vectors are one per-block histogram (lds_hist.h) of 4 K cells: in LDS up to K = 3072, in global memory
//                         above, decided once per kernel.  A pixel touches up to three cells - area_pred[l], area_gt[g] and one of
//                         inter[l] / void_pred[l] - and a lane counts the run of each in a register (HistRun), so a smooth map costs three
//                         histogram accesses per change of (pred, gt) and not per pixel.  With a score tensor the first-maximum arg-max is
//                         taken per pixel in the same sweep.  A predicted label outside [0, K) raises flag 1 and marks the picture.
//   sem_pq_decide_kernel  one block, one lane per class: the matching rule on the four counts, added to stats[c].  It is the only adder of
//                         its cell and the kernels of successive pictures are ordered on the stream: the iou sums of a stream of pictures
//                         grow by one addend per picture in picture order and are bit-identical to the tool's and from run to run.  A
//                         marked picture adds nothing.  The four vectors and the mark are left zeroed for the next picture.
#include <algorithm>

#include "common.h"
#include "lds_hist.h"

namespace odise {

constexpr int kSemPqMaxClasses = kLdsHistCells;            // as odise_hip_semantic_eval
constexpr int64_t kSemPqMaxPixels = (1ll << 29) - 1;       // per picture, as odise_hip_semantic_eval: the counts stay in 32 bits
constexpr int kSemPqHead = 4;                              // int32 cells in front of the vectors: [0] = this picture is marked
constexpr int kSemPqDecideThreads = 1024;

struct SemPqLane {
    HistRun pred, gt, both;   // the cells area_pred[l], area_gt[g], inter[l] / void_pred[l] being counted; cell -1 = none, never added
};

// One pixel.  Cells: [0, K) area_pred, [K, 2K) area_gt, [2K, 3K) inter, [3K, 4K) void_pred.  Returns false for a label outside [0, K),
// which is counted nowhere on the predicted side.
template <bool LDS>
__device__ __forceinline__ bool sem_pq_count(SemPqLane& L, int l, int g, int K, const LdsHist<unsigned>& H) {
    const bool in = (unsigned)l < (unsigned)K;
    g = (g < 0 || g > K) ? K : g;
    L.pred.count<LDS>(in ? l : -1, H);
    L.gt.count<LDS>(g < K ? K + g : -1, H);
    L.both.count<LDS>(!in ? -1 : (g == K ? 3 * K + l : (g == l ? 2 * K + l : -1)), H);
    return in;
}

// the pixels of the block, and the runs the lanes still hold; returns whether this lane met a label outside [0, K)
template <bool LDS, bool kSem>
__device__ __forceinline__ bool sem_pq_pixels(const float* __restrict__ sem, const int* __restrict__ labels, const int* __restrict__ gt, int K, int npix, int vec,
                                              const LdsHist<unsigned>& H) {
    SemPqLane L;
    L.pred.cell = L.gt.cell = L.both.cell = -1;
    bool bad = false;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (kSem) {
        for (int64_t p = first; p < npix; p += stride) sem_pq_count<LDS>(L, argmax_first(sem, K, npix, p), gt[p], K, H);
    } else {
        const int groups = vec ? npix >> 2 : 0;
        for (int64_t q = first; q < groups; q += stride) {
            const int4 l = ((const int4*)labels)[q], g = ((const int4*)gt)[q];
            bad |= !sem_pq_count<LDS>(L, l.x, g.x, K, H);
            bad |= !sem_pq_count<LDS>(L, l.y, g.y, K, H);
            bad |= !sem_pq_count<LDS>(L, l.z, g.z, K, H);
            bad |= !sem_pq_count<LDS>(L, l.w, g.w, K, H);
        }
        // pixel by pixel: everything when the maps are not 16-byte aligned, else the last npix & 3 pixels
        for (int64_t p = (int64_t)groups * 4 + first; p < npix; p += stride) bad |= !sem_pq_count<LDS>(L, labels[p], gt[p], K, H);
    }
    L.pred.flush<LDS>(H);
    L.gt.flush<LDS>(H);
    L.both.flush<LDS>(H);
    return bad;
}

// cells[kSemPqHead + 4 K] += the four vectors of the picture; cells[0] and flags |= 1 for a label outside [0, K).  lds != 0: the launch
// carries lds_hist_bytes(4 K) of dynamic LDS.  vec != 0: labels and gt are 16-byte aligned.
template <bool kSem>
__global__ void __launch_bounds__(256) sem_pq_pixel_kernel(const float* __restrict__ sem, const int* __restrict__ labels, const int* __restrict__ gt, int K,
                                                          int npix, int vec, int lds, unsigned* __restrict__ cells, int* __restrict__ flags) {
    const LdsHist<unsigned> H(cells + kSemPqHead, 4 * K, lds != 0);
    H.clear();
    H.sync();
    const bool bad = H.lds ? sem_pq_pixels<true, kSem>(sem, labels, gt, K, npix, vec, H) : sem_pq_pixels<false, kSem>(sem, labels, gt, K, npix, vec, H);
    H.sync();
    H.flush();
    if (!kSem && bad) {
        atomicOr(&cells[0], 1u);
        atomicOr(flags, 1);
    }
}

// One block.  The decision of every class from its four counts, added to stats [K]; cells left zeroed.
__global__ void __launch_bounds__(kSemPqDecideThreads) sem_pq_decide_kernel(unsigned* __restrict__ cells, int K, odise_pq_stat* __restrict__ stats) {
    const bool bad = cells[0] != 0u;   // read by every lane before lane 0 clears it
    __syncthreads();
    unsigned* v = cells + kSemPqHead;
    for (int c = threadIdx.x; c < K; c += blockDim.x) {
        const unsigned area_pred = v[c], area_gt = v[K + c], inter = v[2 * K + c], void_pred = v[3 * K + c];
        v[c] = v[K + c] = v[2 * K + c] = v[3 * K + c] = 0u;
        if (bad || !(area_pred | area_gt)) continue;
        if (inter > 0u) {
            // area_pred >= inter + void_pred (disjoint pixels of one class), so the union is at least area_gt >= inter > 0
            const int64_t uni = (int64_t)area_pred + (int64_t)area_gt - (int64_t)inter - (int64_t)void_pred;
            const double iou = (double)inter / (double)uni;
            if (iou > 0.5) {
                stats[c].tp += 1;
                stats[c].iou += iou;
                continue;
            }
        }
        if (area_gt > 0u) stats[c].fn += 1;
        if (area_pred > 0u && !((double)void_pred / (double)area_pred > 0.5)) stats[c].fp += 1;
    }
    if (threadIdx.x == 0) cells[0] = 0u;
}

int sem_pq_args(const char* what, int K, int H, int W) {
    ODISE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= kSemPqMaxPixels, "%s: picture size %dx%d out of range", what, H, W);
    ODISE_REQUIRE(K >= 1 && K <= kSemPqMaxClasses, "%s: %d classes (1..%d)", what, K, kSemPqMaxClasses);
    return ODISE_OK;
}

// Both launches of one picture, behind what is already on the context's stream.  Exactly one of labels / sem; arguments checked by the caller.
int sem_pq_enqueue(odise_hip_ctx* ctx, const int* labels, const float* sem, const int* gt, int K, int H, int W, odise_pq_stat* stats, int* flags) {
    // the context's cells: grown on demand for the largest K so far, zero whenever no picture is in flight on the stream
    const size_t need = (size_t)(kSemPqHead + 4 * (int64_t)K) * sizeof(unsigned);
    if (ctx->sem_pq.cap < need) {
        ODISE_TRY(scratch_reserve(ctx->sem_pq, need, 0, drain_streams(ctx->stream), "semantic_pq"));
        ODISE_CHECK_HIP(hipMemsetAsync(ctx->sem_pq.ptr, 0, ctx->sem_pq.cap, ctx->stream));
    }
    unsigned* cells = (unsigned*)ctx->sem_pq.ptr;
    const int npix = H * W;
    const size_t lds = lds_hist_bytes(4 * (int64_t)K);
    if (sem) {
        const dim3 grid((unsigned)std::min<int64_t>(ceil_div(npix, 256), 4 * (int64_t)ctx->cu_count));
        hipLaunchKernelGGL(sem_pq_pixel_kernel<true>, grid, dim3(256), lds, ctx->stream, sem, (const int*)nullptr, gt, K, npix, 0, lds != 0, cells, flags);
    } else {
        const int vec = (((uintptr_t)labels | (uintptr_t)gt) & 15) == 0;
        const dim3 grid((unsigned)std::min<int64_t>(ceil_div(vec ? ceil_div(npix, 4) : npix, 256), 2 * (int64_t)ctx->cu_count));
        hipLaunchKernelGGL(sem_pq_pixel_kernel<false>, grid, dim3(256), lds, ctx->stream, (const float*)nullptr, labels, gt, K, npix, vec, lds != 0, cells, flags);
    }
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sem_pq_decide_kernel, dim3(1), dim3(kSemPqDecideThreads), 0, ctx->stream, cells, K, stats);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_semantic_pq(odise_hip_ctx* ctx, const int32_t* labels, const float* sem_seg, const int32_t* gt, int K, int H, int W,
                                     odise_pq_stat* stats, int32_t* flags) {
    ODISE_REQUIRE(ctx && gt && stats && flags, "semantic_pq: null argument");
    ODISE_REQUIRE((labels != nullptr) != (sem_seg != nullptr), "semantic_pq: exactly one of labels / sem_seg");
    ODISE_TRY(sem_pq_args("semantic_pq", K, H, W));
    ODISE_REQUIRE((((uintptr_t)labels | (uintptr_t)sem_seg | (uintptr_t)gt | (uintptr_t)flags) & 3) == 0 && ((uintptr_t)stats & 7) == 0,
                  "semantic_pq: int32 / float buffers must be 4-byte aligned, the statistics 8-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    return sem_pq_enqueue(ctx, labels, sem_seg, gt, K, H, W, stats, flags);
}
