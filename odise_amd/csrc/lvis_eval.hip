// lvis_eval.hip — odise_hip_lvis_eval: one picture of LVISEval.evaluate_img for iouType "segm" (lvis-api, detectron2's LVISEvaluator) on the
// device.  It is the walk of odise_hip_instance_eval (inst_match.h) at up to 300 detections over ALL categories, with the federated rules
// of a dataset whose pictures are annotated for some categories only.  Host restatement, which is the specification: odise_amd/lvis_eval.py.
//
//   1. distinct  with detections taken from the mask logits the table holds (query, class) pairs, 300 of them over at most 100 queries.
//                One block lists the distinct queries in the order of their first appearance (uniq = n_distinct | query ..) and gives every
//                table index the position of its query in that list (det_row).
//   2. pack      uniq goes through inst_pack where inst_table went: a query is sampled from the mask logits ONCE, and steps 3 and 4 of
//                inst_eval.hip (decode / rasterise, inter, area) run on [n_distinct] x [n_gt] masks.  Dense masks are one per detection:
//                nothing to share, det_row is the identity.
//   3. match     inst_match_walk at a capacity of 300 detections (31 KB of LDS).  LvisSegmIou maps a detection to its query's row of the
//                counts and ignores an unmatched detection of a not-exhaustive category in every range; LvisFederation drops a detection
//                whose category has no ground truth in the picture (pos, counted from gt_rows in the walk) and is not in neg.  The two
//                bitsets are read from global memory: a detection looks at one bit of each.
// Scope: iouType "segm".  LVIS "bbox" and "boundary" would be two more functors over the same walk (det_outside is where the
// not-exhaustive rule enters).
#include "inst_match.h"

namespace odise {

constexpr int kLvisMaxDets = 300;      // LVISEval's max_dets: per picture, over all categories
constexpr int kLvisMaxK = 65535;

__device__ __forceinline__ bool lvis_bit(const uint32_t* __restrict__ bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1u; }

struct LvisSegmIou {   // SegmIou on the packed rows: detection i is row det_row[i] (nullptr: row i)
    static constexpr int kStatusMask = ~0;
    static constexpr bool kPublish = false;
    SegmIou counts;
    const int* det_row;
    const int* det_cls;                    // [topk], checked against num_categories before det_outside looks at it
    const uint32_t* not_exhaustive;
    __device__ int row(int i) const { return det_row ? det_row[i] : i; }
    __device__ int det_area(int i) const { return counts.det_area(row(i)); }
    __device__ int gt_area(int j) const { return counts.gt_area(j); }
    __device__ int gt_check(int) const { return 0; }
    __device__ bool det_outside(int d, int ad, int a) const { return inst_area_outside(ad, a) || lvis_bit(not_exhaustive, det_cls[d]); }
    __device__ double operator()(int d, int j, int ad, int ag, bool) const { return counts(row(d), j, ad, ag, false); }
};
struct LvisFederation {
    static constexpr bool kOn = true;
    const uint32_t* neg;
    __device__ bool keep(int cls, int cnt) const { return cnt > 0 || lvis_bit(neg, cls); }
};

__global__ void __launch_bounds__(kRleThreads) lvis_match_kernel(InstMatchArgs A, LvisSegmIou iou_of, LvisFederation fed) {
    inst_match_walk<LvisSegmIou, kLvisMaxDets>(A, iou_of, fed);
}

// ---- 1. distinct --------------------------------------------------------------------------------------------------------------------------
// uniq = n_distinct | the distinct query indices of table, in the order of their first appearance; det_row[i] = where table index i's query
// stands in that list (i below the count of the table; the rest is not written).  cap: the rows the pack has, the queries of the head or
// topk, whichever is less - a table of valid query indices cannot hold more distinct ones, and one that does is cut there, so that no row
// index leaves the counts.  One block; 300^2 comparisons at the most.
__global__ void __launch_bounds__(256) lvis_distinct_kernel(const int* __restrict__ table, int topk, int cap, int* __restrict__ uniq,
                                                           int* __restrict__ det_row) {
    __shared__ int q[kLvisMaxDets], first[kLvisMaxDets];
    __shared__ int total;
    const int tid = threadIdx.x;
    const int n = inst_count(table, topk);
    if (tid == 0) total = 0;
    for (int i = tid; i < n; i += 256) q[i] = table[1 + i];
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        int j = 0;
        while (j < i && q[j] != q[i]) ++j;
        first[i] = j;
        if (j == i) atomicAdd(&total, 1);
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int f = first[i];
        int r = 0;
        for (int j = 0; j < f; ++j) r += first[j] == j ? 1 : 0;
        det_row[i] = min(r, cap - 1);
        if (f == i && r < cap) uniq[1 + r] = q[i];
    }
    if (tid == 0) uniq[0] = min(total, cap);
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_lvis_eval(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p, const odise_lvis_task* lv) {
    ODISE_REQUIRE(ctx && d && lv, "lvis_eval: null argument");
    ODISE_REQUIRE(lv->neg_bits && lv->not_exhaustive_bits, "lvis_eval: null category bitset");
    ODISE_REQUIRE((((uintptr_t)lv->neg_bits | (uintptr_t)lv->not_exhaustive_bits) & 3) == 0, "lvis_eval: category bitsets must be 4-byte aligned");
    ODISE_REQUIRE(d->iou_thresholds && d->flags && d->rows && d->n_rows, "lvis_eval: null pointer");
    InstSource src = inst_source(*d);
    ODISE_TRY(inst_source_check("lvis_eval", src, true, kRleMaxPixels, kLvisMaxDets));
    ODISE_REQUIRE(d->n_gt >= 0 && d->n_gt <= kInstMaxGt, "lvis_eval: %d ground-truth masks (0..%d)", d->n_gt, kInstMaxGt);
    ODISE_REQUIRE(d->n_gt == 0 || (d->gt_rows && d->gt_runs && d->gt_offsets), "lvis_eval: null ground truth");
    ODISE_REQUIRE(!p || p->n_poly >= 0, "lvis_eval: %d polygons", p->n_poly);
    if (p && (d->n_gt == 0 || p->n_poly == 0)) p = nullptr;   // nothing to rasterise
    ODISE_REQUIRE(!p || (p->xy && p->poly_offsets && p->gt_polys), "lvis_eval: null polygon ground truth");
    ODISE_REQUIRE(d->num_categories >= 1 && d->num_categories <= kLvisMaxK, "lvis_eval: num_categories %d (1..%d)", d->num_categories, kLvisMaxK);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "lvis_eval", src, &ig));
    const RleGrid G = rle_grid(d->h, d->w);
    const int topk = d->topk, n_gt = d->n_gt;
    const bool shared = !src.masks;   // (query, class) pairs: a query is packed once
    const int n_pack = shared ? std::min(topk, ig.g.Q) : topk;   // the masks that are packed, counted and intersected
    InstScratch s;
    ODISE_TRY(inst_scratch(ctx, n_pack, n_gt, G, &s, p != nullptr, false, false, shared ? (size_t)(1 + 2 * topk) * sizeof(int) : 0));
    ODISE_CHECK_HIP(hipMemsetAsync(s.inter, 0, s.inter_bytes, ctx->stream));
    int* status = s.inter + (size_t)n_pack * n_gt;
    int *uniq = (int*)s.extra, *det_row = shared ? uniq + 1 + topk : nullptr;
    if (shared) {
        hipLaunchKernelGGL(lvis_distinct_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)d->inst_table, topk, n_pack, uniq, det_row);
        ODISE_CHECK_HIP(hipGetLastError());
        src.inst_table = uniq;   // the pack reads its count on the device: rows past n_distinct stay unwritten, and no detection maps to them
        src.topk = n_pack;
    }
    ODISE_TRY(inst_pack(ctx, src, ig, G, s.words_d));
    ODISE_TRY(inst_overlaps(ctx, s, G, n_pack, d->gt_runs, d->gt_offsets, n_gt, status, p));
    InstMatchArgs A;
    A.inst_table = (const int*)d->inst_table; A.det_cls = A.inst_table + 1 + topk; A.inst_scores = d->inst_scores; A.gt_rows = (const int*)d->gt_rows;
    A.status = status; A.flags = (int*)d->flags; A.rows = d->rows; A.n_rows = (int*)d->n_rows;
    A.topk = topk; A.n_det = 0; A.n_gt = n_gt; A.num_categories = d->num_categories; A.image = d->image;
    for (int t = 0; t < 10; ++t) A.thr[t] = d->iou_thresholds[t];
    const LvisSegmIou iou{SegmIou{s.inter, s.area, n_pack, n_gt}, det_row, A.det_cls, lv->not_exhaustive_bits};
    hipLaunchKernelGGL(lvis_match_kernel, dim3(1), dim3(kRleThreads), 0, ctx->stream, A, iou, LvisFederation{lv->neg_bits});
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
