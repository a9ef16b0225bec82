// inst_match.h — COCOeval.evaluateImg's walk on the device, written once for the entry points that match detections against ground truth:
// odise_hip_instance_eval(_poly, _bbox, _boundary) (inst_eval.hip: a picture) and odise_hip_video_eval_finish (video_eval.hip: a video,
// whose "detections" are tracks).  The walk takes its IoU, its areas and its area ranges from a functor; the functors of the picture
// tasks stand here beside it, the one of the video task in video_eval.hip.
//   device  rle_iou, InstMatchArgs, SegmIou / BoxIou / BoundaryIou, NoFederation, inst_match_walk (the walk; its detection arrays have a
//           compile-time capacity), inst_match_kernel (the walk at 100 detections without federated rules; LVIS' kernel: lvis_eval.hip)
#pragma once
#include "inst_words.h"

namespace odise {

constexpr int kInstMaxGt = 1024;
constexpr int kInstCells = 40;         // 4 area ranges x 10 thresholds, bit 10 a + t

__device__ __forceinline__ double rle_iou(int inter, long long area_d, long long area_g, bool crowd) {
    if (inter == 0) return 0.0;
    return crowd ? (double)inter / (double)area_d : (double)inter / (double)(area_d + area_g - inter);
}

struct InstMatchArgs {
    const int* inst_table;       // n | query index [topk] | class [topk]; nullptr: n_det detections
    const int* det_cls;          // [topk]: the class of every detection (the third part of inst_table, or a table of the caller's)
    const float* inst_scores;    // [topk]
    const int* gt_rows;          // [n_gt][3]
    int* status;                 // the flags of this picture so far: 1 / 4 / 8 of the decode and the polygons, 2 / 4 of a match that ran before;
                                 // nullptr: none
    odise_inst_eval_row* rows;
    int* n_rows;
    int* flags;
    int topk, n_det, n_gt, num_categories, image;
    double thr[10];
};

__device__ __forceinline__ bool inst_area_outside(int area, int a) {   // [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10], ends included
    return a == 1 ? area > 1024 : a == 2 ? (area < 1024 || area > 9216) : a == 3 ? area < 9216 : false;
}

// What the walk asks of an IoU: the area of a detection and of a ground truth, the check of a ground truth (flag bits), the IoU of a pair,
// and whether an unmatched detection lies outside area range a (det_outside: its index, its area as det_area gave it, the range).
// kStatusMask: the flags of the picture that empty this task's rows; kPublish: the flags found here join `status` for the match behind.
struct SegmIou {   // rleIou on the pixel counts of inst_inter_kernel / inst_area_kernel
    static constexpr int kStatusMask = ~0;
    static constexpr bool kPublish = false;
    const int* inter;            // [topk][n_gt]
    const long long* area;       // [topk + n_gt]
    int topk, n_gt;
    __device__ int det_area(int i) const { return (int)area[i]; }
    __device__ int gt_area(int j) const { return (int)area[topk + j]; }
    __device__ int gt_check(int) const { return 0; }
    __device__ bool det_outside(int, int ad, int a) const { return inst_area_outside(ad, a); }
    __device__ double operator()(int d, int j, int ad, int ag, bool crowd) const { return rle_iou(inter[(int64_t)d * n_gt + j], ad, ag, crowd); }
};
struct BoxIou {    // bbIou of the detection's box (XYXY integers, here as XYWH) and the annotation's box
    static constexpr int kStatusMask = 2 | 4;   // bad runs (1) and bad polygons (8) are the segm task's alone
    static constexpr bool kPublish = true;
    const float* boxes;          // [topk][4] XYXY
    const double* gt_boxes;      // [n_gt][4] XYWH
    __device__ int det_area(int i) const { return (int)(boxes[4 * i + 2] - boxes[4 * i]) * (int)(boxes[4 * i + 3] - boxes[4 * i + 1]); }
    __device__ int gt_area(int) const { return 0; }
    __device__ int gt_check(int j) const {
        const double* g = gt_boxes + 4 * j;
        return isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(g[3]) ? 0 : 4;
    }
    __device__ bool det_outside(int, int ad, int a) const { return inst_area_outside(ad, a); }
    __device__ double operator()(int d, int j, int, int, bool crowd) const {
        const float* b = boxes + 4 * d;
        const double* g = gt_boxes + 4 * j;
        return bb_iou((double)b[0], (double)b[1], (double)(b[2] - b[0]), (double)(b[3] - b[1]), g[0], g[1], g[2], g[3], crowd);
    }
};
struct BoundaryIou {   // Boundary AP's IoU: min(rleIou of the masks, rleIou of their boundaries); areas and flags are the segm task's
    static constexpr int kStatusMask = ~0;
    static constexpr bool kPublish = false;
    SegmIou mask, bnd;           // the counts of the masks and of inst_boundary_words of them
    __device__ int det_area(int i) const { return mask.det_area(i); }
    __device__ int gt_area(int j) const { return mask.gt_area(j); }
    __device__ int gt_check(int) const { return 0; }
    __device__ bool det_outside(int, int ad, int a) const { return inst_area_outside(ad, a); }
    __device__ double operator()(int d, int j, int ad, int ag, bool crowd) const {
        return fmin(mask(d, j, ad, ag, crowd), bnd(d, j, bnd.det_area(d), bnd.gt_area(j), crowd));
    }
};

// The federated rules of a dataset whose pictures are annotated for some categories only (LVIS, lvis_eval.hip), as the walk asks for them:
// kOn: there are such rules, and then no crowds (iscrowd != 0 raises flag 4); keep(cls, cnt): a detection of category cls, which has cnt
// ground truths in the picture, takes part at all - one that does not produces no row.  Without rules every detection takes part.
struct NoFederation {
    static constexpr bool kOn = false;
    __device__ bool keep(int, int) const { return true; }
};

// One block.  Detections in descending score (ties keep table order), ground truths of a category in annotation order.  The 40 (area
// range, threshold) cells of a detection are the lanes 10 a + t of ONE wave, which walks the ground truths of the detection's category
// once (inst_eval.hip, step 5).  kCap: the detections the LDS arrays hold, A.topk <= kCap.
template <class Iou, int kCap, class Fed>
__device__ __forceinline__ void inst_match_walk(const InstMatchArgs& A, const Iou& iou_of, const Fed& fed) {
    __shared__ int g_cat[kInstMaxGt], g_flag[kInstMaxGt], g_area[kInstMaxGt], g_sorted[kInstMaxGt];   // g_flag: iscrowd | outside bits << 1
    __shared__ u64 g_matched[kInstMaxGt];                                                             // bit = cell
    __shared__ int d_cls[kCap], d_area[kCap], d_order[kCap], d_lo[kCap], d_cnt[kCap];
    __shared__ float d_score[kCap];
    __shared__ int bad, n_keep;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int topk = A.topk, n_gt = A.n_gt;
    const int n = A.inst_table ? inst_count(A.inst_table, topk) : min(max(A.n_det, 0), topk);
    if (tid == 0) bad = A.status ? A.status[0] & Iou::kStatusMask : 0;
    __syncthreads();
    int f = 0;
    for (int j = tid; j < n_gt; j += kRleThreads) {
        const int cat = A.gt_rows[3 * j], crowd = A.gt_rows[3 * j + 1];
        if ((unsigned)cat >= (unsigned)A.num_categories || (unsigned)crowd > (Fed::kOn ? 0u : 1u)) f |= 4;
        g_cat[j] = cat;
        g_flag[j] = (crowd & 1) | ((A.gt_rows[3 * j + 2] & 15) << 1);
        f |= iou_of.gt_check(j);
        g_area[j] = iou_of.gt_area(j);
        g_matched[j] = 0ull;
    }
    for (int i = tid; i < n; i += kRleThreads) {
        d_cls[i] = A.det_cls[i];
        if ((unsigned)d_cls[i] >= (unsigned)A.num_categories) f |= 2;
        const float s = A.inst_scores[i];
        d_score[i] = s == s ? s : -INFINITY;
        d_area[i] = iou_of.det_area(i);
    }
    if (f) {
        atomicOr(&bad, f);
        if (Iou::kPublish) atomicOr(A.status, f);
    }
    __syncthreads();
    const odise_inst_eval_row zero = {};
    if (bad) {   // the picture counts nothing
        for (int i = tid; i < topk; i += kRleThreads) A.rows[i] = zero;
        if (tid == 0) {
            A.n_rows[0] = 0;
            atomicOr(A.flags, bad);
        }
        return;
    }
    int nk = n;   // the detections that take part: rows 0 .. nk - 1
    if constexpr (!Fed::kOn) {
        for (int i = n + tid; i < topk; i += kRleThreads) A.rows[i] = zero;
        if (tid == 0) A.n_rows[0] = n;
    } else {      // the ground truths of every detection's category first: they decide who takes part (d_cnt < 0: not this one)
        if (tid == 0) n_keep = 0;
        __syncthreads();
        for (int i = tid; i < n; i += kRleThreads) {
            int lo = 0, cnt = 0;
            for (int j = 0; j < n_gt; ++j) {
                lo += g_cat[j] < d_cls[i] ? 1 : 0;
                cnt += g_cat[j] == d_cls[i] ? 1 : 0;
            }
            const bool keep = fed.keep(d_cls[i], cnt);
            d_lo[i] = lo;
            d_cnt[i] = keep ? cnt : -1;
            if (keep) atomicAdd(&n_keep, 1);
        }
        __syncthreads();
        nk = n_keep;
        for (int i = nk + tid; i < topk; i += kRleThreads) A.rows[i] = zero;
        if (tid == 0) A.n_rows[0] = nk;
    }
    // descending score, ties in table order; the ground truths of a detection's category: g_sorted[d_lo .. d_lo + d_cnt), annotation order
    for (int i = tid; i < n; i += kRleThreads) {
        if constexpr (!Fed::kOn) {
            int r = 0, lo = 0, cnt = 0;
            for (int j = 0; j < n; ++j) r += (d_score[j] > d_score[i] || (d_score[j] == d_score[i] && j < i)) ? 1 : 0;
            d_order[r] = i;
            for (int j = 0; j < n_gt; ++j) {
                lo += g_cat[j] < d_cls[i] ? 1 : 0;
                cnt += g_cat[j] == d_cls[i] ? 1 : 0;
            }
            d_lo[i] = lo;
            d_cnt[i] = cnt;
        } else if (d_cnt[i] >= 0) {   // the rank among those that take part
            int r = 0;
            for (int j = 0; j < n; ++j) r += (d_cnt[j] >= 0 && (d_score[j] > d_score[i] || (d_score[j] == d_score[i] && j < i))) ? 1 : 0;
            d_order[r] = i;
        }
    }
    for (int j = tid; j < n_gt; j += kRleThreads) {
        int r = 0;
        for (int k = 0; k < n_gt; ++k) r += (g_cat[k] < g_cat[j] || (g_cat[k] == g_cat[j] && k < j)) ? 1 : 0;
        g_sorted[r] = j;
    }
    __syncthreads();

    const bool cell = lane < kInstCells;
    const int a = cell ? lane / 10 : 0, t = cell ? lane - 10 * a : 0;
    const double thr = fmin(A.thr[t], 1.0 - 1e-10);
    for (int k = 0; k < nk; ++k) {
        const int d = d_order[k];
        if ((d_cls[d] & (kRleThreads / 64 - 1)) != wave) continue;   // a category belongs to one wave: its ground truths are touched by no other
        const int ad = d_area[d], lo = d_lo[d], cnt = d_cnt[d];
        double best1 = thr, best2 = thr;
        int m1 = -1, m2 = -1;
        for (int base = 0; base < cnt; base += 64) {
            double mine = 0.0;
            if (base + lane < cnt) {
                const int j = g_sorted[lo + base + lane];
                mine = iou_of(d, j, ad, g_area[j], g_flag[j] & 1);
            }
            const int step = min(64, cnt - base);
            for (int q = 0; q < step; ++q) {
                const int j = g_sorted[lo + base + q];
                const double iou = __shfl(mine, q);
                const int gf = g_flag[j];
                const bool crowd = gf & 1, ign = crowd || ((gf >> (1 + a)) & 1), matched = (g_matched[j] >> lane) & 1ull;
                if (!ign) {
                    if (!matched && iou >= best1) { best1 = iou; m1 = j; }
                } else if ((crowd || !matched) && iou >= best2) { best2 = iou; m2 = j; }
            }
        }
        const int m = m1 >= 0 ? m1 : m2;
        bool ig;
        if (m >= 0) {
            ig = m1 < 0;   // the ignore bit of the ground truth it took
            if (cell) atomicOr(&g_matched[m], 1ull << lane);
        } else {
            ig = iou_of.det_outside(d, ad, a);
        }
        const u64 mw = __ballot(cell && m >= 0), iw = __ballot(cell && ig);
        if (lane == 0) {
            odise_inst_eval_row row;
            row.score = A.inst_scores[d]; row.category = d_cls[d]; row.area = ad; row.image = A.image;
            row.matched = mw; row.ignored = iw;
            A.rows[k] = row;
        }
    }
}

template <class Iou>
__global__ void __launch_bounds__(kRleThreads) inst_match_kernel(InstMatchArgs A, Iou iou_of) {
    inst_match_walk<Iou, kInstMaxTopk>(A, iou_of, NoFederation{});
}

}  // namespace odise
