// pq.hip — panoptic quality statistics of one picture on the device (odise_hip_panoptic_quality).
//
// What COCOPanopticEvaluator needs from a prediction is what panopticapi's pq_compute_single_core adds into (iou, tp, fp, fn) per category.
// The prediction is the panoptic record of odise_hip_postprocess_batch / odise_hip_infer (ids, n, (id, isthing, category) rows) and is
// already in HBM; the ground truth is the annotation PNG as decoded (RGB bytes, id = R + 256 G + 65536 B) and its segments_info table.
// Two launches per picture, no synchronisation (host restatement: odise_amd/panoptic_quality.py):
//
//   pq_pixel_kernel   one sweep over the pixels.  Four pixels per lane and step: the prediction as one 16-byte load, the RGB ground truth as
//                     three dwords.  Ids become table SLOTS (0 = VOID, 1 + row, last = "not in the table") through the two id tables held
//                     in LDS; a lane keeps its last (id -> slot) of either side, so on smooth maps the translation is a compare.  Pairs
//                     are counted in the per-block histogram (lds_hist.h) of (n_gt + 2) x (n + 2) cells over the context's matrix; a lane
//                     counts a run of equal pairs in a register and touches the histogram when the pair changes.
//   pq_match_kernel   one block over that matrix: areas (column sums), the flags, the candidate pairs and their IoU in parallel, then the
//                     ORDERED part - the IoU sum of a category is added pair by pair in ascending (gt id, pred id) order by one thread
//                     per category, starting from the value already in `stats`, which makes a stream of pictures bit-identical to the
//                     single-process evaluator - then fn / fp, and the matrix is left zeroed for the next picture.
#include <algorithm>

#include "common.h"
#include "lds_hist.h"
#include "record.h"
#include "rgb.h"

namespace odise {

constexpr int kPqMaxGt = 254;                               // ground-truth rows per picture
constexpr int kPqGtSlots = kPqMaxGt + 2;                    // + VOID + "not in the table"
constexpr int kPqPredSlots = ODISE_MAX_SEGMENTS + 2;
constexpr int kPqMatrixCells = kPqGtSlots * kPqPredSlots;   // the context's matrix holds the caps; a picture uses (n_gt + 2) x (n + 2) of it
constexpr int kPqRing = 8;                                  // pinned staging slots of the ground-truth table (calls in flight before the host waits)
constexpr int kPqMatchThreads = 512;

struct PqScratch {
    int* matrix = nullptr;      // device [kPqMatrixCells], zero between calls
    int* gt_table = nullptr;    // device [kPqMaxGt][4]: the table of the call being enqueued (calls are ordered on the stream)
    int* host = nullptr;        // pinned [kPqRing][kPqMaxGt][4]
    hipEvent_t ev[kPqRing] = {};
    int next = 0;
};

// slot of `id` in a table of `rows` ids: 0 = VOID (id 0 only: a negative id is looked up), 1 + first row holding it, rows + 1 = absent
__device__ __forceinline__ int pq_find_slot(const int* ids, int rows, int id) {
    if (id == 0) return 0;
    const int r = record_find(ids, rows, id);
    return r < 0 ? rows + 1 : r + 1;
}

struct PqTables {   // the two id tables in LDS
    const int* gt_ids;
    int n_gt;
    const int* pred_ids;
    int n;
};

struct PqLane {
    RecordMemo gt, pred;   // the lane's last translations
    HistRun pair;          // the pair being counted and its length so far
};

template <bool LDS>
__device__ __forceinline__ void pq_count(PqLane& L, int gid, int pid, const PqTables& T, const LdsHist<int>& H) {
    const int gslot = record_memo(L.gt, gid, [&](int id) { return pq_find_slot(T.gt_ids, T.n_gt, id); });
    const int pslot = record_memo(L.pred, pid, [&](int id) { return pq_find_slot(T.pred_ids, T.n, id); });
    L.pair.count<LDS>(gslot * (T.n + 2) + pslot, H);   // < (n_gt + 2) * (n + 2) <= kPqMatrixCells
}

// the pixels of the block, and the runs the lanes still hold
template <bool LDS>
__device__ __forceinline__ void pq_pixels(const int* __restrict__ pred, const void* __restrict__ gt, int gt_layout, int npix, int vec, const PqTables& T,
                                          const LdsHist<int>& H) {
    PqLane L = {{0, 0}, {0, 0}, {}};   // VOID -> slot 0 holds for both tables
    const uint8_t* gt8 = (const uint8_t*)gt;
    const int* gt32 = (const int*)gt;
    const int groups = npix >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
            const int4 p = ((const int4*)pred)[q];
            unsigned g[4];
            if (gt_layout == 0) {
                const unsigned* d = (const unsigned*)gt + 3 * q;   // bytes 12 q .. 12 q + 11 < 3 npix
                rgb4_unpack(d[0], d[1], d[2], g);
            } else {
                const uint4 v = ((const uint4*)gt)[q];
                g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
            }
            pq_count<LDS>(L, (int)g[0], p.x, T, H);
            pq_count<LDS>(L, (int)g[1], p.y, T, H);
            pq_count<LDS>(L, (int)g[2], p.z, T, H);
            pq_count<LDS>(L, (int)g[3], p.w, T, H);
        }
    }
    // pixel by pixel: everything when the buffers are not aligned, else the last npix & 3 pixels
    for (int64_t i = (vec ? (int64_t)groups * 4 : 0) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride)
        pq_count<LDS>(L, gt_layout == 0 ? (int)rgb_load(gt8 + 3 * i) : gt32[i], pred[i], T, H);
    L.pair.flush<LDS>(H);
}

// matrix[(n_gt + 2) x (n + 2)] += pair counts of the picture.  vec != 0: pred 16-byte aligned and gt dword aligned (groups of 4 pixels are
// read whole); the last npix & 3 pixels and unaligned buffers are read pixel by pixel.  lds_cells = cells of the dynamic LDS histogram.
__global__ void __launch_bounds__(256) pq_pixel_kernel(const int* __restrict__ pred, const int* __restrict__ pred_segments, const void* __restrict__ gt,
                                                      int gt_layout, const int* __restrict__ gt_table, int n_gt, int npix, int vec, int lds_cells,
                                                      int* __restrict__ matrix) {
    __shared__ int gt_ids[kPqMaxGt];
    __shared__ int pred_tab[ODISE_MAX_SEGMENTS];
    const int n = record_rows(pred_segments);
    const int cells = (n_gt + 2) * (n + 2);
    const LdsHist<int> H(matrix, cells, cells <= lds_cells);
    for (int i = threadIdx.x; i < n_gt; i += blockDim.x) gt_ids[i] = gt_table[4 * i];
    record_load(pred_segments, n, pred_tab);
    const PqTables T = {gt_ids, n_gt, pred_tab, n};
    H.clear();
    __syncthreads();
    if (H.lds) pq_pixels<true>(pred, gt, gt_layout, npix, vec, T, H);
    else pq_pixels<false>(pred, gt, gt_layout, npix, vec, T, H);
    __syncthreads();
    H.flush();
}

// intersection over union of a candidate pair, as the double division of the two integers; a union <= 0 (only a JSON area that disagrees
// with the map can produce one) matches nothing
__device__ __forceinline__ bool pq_pair_iou(int inter, int area_pred, int area_gt, int void_pred, double* iou) {
    const int64_t uni = (int64_t)area_pred + (int64_t)area_gt - inter - void_pred;
    if (uni <= 0) return false;
    *iou = (double)inter / (double)uni;
    return *iou > 0.5;
}

// One block.  matrix [(n_gt + 2) x (n + 2)] pair counts of the picture (slot 0 = VOID, last slot = not in the table); zeroed on return.
__global__ void __launch_bounds__(kPqMatchThreads) pq_match_kernel(int* __restrict__ matrix, const int* __restrict__ pred_segments,
                                                                  const int* __restrict__ gt_table, int n_gt, int C,
                                                                  odise_pq_stat* __restrict__ stats, int* __restrict__ flags) {
    __shared__ int g_id[kPqMaxGt], g_cat[kPqMaxGt], g_crowd[kPqMaxGt], g_area[kPqMaxGt];
    __shared__ int g_order[kPqMaxGt];                 // rows by ascending (id, row)
    __shared__ int g_cnt[kPqMaxGt], g_first[kPqMaxGt];   // matches of a row, and the pred row of its match when there is exactly one
    __shared__ double g_iou[kPqMaxGt];
    __shared__ int p_id[ODISE_MAX_SEGMENTS], p_cat[ODISE_MAX_SEGMENTS], p_order[ODISE_MAX_SEGMENTS], p_matched[ODISE_MAX_SEGMENTS];
    __shared__ int p_area[kPqPredSlots], p_void[kPqPredSlots];
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = record_rows(pred_segments);
    const int W = n + 2, cells = (n_gt + 2) * W;
    if (tid == 0) bad = 0;
    for (int i = tid; i < n_gt; i += nt) {
        g_id[i] = gt_table[4 * i]; g_cat[i] = gt_table[4 * i + 1]; g_crowd[i] = gt_table[4 * i + 2]; g_area[i] = gt_table[4 * i + 3];
        g_cnt[i] = 0; g_first[i] = -1; g_iou[i] = 0.0;
    }
    for (int i = tid; i < n; i += nt) { p_id[i] = record_id(pred_segments, i); p_cat[i] = record_category(pred_segments, i); p_matched[i] = 0; }
    for (int p = tid; p < W; p += nt) {               // pred areas = column sums
        int a = 0;
        for (int g = 0; g < n_gt + 2; ++g) a += matrix[g * W + p];
        p_area[p] = a;
        p_void[p] = matrix[p];
    }
    __syncthreads();
    int f = 0;
    if (tid == 0 && p_area[n + 1] > 0) f |= 1;                                   // an id of the map is missing from the table
    for (int i = tid; i < n; i += nt) {
        if (p_area[1 + i] == 0) f |= 2;                                          // a row without a pixel (also: a second row of an id, id 0)
        if ((unsigned)p_cat[i] >= (unsigned)C) f |= 4;
    }
    if (f) atomicOr(&bad, f);
    // ascending-id orders (unsorted tables; the rank of a row = rows with a smaller (id, row))
    for (int i = tid; i < n_gt; i += nt) {
        int r = 0;
        for (int j = 0; j < n_gt; ++j) r += (g_id[j] < g_id[i] || (g_id[j] == g_id[i] && j < i)) ? 1 : 0;
        g_order[r] = i;
    }
    for (int i = tid; i < n; i += nt) {
        int r = 0;
        for (int j = 0; j < n; ++j) r += (p_id[j] < p_id[i] || (p_id[j] == p_id[i] && j < i)) ? 1 : 0;
        p_order[r] = i;
    }
    __syncthreads();
    if (bad) {                                         // the picture counts nothing
        if (tid == 0) flags[0] |= bad;
        for (int i = tid; i < cells; i += nt) matrix[i] = 0;
        return;
    }
    // candidates: both ids in their tables, pixels in common, not a crowd row, equal categories
    for (int i = tid; i < n_gt * n; i += nt) {
        const int g = i / n, p = i - g * n;
        if (g_crowd[g] || g_cat[g] != p_cat[p]) continue;
        const int inter = matrix[(g + 1) * W + p + 1];
        double iou;
        if (inter <= 0 || !pq_pair_iou(inter, p_area[p + 1], g_area[g], p_void[p + 1], &iou)) continue;
        p_matched[p] = 1;
        if (atomicAdd(&g_cnt[g], 1) == 0) { g_first[g] = p; g_iou[g] = iou; }   // read back only when the row has exactly one match
    }
    __syncthreads();
    // the ordered sums: the first matched row of a category in ascending id order adds all matches of that category, in order
    for (int r = tid; r < n_gt; r += nt) {
        const int g = g_order[r];
        if (!g_cnt[g]) continue;
        const int cat = g_cat[g];
        bool leader = true;
        for (int q = 0; q < r && leader; ++q) leader = !(g_cnt[g_order[q]] && g_cat[g_order[q]] == cat);
        if (!leader) continue;
        double sum = stats[cat].iou;
        int64_t tp = 0;
        for (int q = r; q < n_gt; ++q) {
            const int h = g_order[q];
            if (!g_cnt[h] || g_cat[h] != cat) continue;
            tp += g_cnt[h];
            if (g_cnt[h] == 1) { sum += g_iou[h]; continue; }
            for (int k = 0; k < n; ++k) {              // several matches (a JSON area that disagrees with the map): again, in pred-id order
                const int p = p_order[k];
                if (p_cat[p] != cat) continue;
                const int inter = matrix[(h + 1) * W + p + 1];
                double iou;
                if (inter > 0 && pq_pair_iou(inter, p_area[p + 1], g_area[h], p_void[p + 1], &iou)) sum += iou;
            }
        }
        stats[cat].iou = sum;
        stats[cat].tp += tp;
    }
    // false negatives: unmatched rows that are no crowd rows, with or without pixels
    for (int g = tid; g < n_gt; g += nt)
        if (!g_cnt[g] && !g_crowd[g]) atomicAdd((unsigned long long*)&stats[g_cat[g]].fn, 1ull);
    // false positives: unmatched predictions that do not lie mostly in VOID plus the (last) crowd row of their category
    for (int p = tid; p < n; p += nt) {
        if (p_matched[p]) continue;
        int crowd = -1;
        for (int g = 0; g < n_gt; ++g)
            if (g_crowd[g] && g_cat[g] == p_cat[p]) crowd = g;
        int64_t ign = p_void[p + 1];
        if (crowd >= 0) ign += matrix[(crowd + 1) * W + p + 1];
        if ((double)ign / (double)p_area[p + 1] > 0.5) continue;
        atomicAdd((unsigned long long*)&stats[p_cat[p]].fp, 1ull);
    }
    __syncthreads();
    for (int i = tid; i < cells; i += nt) matrix[i] = 0;
}

void pq_release(odise_hip_ctx* ctx) {
    PqScratch* s = (PqScratch*)ctx->pq;
    if (!s) return;
    if (s->matrix) (void)hipFree(s->matrix);
    if (s->gt_table) (void)hipFree(s->gt_table);
    if (s->host) (void)hipHostFree(s->host);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    ctx->pq = nullptr;
}

// The scratch is published in the context only when all of it exists and the matrix is zeroed; a failure on the way releases what was made,
// so a later call starts over and never counts into a matrix that was not cleared.
static int pq_scratch(odise_hip_ctx* ctx, PqScratch** out) {
    if (!ctx->pq) {
        PqScratch* s = new PqScratch();
        ctx->pq = s;   // pq_release works on the context
        const size_t table = (size_t)kPqMaxGt * 4 * sizeof(int);
        bool ok = hipMalloc((void**)&s->matrix, (size_t)kPqMatrixCells * sizeof(int)) == hipSuccess &&
                  hipMalloc((void**)&s->gt_table, table) == hipSuccess &&
                  hipHostMalloc((void**)&s->host, kPqRing * table, hipHostMallocDefault) == hipSuccess;
        for (hipEvent_t& e : s->ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMemsetAsync(s->matrix, 0, (size_t)kPqMatrixCells * sizeof(int), ctx->stream) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            pq_release(ctx);
            set_error("panoptic_quality: could not set up %zu bytes of scratch", (size_t)kPqMatrixCells * sizeof(int) + (kPqRing + 1) * table);
            return ODISE_ERR_NOMEM;
        }
    }
    *out = (PqScratch*)ctx->pq;
    return ODISE_OK;
}

// everything that can be refused is refused before anything is enqueued
int pq_check_args(const odise_pq_desc* d) {
    ODISE_REQUIRE(d, "panoptic_quality: null descriptor");
    ODISE_REQUIRE(d->pred_ids && d->pred_segments && d->gt && d->stats && d->flags, "panoptic_quality: null pointer");
    ODISE_REQUIRE(d->H >= 1 && d->W >= 1 && (int64_t)d->H * d->W <= INT32_MAX / 4, "panoptic_quality: bad size %dx%d", d->H, d->W);
    ODISE_REQUIRE(d->gt_layout == 0 || d->gt_layout == 1, "panoptic_quality: gt_layout %d (0 = uint8 RGB, 1 = int32 ids)", d->gt_layout);
    ODISE_REQUIRE(d->num_categories >= 1, "panoptic_quality: num_categories %d", d->num_categories);
    ODISE_REQUIRE(d->n_gt >= 0 && d->n_gt <= kPqMaxGt, "panoptic_quality: %d ground-truth segments (at most %d)", d->n_gt, kPqMaxGt);
    ODISE_REQUIRE(d->n_gt == 0 || d->gt_segments, "panoptic_quality: null ground-truth table");
    ODISE_REQUIRE(((uintptr_t)d->pred_ids & 3) == 0 && ((uintptr_t)d->pred_segments & 3) == 0 && (d->gt_layout == 0 || ((uintptr_t)d->gt & 3) == 0),
                  "panoptic_quality: int32 buffers must be 4-byte aligned");
    for (int i = 0; i < d->n_gt; ++i) {
        const int32_t* r = d->gt_segments + 4 * i;
        ODISE_REQUIRE(r[1] >= 0 && r[1] < d->num_categories, "panoptic_quality: ground-truth row %d has category %d outside [0, %d)", i, r[1],
                      d->num_categories);
        ODISE_REQUIRE(r[2] == 0 || r[2] == 1, "panoptic_quality: ground-truth row %d has iscrowd %d", i, r[2]);
    }
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_panoptic_quality(odise_hip_ctx* ctx, const odise_pq_desc* d) {
    ODISE_REQUIRE(ctx, "panoptic_quality: null context");
    ODISE_TRY(pq_check_args(d));
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    PqScratch* s = nullptr;
    ODISE_TRY(pq_scratch(ctx, &s));
    if (d->n_gt) {   // the caller's table -> a pinned slot (free once the copy enqueued from it kernels ago has run) -> the device
        const int slot = s->next;
        s->next = (slot + 1) % kPqRing;
        ODISE_CHECK_HIP(hipEventSynchronize(s->ev[slot]));
        int* h = s->host + (size_t)slot * kPqMaxGt * 4;
        std::copy(d->gt_segments, d->gt_segments + 4 * d->n_gt, h);
        ODISE_CHECK_HIP(hipMemcpyAsync(s->gt_table, h, (size_t)d->n_gt * 4 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ODISE_CHECK_HIP(hipEventRecord(s->ev[slot], ctx->stream));
    }
    const int npix = d->H * d->W;
    const int vec = ((uintptr_t)d->pred_ids & 15) == 0 && ((uintptr_t)d->gt & (d->gt_layout == 0 ? 3 : 15)) == 0;
    const int lds_cells = std::min((d->n_gt + 2) * kPqPredSlots, kLdsHistCells);   // n is read on the device: room for the most it can be
    const int blocks = grid_blocks(ctx, ceil_div(npix, 4), 256);
    hipLaunchKernelGGL(pq_pixel_kernel, dim3(blocks), dim3(256), (size_t)lds_cells * sizeof(unsigned), ctx->stream, (const int*)d->pred_ids,
                       (const int*)d->pred_segments, d->gt, d->gt_layout, (const int*)s->gt_table, d->n_gt, npix, vec, lds_cells, s->matrix);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pq_match_kernel, dim3(1), dim3(kPqMatchThreads), 0, ctx->stream, s->matrix, (const int*)d->pred_segments,
                       (const int*)s->gt_table, d->n_gt, d->num_categories, d->stats, (int*)d->flags);
    const hipError_t launched = hipGetLastError();
    if (launched != hipSuccess) {   // the pixel pass may have counted and nothing will clear its counts: start the next call from new scratch
        pq_release(ctx);
        ODISE_CHECK_HIP(launched);
    }
    return ODISE_OK;
}
