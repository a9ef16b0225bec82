// pq.hip — panoptic quality statistics of one picture on the device (odise_hip_panoptic_quality), and Boundary PQ
// beside them (odise_hip_panoptic_quality_boundary, odise_hip_segment_boundaries).
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
//
// Boundary PQ (the rule: include/odise_hip.h) needs the boundary B(s) of every segment.  The segments of a panoptic map are disjoint, so
// no per-segment mask is made: the pixel pass also stores the slot bytes it has just computed (label_maps.h layout; gt slots reach 255,
// pred slots 101), and ONE erosion of the slot maps gives every boundary at once.  A pixel is off its boundary when its window is
// uniform, i.e. when the window's minimum AND maximum equal the pixel; the erosion kernel is a per-byte minimum with zeros outside, so
// the maximum is the minimum of the complement map 255 - slot, which the pixel pass writes beside the map: four maps per picture, eroded
// as grid.y = 4 of min_taps_kernel (eval_ops.hip).  A window that leaves the picture reads 0 in both and is not uniform for any slot
// that anyone reads.  Then:
//
//   pq_boundary_pairs_kernel  one sweep over the byte maps: (gslot', pslot') counted in the context's second matrix of
//                             (n_gt + 3) x (n + 3) cells, slot' = the slot for a VOID pixel (row 0 stays the VOID term) or a pixel on
//                             its boundary, else the one extra "off its boundary" slot of that side (n_gt + 2, n + 2).  Row sums give
//                             |B(g)|, column sums |B(p)|, row 0 |B(p) over VOID|.  The all-off cell - most pixels of a smooth map -
//                             is kept in a register.
//   pq_match_boundary_kernel  pq_match_kernel's passes twice over one load of the tables: with the mask IoU into `stats` (the same
//                             operations in the same order: bit-identical), with fmin(mask IoU, boundary IoU) into the boundary
//                             statistics.  Both matrices are left zeroed.
#include <algorithm>

#include "common.h"
#include "label_maps.h"
#include "lds_hist.h"
#include "record.h"
#include "rgb.h"

namespace odise {

constexpr int kPqMaxGt = 254;                               // ground-truth rows per picture
constexpr int kPqGtSlots = kPqMaxGt + 2;                    // + VOID + "not in the table"
constexpr int kPqPredSlots = ODISE_MAX_SEGMENTS + 2;
constexpr int kPqMatrixCells = kPqGtSlots * kPqPredSlots;   // the context's matrix holds the caps; a picture uses (n_gt + 2) x (n + 2) of it
constexpr int kPqBoundaryCells = (kPqGtSlots + 1) * (kPqPredSlots + 1);   // the second matrix: one "off its boundary" slot more per side
constexpr int kPqRing = 8;                                  // pinned staging slots of the ground-truth table (calls in flight before the host waits)
constexpr int kPqMatchThreads = 512;

struct PqScratch {
    int* matrix = nullptr;      // device [kPqMatrixCells], zero between calls
    int* bmatrix = nullptr;     // device [kPqBoundaryCells], zero between calls (Boundary PQ)
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

struct PqSlots { int g, p; };   // the two slots of a pixel

template <bool LDS>
__device__ __forceinline__ PqSlots pq_count(PqLane& L, int gid, int pid, const PqTables& T, const LdsHist<int>& H) {
    const int gslot = record_memo(L.gt, gid, [&](int id) { return pq_find_slot(T.gt_ids, T.n_gt, id); });
    const int pslot = record_memo(L.pred, pid, [&](int id) { return pq_find_slot(T.pred_ids, T.n, id); });
    L.pair.count<LDS>(gslot * (T.n + 2) + pslot, H);   // < (n_gt + 2) * (n + 2) <= kPqMatrixCells
    return {gslot, pslot};
}

// The slot maps of Boundary PQ: map k of `maps` = [gt slots, pred slots, 255 - gt slots, 255 - pred slots][k], per_map dwords each.
struct PqMaps {
    LabelGrid G;
    int64_t per_map;
    unsigned* maps;
};
// byte `at` (= y * 4 Pd + x, store_label's address) of the four maps
__device__ __forceinline__ void pq_store_at(const PqMaps& M, int64_t at, PqSlots s) {
    uint8_t* m = (uint8_t*)M.maps;
    m[at] = (uint8_t)s.g;
    m[4 * M.per_map + at] = (uint8_t)s.p;
    m[8 * M.per_map + at] = (uint8_t)(255 - s.g);
    m[12 * M.per_map + at] = (uint8_t)(255 - s.p);
}
__device__ __forceinline__ void pq_store_pixel(const PqMaps& M, int64_t p, PqSlots s) {
    const int y = (int)(p / M.G.W), x = (int)(p - (int64_t)y * M.G.W);
    pq_store_at(M, (int64_t)y * M.G.Pd * 4 + x, s);
}
// pixels 4 q .. 4 q + 3: with W a multiple of 4 they are dword q of a map (rows have no padding), else four byte stores per map behind
// one division for the group
__device__ __forceinline__ void pq_store_group(const PqMaps& M, int64_t q, const PqSlots (&s)[4]) {
    if ((M.G.W & 3) == 0) {
        const unsigned g = (unsigned)s[0].g | ((unsigned)s[1].g << 8) | ((unsigned)s[2].g << 16) | ((unsigned)s[3].g << 24);
        const unsigned p = (unsigned)s[0].p | ((unsigned)s[1].p << 8) | ((unsigned)s[2].p << 16) | ((unsigned)s[3].p << 24);
        M.maps[q] = g;
        M.maps[M.per_map + q] = p;
        M.maps[2 * M.per_map + q] = ~g;
        M.maps[3 * M.per_map + q] = ~p;
    } else {
        int y = (int)(4 * q / M.G.W), x = (int)(4 * q - (int64_t)y * M.G.W);
        for (int j = 0; j < 4; ++j) {
            pq_store_at(M, (int64_t)y * M.G.Pd * 4 + x, s[j]);
            if (++x == M.G.W) { x = 0; ++y; }   // 4 q + 3 < npix: y stays below H
        }
    }
}

// the pixels of the block, and the runs the lanes still hold
template <bool LDS, bool kMaps>
__device__ __forceinline__ void pq_pixels(const int* __restrict__ pred, const void* __restrict__ gt, int gt_layout, int npix, int vec, const PqTables& T,
                                          const LdsHist<int>& H, const PqMaps& M) {
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
            PqSlots s[4];
            s[0] = pq_count<LDS>(L, (int)g[0], p.x, T, H);
            s[1] = pq_count<LDS>(L, (int)g[1], p.y, T, H);
            s[2] = pq_count<LDS>(L, (int)g[2], p.z, T, H);
            s[3] = pq_count<LDS>(L, (int)g[3], p.w, T, H);
            if (kMaps) pq_store_group(M, q, s);
        }
    }
    // pixel by pixel: everything when the buffers are not aligned, else the last npix & 3 pixels
    for (int64_t i = (vec ? (int64_t)groups * 4 : 0) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const PqSlots s = pq_count<LDS>(L, gt_layout == 0 ? (int)rgb_load(gt8 + 3 * i) : gt32[i], pred[i], T, H);
        if (kMaps) pq_store_pixel(M, i, s);
    }
    L.pair.flush<LDS>(H);
}

// matrix[(n_gt + 2) x (n + 2)] += pair counts of the picture.  vec != 0: pred 16-byte aligned and gt dword aligned (groups of 4 pixels are
// read whole); the last npix & 3 pixels and unaligned buffers are read pixel by pixel.  lds_cells = cells of the dynamic LDS histogram.
// kMaps: the slots are also kept as the four byte maps of M (Boundary PQ); M.G.H * M.G.W = npix.
template <bool kMaps>
__global__ void __launch_bounds__(256) pq_pixel_kernel(const int* __restrict__ pred, const int* __restrict__ pred_segments, const void* __restrict__ gt,
                                                      int gt_layout, const int* __restrict__ gt_table, int n_gt, int npix, int vec, int lds_cells,
                                                      int* __restrict__ matrix, PqMaps M) {
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
    if (H.lds) pq_pixels<true, kMaps>(pred, gt, gt_layout, npix, vec, T, H, M);
    else pq_pixels<false, kMaps>(pred, gt, gt_layout, npix, vec, T, H, M);
    __syncthreads();
    H.flush();
}

// ---- Boundary PQ: the boundary pixels of the slot maps ------------------------------------------------------------------------------------
// Per byte non-zero where the pixel's window is not uniform: m = four slots, em / ec = the eroded map and the eroded complement map.
__device__ __forceinline__ unsigned pq_on_boundary(unsigned m, unsigned em, unsigned ec) { return (m ^ em) | (~m ^ ec); }

template <bool LDS>
__device__ __forceinline__ unsigned pq_boundary_pixels(const unsigned* __restrict__ m, const unsigned* __restrict__ e, const LabelGrid& G, int n_gt, int n,
                                                       const LdsHist<int>& H) {
    const int64_t per_map = (int64_t)G.H * G.Pd;
    const int Wb = n + 3, off_g = n_gt + 2, off_p = n + 2, all_off = off_g * Wb + off_p;
    HistRun run;
    unsigned own_off = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * blockDim.x) {
        const int xd = (int)(i % G.Pd);
        const int nb = min(4, G.W - 4 * xd);   // the bytes past W hold nothing
        const unsigned mg = m[i], mp = m[per_map + i];
        const unsigned bg = pq_on_boundary(mg, e[i], e[2 * per_map + i]), bp = pq_on_boundary(mp, e[per_map + i], e[3 * per_map + i]);
        for (int j = 0; j < nb; ++j) {
            const int gs = (int)((mg >> (8 * j)) & 255u), ps = (int)((mp >> (8 * j)) & 255u);
            const int gb = (gs == 0 || ((bg >> (8 * j)) & 255u)) ? gs : off_g;
            const int pb = (ps == 0 || ((bp >> (8 * j)) & 255u)) ? ps : off_p;
            const int cell = gb * Wb + pb;
            if (cell == all_off) ++own_off;
            else run.count<LDS>(cell, H);   // a slot is at most rows + 1: below (n_gt + 3) * (n + 3); HistRun never counts past H.n
        }
    }
    run.flush<LDS>(H);
    return own_off;
}

// bmatrix[(n_gt + 3) x (n + 3)] += (gslot', pslot') of the picture; m, e = [4][H][Pd]: the maps of pq_pixel_kernel<true> and their erosions
__global__ void __launch_bounds__(256) pq_boundary_pairs_kernel(const unsigned* __restrict__ m, const unsigned* __restrict__ e, LabelGrid G,
                                                               const int* __restrict__ pred_segments, int n_gt, int lds_cells,
                                                               int* __restrict__ bmatrix) {
    __shared__ unsigned all_off;   // the cell of the pixels that lie on no boundary on either side
    const int n = record_rows(pred_segments);
    const int cells = (n_gt + 3) * (n + 3);
    const LdsHist<int> H(bmatrix, cells, cells <= lds_cells);
    H.clear();
    if (threadIdx.x == 0) all_off = 0;
    __syncthreads();
    const unsigned own = H.lds ? pq_boundary_pixels<true>(m, e, G, n_gt, n, H) : pq_boundary_pixels<false>(m, e, G, n_gt, n, H);
    if (own) atomicAdd(&all_off, own);
    __syncthreads();
    if (threadIdx.x == 0 && all_off) atomicAdd(&bmatrix[cells - 1], (int)all_off);
    H.flush();
}

// odise_hip_segment_boundaries, first half: maps[0] = the slots of ids in `table`, maps[1] = 255 - them
__global__ void __launch_bounds__(256) pq_slot_maps_kernel(const int* __restrict__ ids, const int* __restrict__ table, int n, LabelGrid G,
                                                          unsigned* __restrict__ maps) {
    __shared__ int tab[kPqMaxGt];
    for (int i = threadIdx.x; i < n; i += blockDim.x) tab[i] = table[i];
    __syncthreads();
    const int64_t npix = (int64_t)G.H * G.W, per_map = (int64_t)G.H * G.Pd;
    RecordMemo memo = {0, 0};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int slot = record_memo(memo, ids[p], [&](int id) { return pq_find_slot(tab, n, id); });
        store_label(maps, p, G, slot);
        store_label(maps + per_map, p, G, 255 - slot);
    }
}

// second half: boundary [H,W] = 1 where a pixel of a table row lies on its boundary, area[row] += those pixels; m, e = [2][H][Pd]
__global__ void __launch_bounds__(256) pq_unpack_boundaries_kernel(const unsigned* __restrict__ m, const unsigned* __restrict__ e, LabelGrid G, int n,
                                                                  uint8_t* __restrict__ boundary, unsigned long long* __restrict__ area) {
    const LdsHist<unsigned long long> H(area, n, area != nullptr);   // n <= 254 cells of the launch's dynamic LDS
    H.clear();
    H.sync();
    const int64_t per_map = (int64_t)G.H * G.Pd;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / G.Pd), xd = (int)(i - (int64_t)y * G.Pd);
        const int nb = min(4, G.W - 4 * xd);
        const unsigned mv = m[i], b = pq_on_boundary(mv, e[i], e[per_map + i]);
        for (int j = 0; j < nb; ++j) {
            const int s = (int)((mv >> (8 * j)) & 255u);
            const bool on = s >= 1 && s <= n && ((b >> (8 * j)) & 255u);
            boundary[(int64_t)y * G.W + 4 * xd + j] = on ? 1 : 0;
            if (on && H.lds) H.add_lds(s - 1, 1u);
        }
    }
    H.sync();
    H.flush();
}

// ---- matching -----------------------------------------------------------------------------------------------------------------------------
// intersection over union of a candidate pair, as the double division of the two integers; a union <= 0 (only a JSON area that disagrees
// with the map can produce one) matches nothing
__device__ __forceinline__ bool pq_pair_iou(int inter, int area_pred, int area_gt, int void_pred, double* iou) {
    const int64_t uni = (int64_t)area_pred + (int64_t)area_gt - inter - void_pred;
    if (uni <= 0) return false;
    *iou = (double)inter / (double)uni;
    return *iou > 0.5;
}

struct PqMatch {   // the block's view of the two tables and of the matching of one pass (LDS)
    int g_id[kPqMaxGt], g_cat[kPqMaxGt], g_crowd[kPqMaxGt], g_area[kPqMaxGt];
    int g_order[kPqMaxGt];   // rows by ascending (id, row)
    int g_cnt[kPqMaxGt];     // matches of a row
    double g_iou[kPqMaxGt];  // the IoU of its match when there is exactly one
    int p_id[ODISE_MAX_SEGMENTS], p_cat[ODISE_MAX_SEGMENTS], p_order[ODISE_MAX_SEGMENTS], p_matched[ODISE_MAX_SEGMENTS];
    int p_area[kPqPredSlots], p_void[kPqPredSlots];
    int bad;
};

// Whole block.  The tables, the predicted areas (column sums of matrix [(n_gt + 2) x (n + 2)]), the ascending-id orders -> the picture's flags.
__device__ __forceinline__ int pq_match_load(PqMatch& S, const int* __restrict__ matrix, const int* __restrict__ pred_segments,
                                             const int* __restrict__ gt_table, int n_gt, int n, int C) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int W = n + 2;
    if (tid == 0) S.bad = 0;
    for (int i = tid; i < n_gt; i += nt) {
        S.g_id[i] = gt_table[4 * i]; S.g_cat[i] = gt_table[4 * i + 1]; S.g_crowd[i] = gt_table[4 * i + 2]; S.g_area[i] = gt_table[4 * i + 3];
    }
    for (int i = tid; i < n; i += nt) { S.p_id[i] = record_id(pred_segments, i); S.p_cat[i] = record_category(pred_segments, i); }
    for (int p = tid; p < W; p += nt) {               // pred areas = column sums
        int a = 0;
        for (int g = 0; g < n_gt + 2; ++g) a += matrix[g * W + p];
        S.p_area[p] = a;
        S.p_void[p] = matrix[p];
    }
    __syncthreads();
    int f = 0;
    if (tid == 0 && S.p_area[n + 1] > 0) f |= 1;                                   // an id of the map is missing from the table
    for (int i = tid; i < n; i += nt) {
        if (S.p_area[1 + i] == 0) f |= 2;                                          // a row without a pixel (also: a second row of an id, id 0)
        if ((unsigned)S.p_cat[i] >= (unsigned)C) f |= 4;
    }
    if (f) atomicOr(&S.bad, f);
    // ascending-id orders (unsorted tables; the rank of a row = rows with a smaller (id, row))
    for (int i = tid; i < n_gt; i += nt) {
        int r = 0;
        for (int j = 0; j < n_gt; ++j) r += (S.g_id[j] < S.g_id[i] || (S.g_id[j] == S.g_id[i] && j < i)) ? 1 : 0;
        S.g_order[r] = i;
    }
    for (int i = tid; i < n; i += nt) {
        int r = 0;
        for (int j = 0; j < n; ++j) r += (S.p_id[j] < S.p_id[i] || (S.p_id[j] == S.p_id[i] && j < i)) ? 1 : 0;
        S.p_order[r] = i;
    }
    __syncthreads();
    return S.bad;
}

// Whole block; ends on a barrier.  One matching of the picture added to `stats`: match(g, p, &iou) = rows g and p hold a matching pair.
template <class Match>
__device__ __forceinline__ void pq_match_add(PqMatch& S, const int* __restrict__ matrix, int n_gt, int n, const Match& match,
                                             odise_pq_stat* __restrict__ stats) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int W = n + 2;
    for (int i = tid; i < n_gt; i += nt) { S.g_cnt[i] = 0; S.g_iou[i] = 0.0; }
    for (int i = tid; i < n; i += nt) S.p_matched[i] = 0;
    __syncthreads();
    // candidates: both ids in their tables, pixels in common, not a crowd row, equal categories
    for (int i = tid; i < n_gt * n; i += nt) {
        const int g = i / n, p = i - g * n;
        if (S.g_crowd[g] || S.g_cat[g] != S.p_cat[p]) continue;
        double iou;
        if (!match(g, p, &iou)) continue;
        S.p_matched[p] = 1;
        if (atomicAdd(&S.g_cnt[g], 1) == 0) S.g_iou[g] = iou;   // read back only when the row has exactly one match
    }
    __syncthreads();
    // the ordered sums: the first matched row of a category in ascending id order adds all matches of that category, in order
    for (int r = tid; r < n_gt; r += nt) {
        const int g = S.g_order[r];
        if (!S.g_cnt[g]) continue;
        const int cat = S.g_cat[g];
        bool leader = true;
        for (int q = 0; q < r && leader; ++q) leader = !(S.g_cnt[S.g_order[q]] && S.g_cat[S.g_order[q]] == cat);
        if (!leader) continue;
        double sum = stats[cat].iou;
        int64_t tp = 0;
        for (int q = r; q < n_gt; ++q) {
            const int h = S.g_order[q];
            if (!S.g_cnt[h] || S.g_cat[h] != cat) continue;
            tp += S.g_cnt[h];
            if (S.g_cnt[h] == 1) { sum += S.g_iou[h]; continue; }
            for (int k = 0; k < n; ++k) {              // several matches (a JSON area that disagrees with the map): again, in pred-id order
                const int p = S.p_order[k];
                if (S.p_cat[p] != cat) continue;
                double iou;
                if (match(h, p, &iou)) sum += iou;
            }
        }
        stats[cat].iou = sum;
        stats[cat].tp += tp;
    }
    // false negatives: unmatched rows that are no crowd rows, with or without pixels
    for (int g = tid; g < n_gt; g += nt)
        if (!S.g_cnt[g] && !S.g_crowd[g]) atomicAdd((unsigned long long*)&stats[S.g_cat[g]].fn, 1ull);
    // false positives: unmatched predictions that do not lie mostly in VOID plus the (last) crowd row of their category
    for (int p = tid; p < n; p += nt) {
        if (S.p_matched[p]) continue;
        int crowd = -1;
        for (int g = 0; g < n_gt; ++g)
            if (S.g_crowd[g] && S.g_cat[g] == S.p_cat[p]) crowd = g;
        int64_t ign = S.p_void[p + 1];
        if (crowd >= 0) ign += matrix[(crowd + 1) * W + p + 1];
        if ((double)ign / (double)S.p_area[p + 1] > 0.5) continue;
        atomicAdd((unsigned long long*)&stats[S.p_cat[p]].fp, 1ull);
    }
    __syncthreads();
}

struct PqMaskMatch {   // PQ: pixels in common and a mask IoU above one half
    const PqMatch& S;
    const int* matrix;
    int W;
    __device__ __forceinline__ bool operator()(int g, int p, double* iou) const {
        const int inter = matrix[(g + 1) * W + p + 1];
        return inter > 0 && pq_pair_iou(inter, S.p_area[p + 1], S.g_area[g], S.p_void[p + 1], iou);
    }
};

struct PqBoundaryMatch {   // Boundary PQ: fmin(that IoU, the IoU of the two boundaries) above one half
    PqMaskMatch mask;
    const int* bmatrix;    // [(n_gt + 3) x Wb]
    int Wb;
    const int *bg_area, *bp_area, *bp_void;   // |B(g)| by row, |B(p)| and |B(p) over VOID| by pred slot
    __device__ __forceinline__ bool operator()(int g, int p, double* iou) const {
        double m;
        if (!mask(g, p, &m)) return false;   // fmin(m, b) <= m
        const int inter = bmatrix[(g + 1) * Wb + p + 1];
        const int64_t uni = (int64_t)bp_area[p + 1] + (int64_t)bg_area[g] - inter - bp_void[p + 1];
        const double b = uni > 0 ? (double)inter / (double)uni : 0.0;
        *iou = fmin(m, b);
        return *iou > 0.5;
    }
};

// One block.  matrix [(n_gt + 2) x (n + 2)] pair counts of the picture (slot 0 = VOID, last slot = not in the table); zeroed on return.
__global__ void __launch_bounds__(kPqMatchThreads) pq_match_kernel(int* __restrict__ matrix, const int* __restrict__ pred_segments,
                                                                  const int* __restrict__ gt_table, int n_gt, int C,
                                                                  odise_pq_stat* __restrict__ stats, int* __restrict__ flags) {
    __shared__ PqMatch S;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = record_rows(pred_segments);
    const int cells = (n_gt + 2) * (n + 2);
    const int bad = pq_match_load(S, matrix, pred_segments, gt_table, n_gt, n, C);
    if (bad) {                                         // the picture counts nothing
        if (tid == 0) flags[0] |= bad;
    } else {
        pq_match_add(S, matrix, n_gt, n, PqMaskMatch{S, matrix, n + 2}, stats);
    }
    for (int i = tid; i < cells; i += nt) matrix[i] = 0;
}

// One block.  The same, and bmatrix [(n_gt + 3) x (n + 3)] of pq_boundary_pairs_kernel -> bstats; both matrices zeroed on return.
__global__ void __launch_bounds__(kPqMatchThreads) pq_match_boundary_kernel(int* __restrict__ matrix, int* __restrict__ bmatrix,
                                                                           const int* __restrict__ pred_segments, const int* __restrict__ gt_table,
                                                                           int n_gt, int C, odise_pq_stat* __restrict__ stats,
                                                                           odise_pq_stat* __restrict__ bstats, int* __restrict__ flags) {
    __shared__ PqMatch S;
    __shared__ int bg_area[kPqMaxGt], bp_area[kPqPredSlots], bp_void[kPqPredSlots];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n = record_rows(pred_segments);
    const int cells = (n_gt + 2) * (n + 2), Wb = n + 3, bcells = (n_gt + 3) * Wb;
    const int bad = pq_match_load(S, matrix, pred_segments, gt_table, n_gt, n, C);
    if (bad) {
        if (tid == 0) flags[0] |= bad;
    } else {
        for (int g = tid; g < n_gt; g += nt) {         // |B(g)| = row sums
            int a = 0;
            for (int p = 0; p < Wb; ++p) a += bmatrix[(g + 1) * Wb + p];
            bg_area[g] = a;
        }
        for (int p = tid; p < n + 2; p += nt) {        // |B(p)| = column sums
            int a = 0;
            for (int g = 0; g < n_gt + 3; ++g) a += bmatrix[g * Wb + p];
            bp_area[p] = a;
            bp_void[p] = bmatrix[p];
        }
        const PqMaskMatch mask = {S, matrix, n + 2};
        pq_match_add(S, matrix, n_gt, n, mask, stats);   // its first barrier publishes the boundary areas as well
        pq_match_add(S, matrix, n_gt, n, PqBoundaryMatch{mask, bmatrix, Wb, bg_area, bp_area, bp_void}, bstats);
    }
    for (int i = tid; i < cells; i += nt) matrix[i] = 0;
    for (int i = tid; i < bcells; i += nt) bmatrix[i] = 0;
}

void pq_release(odise_hip_ctx* ctx) {
    PqScratch* s = (PqScratch*)ctx->pq;
    if (!s) return;
    if (s->matrix) (void)hipFree(s->matrix);
    if (s->bmatrix) (void)hipFree(s->bmatrix);
    if (s->gt_table) (void)hipFree(s->gt_table);
    if (s->host) (void)hipHostFree(s->host);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
    ctx->pq = nullptr;
}

// The scratch is published in the context only when all of it exists and the matrices are zeroed; a failure on the way releases what was
// made, so a later call starts over and never counts into a matrix that was not cleared.
static int pq_scratch(odise_hip_ctx* ctx, PqScratch** out) {
    if (!ctx->pq) {
        PqScratch* s = new PqScratch();
        ctx->pq = s;   // pq_release works on the context
        const size_t table = (size_t)kPqMaxGt * 4 * sizeof(int);
        const size_t matrices = (size_t)(kPqMatrixCells + kPqBoundaryCells) * sizeof(int);
        bool ok = hipMalloc((void**)&s->matrix, (size_t)kPqMatrixCells * sizeof(int)) == hipSuccess &&
                  hipMalloc((void**)&s->bmatrix, (size_t)kPqBoundaryCells * sizeof(int)) == hipSuccess &&
                  hipMalloc((void**)&s->gt_table, table) == hipSuccess &&
                  hipHostMalloc((void**)&s->host, kPqRing * table, hipHostMallocDefault) == hipSuccess;
        for (hipEvent_t& e : s->ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipMemsetAsync(s->matrix, 0, (size_t)kPqMatrixCells * sizeof(int), ctx->stream) == hipSuccess &&
             hipMemsetAsync(s->bmatrix, 0, (size_t)kPqBoundaryCells * sizeof(int), ctx->stream) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            pq_release(ctx);
            set_error("panoptic_quality: could not set up %zu bytes of scratch", matrices + (kPqRing + 1) * table);
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

// the launches of one picture; b = the Boundary PQ task or null.  *counted: the pixel pass was launched - a failure after that leaves
// counts that nothing will clear, and the caller releases the scratch.
static int pq_enqueue(odise_hip_ctx* ctx, const odise_pq_desc* d, const odise_pq_boundary_task* b, PqScratch* s, BoundaryMaps* bm, bool* counted) {
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
    const PqMaps M = b ? PqMaps{bm->G, bm->per_map, bm->m} : PqMaps{};
    const auto pixel_kernel = b ? pq_pixel_kernel<true> : pq_pixel_kernel<false>;
    hipLaunchKernelGGL(pixel_kernel, dim3(blocks), dim3(256), (size_t)lds_cells * sizeof(unsigned), ctx->stream, (const int*)d->pred_ids, (const int*)d->pred_segments, d->gt, d->gt_layout, (const int*)s->gt_table, d->n_gt, npix, vec, lds_cells,
                       s->matrix, M);
    ODISE_CHECK_HIP(hipGetLastError());
    *counted = true;
    if (!b) {
        hipLaunchKernelGGL(pq_match_kernel, dim3(1), dim3(kPqMatchThreads), 0, ctx->stream, s->matrix, (const int*)d->pred_segments,
                           (const int*)s->gt_table, d->n_gt, d->num_categories, d->stats, (int*)d->flags);
        ODISE_CHECK_HIP(hipGetLastError());
        return ODISE_OK;
    }
    ODISE_TRY(erode_maps(ctx, bm, 4, b->radius > 0 ? b->radius : boundary_radius(d->H, d->W)));
    const int b_lds_cells = std::min((d->n_gt + 3) * (kPqPredSlots + 1), kLdsHistCells);
    hipLaunchKernelGGL(pq_boundary_pairs_kernel, dim3(grid_blocks(ctx, bm->per_map, 256)), dim3(256), (size_t)b_lds_cells * sizeof(unsigned), ctx->stream,
                       (const unsigned*)bm->m, (const unsigned*)bm->e, bm->G, (const int*)d->pred_segments, d->n_gt, b_lds_cells, s->bmatrix);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pq_match_boundary_kernel, dim3(1), dim3(kPqMatchThreads), 0, ctx->stream, s->matrix, s->bmatrix, (const int*)d->pred_segments,
                       (const int*)s->gt_table, d->n_gt, d->num_categories, d->stats, b->stats, (int*)d->flags);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

static int pq_run(odise_hip_ctx* ctx, const odise_pq_desc* d, const odise_pq_boundary_task* b) {
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    PqScratch* s = nullptr;
    ODISE_TRY(pq_scratch(ctx, &s));
    BoundaryMaps bm{};
    if (b) ODISE_TRY(boundary_maps(ctx, d->H, d->W, 4, &bm));
    bool counted = false;
    const int rc = pq_enqueue(ctx, d, b, s, &bm, &counted);
    if (rc != ODISE_OK && counted) pq_release(ctx);   // the pixel pass may have counted and nothing will clear its counts: start the next call from new scratch
    return rc;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_sizeof_pq_boundary_task(void) { return (int)sizeof(odise_pq_boundary_task); }

extern "C" int odise_hip_panoptic_quality(odise_hip_ctx* ctx, const odise_pq_desc* d) {
    ODISE_REQUIRE(ctx, "panoptic_quality: null context");
    ODISE_TRY(pq_check_args(d));
    return pq_run(ctx, d, nullptr);
}

extern "C" int odise_hip_panoptic_quality_boundary(odise_hip_ctx* ctx, const odise_pq_desc* d, const odise_pq_boundary_task* b) {
    ODISE_REQUIRE(ctx, "panoptic_quality_boundary: null context");
    ODISE_TRY(pq_check_args(d));
    ODISE_REQUIRE(b && b->stats, "panoptic_quality_boundary: null boundary task or statistics");
    ODISE_REQUIRE(((uintptr_t)b->stats & 7) == 0, "panoptic_quality_boundary: the boundary statistics must be 8-byte aligned");
    ODISE_REQUIRE(b->stats + d->num_categories <= d->stats || d->stats + d->num_categories <= b->stats,
                  "panoptic_quality_boundary: the boundary statistics overlap the statistics");
    return pq_run(ctx, d, b);
}

extern "C" int odise_hip_segment_boundaries(odise_hip_ctx* ctx, const int32_t* ids, int H, int W, const int32_t* table, int n, int radius,
                                            uint8_t* boundary, int64_t* area) {
    ODISE_REQUIRE(ctx && ids && boundary, "segment_boundaries: null argument");
    ODISE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX / 4, "segment_boundaries: bad size %dx%d", H, W);
    ODISE_REQUIRE(n >= 0 && n <= kPqMaxGt && (n == 0 || table), "segment_boundaries: a table of %d ids (at most %d)", n, kPqMaxGt);
    ODISE_REQUIRE((((uintptr_t)ids | (uintptr_t)table) & 3) == 0 && ((uintptr_t)area & 7) == 0,
                  "segment_boundaries: int32 buffers must be 4-byte aligned, area 8-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    BoundaryMaps bm;
    ODISE_TRY(boundary_maps(ctx, H, W, 2, &bm));
    if (area && n) ODISE_CHECK_HIP(hipMemsetAsync(area, 0, (size_t)n * sizeof(int64_t), ctx->stream));
    hipLaunchKernelGGL(pq_slot_maps_kernel, dim3(grid_blocks(ctx, (int64_t)H * W, 256)), dim3(256), 0, ctx->stream, (const int*)ids, (const int*)table, n,
                       bm.G, bm.m);
    ODISE_CHECK_HIP(hipGetLastError());
    ODISE_TRY(erode_maps(ctx, &bm, 2, radius > 0 ? radius : boundary_radius(H, W)));
    hipLaunchKernelGGL(pq_unpack_boundaries_kernel, dim3(grid_blocks(ctx, bm.per_map, 256)), dim3(256), lds_hist_bytes(n), ctx->stream,
                       (const unsigned*)bm.m, (const unsigned*)bm.e, bm.G, n, boundary, (unsigned long long*)area);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
