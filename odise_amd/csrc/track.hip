// track.hip — a thing keeps its colour from frame to frame (odise_hip_track_*; detectron2 VideoVisualizer._assign_colors, mask-IoU path).
//
// The tracker owns a ring of kTrackRing byte maps (0 = no instance, 1 + table row of the frame's record), the live list (at most
// kTrackRing x ODISE_MAX_SEGMENTS rows: a row can only come from the last ttl <= 8 frames) and a pair-count matrix that is zero between
// calls.  Two launches per frame, no synchronisation (host restatement: odise_amd/video.py):
//
//   track_pixel_kernel   one sweep over the pixels.  Four pixels per lane and step: the new map as one 16-byte load, every retained map
//                        that still has a live row as one dword.  The new ids become 1 + table row through the table held in LDS (a lane
//                        keeps its last translation).  One (rows_old + 1) x (n + 1) matrix per retained map, laid end to end, is counted in
//                        the per-block histogram (lds_hist.h); a lane counts a run of equal pairs per map in a register.  The new byte map
//                        goes where the oldest lay: a pixel's old byte is read by the lane that overwrites it, before it does.
//   track_match_kernel   one block, a thread per live row: new areas (column sums), the first-maximum arg-max of every live row, the
//                        winner of a new instance = the smallest list position among the rows that chose it (atomicMin in LDS), colours,
//                        then the list compacted by a block scan behind the new instances, and the matrix zeroed again.
#include <algorithm>

#include "common.h"
#include "lds_hist.h"
#include "record.h"
#include "rgb.h"
#include "track_match.h"
#include "vis_scan.h"

namespace odise {

// kTrackRing (retained frames = the largest ttl), kTrackLiveCap and kTrackMatchThreads: track_match.h
constexpr int kTrackSlots = ODISE_MAX_SEGMENTS + 1;                      // 0 = no instance, 1 + table row
constexpr int kTrackMatrixCells = kTrackRing * kTrackSlots * kTrackSlots;

struct TrackState {   // device
    int frame, counter, n_live, pad;         // frames since the reset, pool counter (kept modulo n_pool), rows of `live`
    int slot_rows[kTrackRing];               // table rows of the frame a ring slot holds
    odise_track_row live[kTrackLiveCap];
    int live_row[kTrackLiveCap];             // table row of a live instance in its own frame: its byte in that frame's map, minus one
};

}  // namespace odise

struct odise_track {
    int H = 0, W = 0;
    int64_t map_stride = 0;                  // bytes between ring maps (npix rounded up to 16)
    odise::TrackState* state = nullptr;
    uint8_t* maps = nullptr;                 // [kTrackRing][map_stride]
    int* matrix = nullptr;                   // [kTrackMatrixCells], zero between calls
    odise::TrackPool pool;
};

namespace odise {

// The matrices of a frame: one per retained map that still has a live row, (rows + 1) x (n + 1) cells each, laid end to end; with no live
// row at all a single 1 x (n + 1) matrix without a map (the new areas are column sums of the first matrix).
struct TrackLayout {
    int n, passes, cells;
    int slot[kTrackRing];      // ring slot of a pass, -1 = no map
    int off[kTrackRing];       // first cell of its matrix
    int pass_of[kTrackRing];   // ring slot -> pass, -1 = not retained
};

// tab[i] = id of table row i when the row can be an instance (a thing, id > 0, the first row of its id), else 0.  Whole block; no barrier.
__device__ __forceinline__ void track_load_table(const int* __restrict__ seg, int n, int* tab) {
    record_load(seg, n, tab, nullptr, kRecordIsThing, [seg](int i, int id) {
        bool first = id > 0 && record_isthing(seg, i) != 0;
        for (int r = 0; r < i && first; ++r) first = record_id(seg, r) != id;
        return first ? id : 0;
    });
}

// Whole block: `active` is scratch, `L` the result; both are published by the barriers in here.
__device__ __forceinline__ void track_layout(const TrackState* __restrict__ st, int n, int* active, TrackLayout* L) {
    if (threadIdx.x < kTrackRing) active[threadIdx.x] = 0;
    __syncthreads();
    const int n_live = track_clamp(st->n_live, kTrackLiveCap);
    for (int r = threadIdx.x; r < n_live; r += blockDim.x) active[st->live[r].frame & (kTrackRing - 1)] = 1;
    __syncthreads();
    if (threadIdx.x == 0) {
        int passes = 0, cells = 0;
        for (int s = 0; s < kTrackRing; ++s) {
            L->pass_of[s] = -1;
            if (!active[s]) continue;
            L->pass_of[s] = passes;
            L->slot[passes] = s;
            L->off[passes] = cells;
            cells += (track_clamp(st->slot_rows[s], ODISE_MAX_SEGMENTS) + 1) * (n + 1);
            ++passes;
        }
        if (!passes) { L->slot[0] = -1; L->off[0] = 0; cells = n + 1; passes = 1; }
        for (int k = passes; k < kTrackRing; ++k) { L->slot[k] = -1; L->off[k] = 0; }
        L->n = n; L->passes = passes; L->cells = cells;   // <= kTrackRing * kTrackSlots * kTrackSlots
    }
    __syncthreads();
}

// 1 + the row of the filtered table that holds `id`; 0 = no instance (id <= 0, or no such row)
__device__ __forceinline__ int track_find(const int* tab, int n, int id) { return id <= 0 ? 0 : record_find(tab, n, id) + 1; }

struct TrackLane {
    RecordMemo last;             // the lane's last translation
    HistRun pair[kTrackRing];    // per pass: the pair being counted and its length so far (registers: the loops are unrolled)
};

__device__ __forceinline__ int track_translate(TrackLane& T, const int* tab, int n, int id) {
    return record_memo(T.last, id, [&](int v) { return track_find(tab, n, v); });
}

// four pixels of group q (bytes 4 q .. 4 q + 3 of every map; the maps are 16-byte aligned)
template <bool LDS>
__device__ __forceinline__ void track_group(TrackLane& T, const TrackLayout& L, uint8_t* maps, int64_t map_stride, int new_slot, int64_t q,
                                            int j0, int j1, int j2, int j3, const LdsHist<int>& H) {
    const int w = L.n + 1;
#pragma unroll
    for (int k = 0; k < kTrackRing; ++k) {
        if (k >= L.passes) break;
        const int s = L.slot[k];
        const unsigned o = s >= 0 ? ((const unsigned*)(maps + (int64_t)s * map_stride))[q] : 0u;
        const int base = L.off[k];
        const int o0 = (int)(o & 255u), o1 = (int)((o >> 8) & 255u), o2 = (int)((o >> 16) & 255u), o3 = (int)(o >> 24);
        if (o0 | j0) T.pair[k].count<LDS>(base + o0 * w + j0, H);   // the (nothing, nothing) pair is not needed
        if (o1 | j1) T.pair[k].count<LDS>(base + o1 * w + j1, H);
        if (o2 | j2) T.pair[k].count<LDS>(base + o2 * w + j2, H);
        if (o3 | j3) T.pair[k].count<LDS>(base + o3 * w + j3, H);
    }
    ((unsigned*)(maps + (int64_t)new_slot * map_stride))[q] = (unsigned)j0 | ((unsigned)j1 << 8) | ((unsigned)j2 << 16) | ((unsigned)j3 << 24);
}

template <bool LDS>
__device__ __forceinline__ void track_pixel(TrackLane& T, const TrackLayout& L, uint8_t* maps, int64_t map_stride, int new_slot, int64_t i, int j,
                                            const LdsHist<int>& H) {
    const int w = L.n + 1;
#pragma unroll
    for (int k = 0; k < kTrackRing; ++k) {
        if (k >= L.passes) break;
        const int s = L.slot[k];
        const int o = s >= 0 ? (int)maps[(int64_t)s * map_stride + i] : 0;
        if (o | j) T.pair[k].count<LDS>(L.off[k] + o * w + j, H);
    }
    maps[(int64_t)new_slot * map_stride + i] = (uint8_t)j;
}

// the pixels of the block, and the runs the lanes still hold
template <bool LDS>
__device__ __forceinline__ void track_pixels(const int* __restrict__ pred, const int* tab, int n, const TrackLayout& L, uint8_t* maps, int64_t map_stride,
                                             int new_slot, int npix, int vec, const LdsHist<int>& H) {
    TrackLane T = {{0, 0}, {}};   // VOID is no instance
    const int groups = npix >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
            const int4 p = ((const int4*)pred)[q];
            const int j0 = track_translate(T, tab, n, p.x), j1 = track_translate(T, tab, n, p.y);
            const int j2 = track_translate(T, tab, n, p.z), j3 = track_translate(T, tab, n, p.w);
            track_group<LDS>(T, L, maps, map_stride, new_slot, q, j0, j1, j2, j3, H);
        }
    }
    for (int64_t i = (vec ? (int64_t)groups * 4 : 0) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride)
        track_pixel<LDS>(T, L, maps, map_stride, new_slot, i, track_translate(T, tab, n, pred[i]), H);
#pragma unroll
    for (int k = 0; k < kTrackRing; ++k) T.pair[k].flush<LDS>(H);
}

// matrix += the pair counts of the frame; maps[frame & 7] = the frame's byte map.  vec != 0: pred is 16-byte aligned (groups of four pixels
// are read whole; the last npix & 3 pixels and an unaligned map are read pixel by pixel).  lds_cells = cells of the dynamic LDS histogram.
// A pixel is read and written by one lane only, and its old bytes are read before its new byte is stored (maps is not __restrict__).
__global__ void __launch_bounds__(256) track_pixel_kernel(const int* __restrict__ pred, const int* __restrict__ pred_segments,
                                                         const TrackState* __restrict__ st, uint8_t* maps, int64_t map_stride, int npix, int vec,
                                                         int lds_cells, int* __restrict__ matrix) {
    __shared__ int tab[ODISE_MAX_SEGMENTS];
    __shared__ int active[kTrackRing];
    __shared__ TrackLayout L;
    const int n = record_rows(pred_segments);
    track_load_table(pred_segments, n, tab);
    track_layout(st, n, active, &L);
    const LdsHist<int> H(matrix, L.cells, L.cells <= lds_cells);
    H.clear();
    __syncthreads();
    const int new_slot = st->frame & (kTrackRing - 1);
    if (H.lds) track_pixels<true>(pred, tab, n, L, maps, map_stride, new_slot, npix, vec, H);
    else track_pixels<false>(pred, tab, n, L, maps, map_stride, new_slot, npix, vec, H);
    __syncthreads();
    H.flush();
}

// One block of kTrackMatchThreads.  matrix: the pair counts of the frame (zeroed on return); st: the tracker before the frame -> after it.
// The match, colour and compact step itself is track_match_block (track_match.h), shared with inst_track.hip.
__global__ void __launch_bounds__(kTrackMatchThreads) track_match_kernel(int* __restrict__ matrix, const int* __restrict__ pred_segments,
                                                                        TrackState* __restrict__ st, const uint8_t* __restrict__ pool, int n_pool,
                                                                        int ttl, uint8_t* __restrict__ colors, odise_track_row* __restrict__ live_out,
                                                                        int live_cap, int* __restrict__ n_live_out, double* __restrict__ iou_out,
                                                                        int iou_cap) {
    __shared__ int tab[ODISE_MAX_SEGMENTS], cat[ODISE_MAX_SEGMENTS], area[ODISE_MAX_SEGMENTS];
    __shared__ int active[kTrackRing];
    __shared__ TrackLayout L;
    const int tid = threadIdx.x;
    const int n = record_rows(pred_segments);
    const int n_live = track_clamp(st->n_live, kTrackLiveCap), frame = st->frame, counter = st->counter;
    track_load_table(pred_segments, n, tab);
    track_layout(st, n, active, &L);   // its barriers also order the reads of st->frame / n_live / counter above before anything is written
    const int w = n + 1;

    // the frame's instances: candidates that own a pixel (area = column sum of the first matrix, whose rows cover every pixel of the map)
    if (tid < n) {
        int a = 0;
        if (tab[tid]) {
            const int rows = L.slot[0] >= 0 ? track_clamp(st->slot_rows[L.slot[0]], ODISE_MAX_SEGMENTS) + 1 : 1;
            for (int o = 0; o < rows; ++o) a += matrix[L.off[0] + o * w + tid + 1];
        }
        area[tid] = a;
        cat[tid] = record_category(pred_segments, tid);
    }
    __syncthreads();
    const TrackMatchIo io = {pool, n_pool, ttl, colors, nullptr, live_out, live_cap, n_live_out, iou_out, iou_cap};
    // the cell of live row (frame, table row aux) and new row j; a row whose frame has no matrix shares no pixel
    const TrackMatched m = track_match_block(n, tab, cat, area, area, st->live, st->live_row, n_live, frame, counter, io, 0.5,
                                             [&](int, const odise_track_row& row, int aux, int j) {
                                                 const int k = L.pass_of[row.frame & (kTrackRing - 1)];
                                                 return track_count_iou(row.area, area[j], k < 0 ? 0 : matrix[L.off[k] + (aux + 1) * w + j + 1]);
                                             });
    if (tid == 0) {
        st->n_live = m.total;
        st->frame = frame + 1;
        st->counter = (counter + m.n_new) % n_pool;
        st->slot_rows[frame & (kTrackRing - 1)] = n;
    }
    for (int i = tid; i < L.cells; i += kTrackMatchThreads) matrix[i] = 0;
}

static void track_free(odise_track* t) {
    if (t->state) (void)hipFree(t->state);
    if (t->maps) (void)hipFree(t->maps);
    if (t->matrix) (void)hipFree(t->matrix);
    track_pool_free(&t->pool);
    delete t;
}

static int track_clear(odise_hip_ctx* ctx, odise_track* t) {
    ODISE_CHECK_HIP(hipMemsetAsync(t->state, 0, sizeof(TrackState), ctx->stream));
    ODISE_CHECK_HIP(hipMemsetAsync(t->matrix, 0, (size_t)kTrackMatrixCells * sizeof(int), ctx->stream));
    return ODISE_OK;
}

// everything that can be refused is refused before anything is enqueued
static int track_check_args(const odise_track_desc* d) {
    ODISE_REQUIRE(d, "track_frame: null descriptor");
    ODISE_REQUIRE(d->track && d->pred_ids && d->pred_segments && d->colors, "track_frame: null pointer");
    ODISE_TRY(vis_check_size("track_frame", d->H, d->W));
    ODISE_REQUIRE(d->H == d->track->H && d->W == d->track->W, "track_frame: a %dx%d frame for a tracker of %dx%d", d->H, d->W, d->track->H,
                  d->track->W);
    ODISE_TRY(track_check_dumps("track_frame", d));
    ODISE_REQUIRE((((uintptr_t)d->pred_ids | (uintptr_t)d->pred_segments) & 3) == 0, "track_frame: pred_ids / pred_segments must be 4-byte aligned");
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_track_create(odise_hip_ctx* ctx, int H, int W, int ttl, const uint8_t* pool_rgb, int n_pool, odise_track** out) {
    ODISE_REQUIRE(ctx, "track_create: null context");
    ODISE_REQUIRE(out && pool_rgb, "track_create: null pointer");
    ODISE_TRY(vis_check_size("track_create", H, W));
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    odise_track* t = new odise_track();
    t->H = H; t->W = W;
    t->map_stride = round_up((int64_t)H * W, 16);
    int rc = track_pool_create("track_create", ttl, pool_rgb, n_pool, &t->pool);
    if (rc == ODISE_OK) {
        const bool ok = hipMalloc((void**)&t->state, sizeof(TrackState)) == hipSuccess &&
                        hipMalloc((void**)&t->maps, (size_t)kTrackRing * t->map_stride) == hipSuccess &&
                        hipMalloc((void**)&t->matrix, (size_t)kTrackMatrixCells * sizeof(int)) == hipSuccess;
        if (!ok) rc = track_no_memory("track_create", sizeof(TrackState) + (size_t)kTrackRing * t->map_stride + (size_t)kTrackMatrixCells * sizeof(int));
    }
    return track_created(rc, ctx, t, out, track_clear, track_free);
}

extern "C" int odise_hip_track_reset(odise_hip_ctx* ctx, odise_track* track) { return track_reset("track_reset", ctx, track, track_clear); }

extern "C" int odise_hip_track_destroy(odise_hip_ctx* ctx, odise_track* track) { return track_destroy("track_destroy", ctx, track, track_free); }

extern "C" int odise_hip_track_frame(odise_hip_ctx* ctx, const odise_track_desc* d) {
    ODISE_REQUIRE(ctx, "track_frame: null context");
    ODISE_TRY(track_check_args(d));
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    odise_track* t = d->track;
    const int npix = d->H * d->W;
    const int vec = ((uintptr_t)d->pred_ids & 15) == 0;
    const int lds_cells = kLdsHistCells;   // the tables are read on the device: room for the most the histogram holds
    const int blocks = grid_blocks(ctx, ceil_div(npix, 4), 256);
    hipLaunchKernelGGL(track_pixel_kernel, dim3(blocks), dim3(256), lds_hist_bytes(lds_cells), ctx->stream, (const int*)d->pred_ids,
                       (const int*)d->pred_segments, (const TrackState*)t->state, t->maps, t->map_stride, npix, vec, lds_cells, t->matrix);
    ODISE_CHECK_HIP(hipGetLastError());
    // the kernel keeps its loose __restrict__ parameters: with the struct by value a frame measured 1.3 us longer (profiles/tracker_host_refactor.json)
    const TrackMatchIo io = track_match_io(t->pool, d);
    hipLaunchKernelGGL(track_match_kernel, dim3(1), dim3(kTrackMatchThreads), 0, ctx->stream, t->matrix, (const int*)d->pred_segments, t->state,
                       io.pool, io.n_pool, io.ttl, io.colors, io.live_out, io.live_cap, io.n_live_out, io.iou_out, io.iou_cap);
    return track_match_launched(ctx, t->matrix, (size_t)kTrackMatrixCells * sizeof(int));   // the pixel pass has counted
}
