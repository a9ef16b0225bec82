// inst_track.hip — overlapping instance masks keep their colours from frame to frame (odise_hip_inst_track_*; detectron2
// VideoVisualizer._assign_colors on box-less instances: the mask-IoU path).  Host restatement: odise_amd/video.py InstanceColorTracker.
//
// Instance masks overlap, so there is no label map to count pairs on (track.hip): the tracker retains the bit-packed words of rle_pack.h
// ([topk][w][R] per frame) in a ring of ttl + 1 slots - a row made in frame f is last matched against in frame f + ttl, and the new frame
// never lands in a slot a live row points to - and a live row finds its words through its (frame, id).  Four launches per frame, no
// synchronisation, no count read by the host:
//
//   pack                     inst_pack (inst_words.h) straight into the ring slot frame mod (ttl + 1)
//   inst_track_area_kernel   a block per table index: area = popcount of its words when the index is a candidate (inst_candidate, the rule
//                            of odise_hip_instance_draw: area > 0 is its `kept`), else 0, and its class
//   inst_track_inter_kernel  inter[live o][new j] += popcount(words_o & words_j), tiled like inst_inter_kernel (inst_eval.hip; the tile
//                            sizes and the split of the word axis are the ones of inst_words.h): 64 live rows x 32 new masks x 32 words
//                            in LDS, padded rows, a thread forms 4 x 2 pairs, the word axis split over blockIdx.z.
//                            The grid is sized for the caps (800 x topk): a tile past the live count or the table count
//                            leaves at once, and so does - decided once per tile, by the whole block - a tile in which no live row
//                            shares a class with a kept new mask.  Neither has loaded a word by then.  Integer atomics; pairs of
//                            different classes are not added (the matching never reads them).
//   inst_track_match_kernel  one block: track_match_block (track_match.h, shared with track.hip), then the matrix zeroed again
#include "inst_words.h"
#include "track_match.h"
#include "vis_scan.h"

namespace odise {

constexpr int kGatherBlocks = 2048;                                      // the grid's target size; most of it leaves at once

struct InstTrackState {   // device
    int counter, n_live, pad0, pad1;         // pool counter (kept modulo n_pool), rows of `live`
    odise_track_row live[kTrackLiveCap];     // id = table index in the row's own frame; its words: ring slot frame mod slots, mask id
};

}  // namespace odise

struct odise_inst_track {
    int H = 0, W = 0, topk = 0, slots = 0;
    int frame = 0;                           // frames since the reset, counted on the host: it chooses the slot the pack launch writes
    odise::RleGrid G = {};
    odise::InstTrackState* state = nullptr;
    odise::u64* ring = nullptr;              // [slots][topk][G.nw]
    int* inter = nullptr;                    // [kTrackLiveCap][topk], zero between calls
    int* area = nullptr;                     // [topk] areas (0 = not an instance of the frame) | [topk] classes
    odise::TrackPool pool;
};

namespace odise {

// words: the new frame's slot.  area[i] = pixels of mask i when i is an instance candidate (below the count, score >= min_score), else 0.
__global__ void __launch_bounds__(256) inst_track_area_kernel(const u64* __restrict__ words, int64_t nw, const int* __restrict__ table,
                                                             const float* __restrict__ scores, int topk, float min_score, int* __restrict__ area,
                                                             int* __restrict__ cls) {
    const int i = blockIdx.x;
    const bool cand = inst_candidate(table, scores, topk, min_score, i);
    const long long s = block_popcount(words + (int64_t)i * nw, cand ? nw : 0);
    if (threadIdx.x == 0) {
        area[i] = (int)s;   // at most h * w < 2^29
        cls[i] = (table && cand) ? table[1 + topk + i] : 0;
    }
}

// inter[o][j] += over the words [blockIdx.z * per, + per) of live row o and new mask j; `per` is a multiple of kInterKC
__global__ void __launch_bounds__(256) inst_track_inter_kernel(const u64* __restrict__ ring, const InstTrackState* __restrict__ st,
                                                              const int* __restrict__ table, const int* __restrict__ area,
                                                              const int* __restrict__ cls, int topk, int slots, int new_slot, int64_t nw, int64_t per,
                                                              int* __restrict__ inter) {
    __shared__ u64 sl[kInterRows][kInterKC + 1];
    __shared__ u64 sn[kInterCols][kInterKC + 1];
    __shared__ long long base[kInterRows + kInterCols];   // first word of a row's mask in the ring, -1 = no such row
    __shared__ int cat[kInterRows + kInterCols];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int o0 = blockIdx.x * kInterRows, j0 = blockIdx.y * kInterCols;
    const int n_live = track_clamp(st->n_live, kTrackLiveCap), n = inst_count(table, topk);
    if (o0 >= n_live || j0 >= n) return;   // block-uniform: nothing is loaded for a tile past either count
    if (tid < kInterRows) {
        long long b = -1;
        int c = 0;
        const int o = o0 + tid;
        if (o < n_live) {
            const int frame = st->live[o].frame, id = st->live[o].id;
            if (frame >= 0 && (unsigned)id < (unsigned)topk) {   // what the match step wrote; anything else addresses nothing
                b = ((long long)(frame % slots) * topk + id) * nw;
                c = st->live[o].category;
            }
        }
        base[tid] = b; cat[tid] = c;
    } else if (tid < kInterRows + kInterCols) {
        long long b = -1;
        int c = 0;
        const int j = j0 + tid - kInterRows;
        if (j < n && area[j] > 0) {
            b = ((long long)new_slot * topk + j) * nw;
            c = cls[j];
        }
        base[tid] = b; cat[tid] = c;
    }
    __syncthreads();
    bool pair[4][2];
    int any = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int a = ty + 16 * i, b = kInterRows + tx + 16 * j;
            pair[i][j] = base[a] >= 0 && base[b] >= 0 && cat[a] == cat[b];
            any |= pair[i][j] ? 1 : 0;
        }
    if (!__syncthreads_or(any)) return;    // no (live, new) pair of one class in the tile: decided once, before a word is loaded

    const int64_t k_begin = (int64_t)blockIdx.z * per, k_end = min(nw, k_begin + per);
    int acc[4][2] = {};
    for (int64_t k0 = k_begin; k0 < k_end; k0 += kInterKC) {
        for (int e = tid; e < (kInterRows + kInterCols) * kInterKC; e += 256) {
            const int row = e / kInterKC, kk = e - row * kInterKC;
            const int64_t k = k0 + kk;
            const long long b = base[row];
            const u64 v = (b >= 0 && k < k_end) ? ring[b + k] : 0ull;
            if (row < kInterRows) sl[row][kk] = v;
            else sn[row - kInterRows][kk] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kInterKC; ++kk) {
            const u64 b0 = sn[tx][kk], b1 = sn[tx + 16][kk];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u64 a = sl[ty + 16 * i][kk];
                acc[i][0] += __popcll(a & b0);
                acc[i][1] += __popcll(a & b1);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (pair[i][j] && acc[i][j]) atomicAdd(&inter[(int64_t)(o0 + ty + 16 * i) * topk + j0 + tx + 16 * j], acc[i][j]);
}

// One block of kTrackMatchThreads.  inter: the intersections of the frame (zeroed on return); st: the tracker before the frame -> after it.
__global__ void __launch_bounds__(kTrackMatchThreads) inst_track_match_kernel(int* __restrict__ inter, const int* __restrict__ table,
                                                                             const int* __restrict__ area_g, const int* __restrict__ cls_g,
                                                                             InstTrackState* __restrict__ st, int topk, int frame, TrackMatchIo io) {
    __shared__ int tab[ODISE_MAX_SEGMENTS], cat[ODISE_MAX_SEGMENTS], area[ODISE_MAX_SEGMENTS];
    const int tid = threadIdx.x;
    const int n = inst_count(table, topk);
    const int n_live = track_clamp(st->n_live, kTrackLiveCap), counter = st->counter;
    if (tid < n) {
        tab[tid] = tid;
        cat[tid] = cls_g[tid];
        area[tid] = area_g[tid];
    }
    __syncthreads();   // also: n_live and the counter are read before anything is written
    const TrackMatched m = track_match_block(n, tab, cat, area, area, st->live, nullptr, n_live, frame, counter, io, 0.5,
                                             [&](int o, const odise_track_row& row, int, int j) { return track_count_iou(row.area, area[j], inter[o * topk + j]); });
    if (tid == 0) {
        st->n_live = m.total;
        st->counter = (counter + m.n_new) % io.n_pool;
    }
    for (int i = tid; i < n_live * topk; i += kTrackMatchThreads) inter[i] = 0;
}

static void inst_track_free(odise_inst_track* t) {
    if (t->state) (void)hipFree(t->state);
    if (t->ring) (void)hipFree(t->ring);
    if (t->inter) (void)hipFree(t->inter);
    if (t->area) (void)hipFree(t->area);
    track_pool_free(&t->pool);
    delete t;
}

static size_t inst_track_inter_bytes(const odise_inst_track* t) { return (size_t)kTrackLiveCap * t->topk * sizeof(int); }

static int inst_track_clear(odise_hip_ctx* ctx, odise_inst_track* t) {
    ODISE_CHECK_HIP(hipMemsetAsync(t->state, 0, sizeof(InstTrackState), ctx->stream));
    ODISE_CHECK_HIP(hipMemsetAsync(t->inter, 0, inst_track_inter_bytes(t), ctx->stream));
    t->frame = 0;
    return ODISE_OK;
}

// everything that can be refused without the model is refused here, before anything is enqueued
static int inst_track_check_args(const odise_inst_track_desc* d) {
    ODISE_REQUIRE(d, "inst_track_frame: null descriptor");
    ODISE_REQUIRE(d->track && d->colors, "inst_track_frame: null pointer");
    ODISE_TRY(inst_source_check("inst_track_frame", inst_source(*d), false, kVisMaxPixels));
    const odise_inst_track* t = d->track;
    ODISE_REQUIRE(d->h == t->H && d->w == t->W && d->topk == t->topk, "inst_track_frame: a %dx%d frame of %d masks for a tracker of %dx%d and %d",
                  d->h, d->w, d->topk, t->H, t->W, t->topk);
    return track_check_dumps("inst_track_frame", d);
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_inst_track_create(odise_hip_ctx* ctx, int H, int W, int topk, int ttl, const uint8_t* pool_rgb, int n_pool,
                                           odise_inst_track** out) {
    ODISE_REQUIRE(ctx, "inst_track_create: null context");
    ODISE_REQUIRE(out && pool_rgb, "inst_track_create: null pointer");
    ODISE_TRY(vis_check_size("inst_track_create", H, W));
    ODISE_REQUIRE(topk >= 1 && topk <= kInstMaxTopk, "inst_track_create: topk %d outside 1..%d", topk, kInstMaxTopk);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    odise_inst_track* t = new odise_inst_track();
    t->H = H; t->W = W; t->topk = topk;
    t->G = rle_grid(H, W);
    int rc = track_pool_create("inst_track_create", ttl, pool_rgb, n_pool, &t->pool);
    if (rc == ODISE_OK) {
        t->slots = ttl + 1;
        const size_t ring_bytes = (size_t)t->slots * topk * (size_t)t->G.nw * sizeof(u64);
        const bool ok = hipMalloc((void**)&t->state, sizeof(InstTrackState)) == hipSuccess && hipMalloc((void**)&t->ring, ring_bytes) == hipSuccess &&
                        hipMalloc((void**)&t->inter, inst_track_inter_bytes(t)) == hipSuccess &&
                        hipMalloc((void**)&t->area, (size_t)2 * topk * sizeof(int)) == hipSuccess;
        if (!ok) rc = track_no_memory("inst_track_create", sizeof(InstTrackState) + ring_bytes + inst_track_inter_bytes(t) + (size_t)2 * topk * sizeof(int));
    }
    return track_created(rc, ctx, t, out, inst_track_clear, inst_track_free);
}

extern "C" int odise_hip_inst_track_reset(odise_hip_ctx* ctx, odise_inst_track* track) {
    return track_reset("inst_track_reset", ctx, track, inst_track_clear);
}

extern "C" int odise_hip_inst_track_destroy(odise_hip_ctx* ctx, odise_inst_track* track) {
    return track_destroy("inst_track_destroy", ctx, track, inst_track_free);
}

extern "C" int odise_hip_inst_track_frame(odise_hip_ctx* ctx, const odise_inst_track_desc* d) {
    ODISE_REQUIRE(ctx, "inst_track_frame: null context");
    ODISE_TRY(inst_track_check_args(d));
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    odise_inst_track* t = d->track;
    const int topk = t->topk;
    const RleGrid& G = t->G;
    const InstSource src = inst_source(*d);
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "inst_track_frame", src, &ig));
    const int new_slot = t->frame % t->slots;
    u64* words = t->ring + (int64_t)new_slot * topk * G.nw;
    const int* table = (const int*)d->inst_table;
    int* cls = t->area + topk;
    ODISE_TRY(inst_pack(ctx, src, ig, G, words));
    hipLaunchKernelGGL(inst_track_area_kernel, dim3((unsigned)topk), dim3(256), 0, ctx->stream, (const u64*)words, G.nw, table, d->inst_scores, topk,
                       d->min_score, t->area, cls);
    ODISE_CHECK_HIP(hipGetLastError());
    // the counts are device values: the grid covers the caps, and the word axis is split until it has about kGatherBlocks blocks
    const InterSplit sp = inst_inter_split(kTrackLiveCap, topk, G.nw, kGatherBlocks);
    hipLaunchKernelGGL(inst_track_inter_kernel, sp.grid, dim3(256), 0, ctx->stream, (const u64*)t->ring, (const InstTrackState*)t->state, table,
                       (const int*)t->area, (const int*)cls, topk, t->slots, new_slot, G.nw, sp.per, t->inter);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(inst_track_match_kernel, dim3(1), dim3(kTrackMatchThreads), 0, ctx->stream, t->inter, table, (const int*)t->area, (const int*)cls,
                       t->state, topk, t->frame, track_match_io(t->pool, d));
    ODISE_TRY(track_match_launched(ctx, t->inter, inst_track_inter_bytes(t)));   // the intersections are counted
    t->frame += 1;
    return ODISE_OK;
}
