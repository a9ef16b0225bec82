// box_track.hip — instances that carry boxes keep their colours from frame to frame (odise_hip_box_track_*; detectron2
// VideoVisualizer._assign_colors, its FIRST path: an instance with a box is matched on box IoU above 0.6).  Host restatement:
// odise_amd/video.py BoxColorTracker.
//
// A box tracker needs no pixels and no ring: the state is the live rows of track_match.h and one float [4] per row.  One launch of one
// block per frame, no synchronisation; the frame number lives in the state, so the call can be replayed from a captured graph.
//
//   box_track_kernel   the table entries of the frame into LDS (kept = a candidate of inst_candidate whose box is finite and has a
//                      positive width and height), the live boxes into LDS, then track_match_block (track_match.h, shared with
//                      track.hip and inst_track.hip) with bb_iou (inst_words.h, the arithmetic of odise_hip_box_iou) of the two boxes as
//                      XYWH doubles and the threshold 0.6; a row's box moves with it through the `live_aux` slot of the match step.
#include "inst_words.h"
#include "track_match.h"

namespace odise {

constexpr double kBoxTrackIou = 0.6;     // detectron2 _assign_colors: threshold = 0.6 for boxes (0.5 for masks)

struct BoxTrackState {   // device
    int counter, n_live, frame, pad0;        // pool counter (kept modulo n_pool), rows of `live`, frames since the reset
    odise_track_row live[kTrackLiveCap];     // id = table index in the row's own frame, area = (int32) of the box's w * h
    float box[kTrackLiveCap][4];             // XYXY of live[k]
};

}  // namespace odise

struct odise_box_track {
    int topk = 0;
    odise::BoxTrackState* state = nullptr;
    odise::TrackPool pool;
};

namespace odise {

__device__ __forceinline__ bool box_finite(const float* b) { return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]); }

// bb_iou of two XYXY float boxes as XYWH doubles, (x0, y0, x1 - x0, y1 - y0) computed in double; crowd = 0
__device__ __forceinline__ double box_xyxy_iou(const float* a, const float* b) {
    return bb_iou((double)a[0], (double)a[1], (double)a[2] - (double)a[0], (double)a[3] - (double)a[1], (double)b[0], (double)b[1],
                  (double)b[2] - (double)b[0], (double)b[3] - (double)b[1], false);
}

// One block of kTrackMatchThreads.  st: the tracker before the frame -> after it.
__global__ void __launch_bounds__(kTrackMatchThreads) box_track_kernel(const float* __restrict__ boxes, const int* __restrict__ table,
                                                                      const float* __restrict__ scores, int topk, float min_score,
                                                                      BoxTrackState* __restrict__ st, TrackMatchIo io) {
    __shared__ int tab[ODISE_MAX_SEGMENTS], cat[ODISE_MAX_SEGMENTS], kept[ODISE_MAX_SEGMENTS], area[ODISE_MAX_SEGMENTS];
    __shared__ float nbox[ODISE_MAX_SEGMENTS][4];
    __shared__ float lbox[kTrackLiveCap][4];
    __shared__ int aux[kTrackLiveCap];       // before: -1 - list position; after: the same for a survivor, the table index of a fresh row
    const int tid = threadIdx.x;
    const int n = inst_count(table, topk);
    const int n_live = track_clamp(st->n_live, kTrackLiveCap), counter = st->counter, frame = st->frame;
    if (tid < n) {
        float b[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) b[c] = boxes[4 * tid + c];
        const bool k = inst_candidate(table, scores, topk, min_score, tid) && box_finite(b) && b[2] > b[0] && b[3] > b[1];
        tab[tid] = tid;
        cat[tid] = (table && k) ? table[1 + topk + tid] : 0;
        kept[tid] = k ? 1 : 0;
        int a = 0;
        if (k) {   // a product of two differences: nothing to contract
            const double wh = ((double)b[2] - (double)b[0]) * ((double)b[3] - (double)b[1]);
            a = wh >= 2147483647.0 ? INT32_MAX : (int)wh;
        }
        area[tid] = a;
#pragma unroll
        for (int c = 0; c < 4; ++c) nbox[tid][c] = b[c];
    }
    if (tid < n_live) {
#pragma unroll
        for (int c = 0; c < 4; ++c) lbox[tid][c] = st->box[tid][c];
        aux[tid] = -1 - tid;
    }
    __syncthreads();   // also: n_live, the counter and the frame are read before anything is written
    const TrackMatched m = track_match_block(n, tab, cat, kept, area, st->live, aux, n_live, frame, counter, io, kBoxTrackIou,
                                             [&](int o, const odise_track_row&, int, int j) { return box_xyxy_iou(lbox[o], nbox[j]); });
    __syncthreads();   // aux of every row of the new list is written
    if (tid < m.total) {
        const int a = aux[tid];
        const float* b = a >= 0 ? nbox[a] : lbox[-1 - a];
#pragma unroll
        for (int c = 0; c < 4; ++c) st->box[tid][c] = b[c];
    }
    if (tid == 0) {
        st->n_live = m.total;
        st->counter = (counter + m.n_new) % io.n_pool;
        st->frame = frame + 1;
    }
}

static void box_track_free(odise_box_track* t) {
    if (t->state) (void)hipFree(t->state);
    track_pool_free(&t->pool);
    delete t;
}

static int box_track_clear(odise_hip_ctx* ctx, odise_box_track* t) {
    ODISE_CHECK_HIP(hipMemsetAsync(t->state, 0, sizeof(BoxTrackState), ctx->stream));
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_sizeof_box_track_desc(void) { return (int)sizeof(odise_box_track_desc); }

extern "C" int odise_hip_box_track_create(odise_hip_ctx* ctx, int topk, int ttl, const uint8_t* pool_rgb, int n_pool, odise_box_track** out) {
    ODISE_REQUIRE(ctx, "box_track_create: null context");
    ODISE_REQUIRE(out && pool_rgb, "box_track_create: null pointer");
    ODISE_REQUIRE(topk >= 1 && topk <= kInstMaxTopk, "box_track_create: topk %d outside 1..%d", topk, kInstMaxTopk);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    odise_box_track* t = new odise_box_track();
    t->topk = topk;
    int rc = track_pool_create("box_track_create", ttl, pool_rgb, n_pool, &t->pool);
    if (rc == ODISE_OK && hipMalloc((void**)&t->state, sizeof(BoxTrackState)) != hipSuccess) rc = track_no_memory("box_track_create", sizeof(BoxTrackState));
    return track_created(rc, ctx, t, out, box_track_clear, box_track_free);
}

extern "C" int odise_hip_box_track_reset(odise_hip_ctx* ctx, odise_box_track* track) {
    return track_reset("box_track_reset", ctx, track, box_track_clear);
}

extern "C" int odise_hip_box_track_destroy(odise_hip_ctx* ctx, odise_box_track* track) {
    return track_destroy("box_track_destroy", ctx, track, box_track_free);
}

extern "C" int odise_hip_box_track_frame(odise_hip_ctx* ctx, const odise_box_track_desc* d) {
    ODISE_REQUIRE(ctx, "box_track_frame: null context");
    ODISE_REQUIRE(d, "box_track_frame: null descriptor");
    ODISE_REQUIRE(d->track && d->boxes && d->colors, "box_track_frame: null pointer");
    const odise_box_track* t = d->track;
    ODISE_REQUIRE(d->topk == t->topk, "box_track_frame: a frame of %d boxes for a tracker of %d", d->topk, t->topk);
    ODISE_TRY(track_check_dumps("box_track_frame", d));
    ODISE_REQUIRE((((uintptr_t)d->boxes | (uintptr_t)d->inst_table | (uintptr_t)d->inst_scores) & 3) == 0,
                  "box_track_frame: boxes / inst_table / inst_scores must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(box_track_kernel, dim3(1), dim3(kTrackMatchThreads), 0, ctx->stream, d->boxes, (const int*)d->inst_table, d->inst_scores, t->topk,
                       d->min_score, t->state, track_match_io(t->pool, d));
    return track_match_launched(ctx, nullptr, 0);   // one launch: nothing was counted before it
}
