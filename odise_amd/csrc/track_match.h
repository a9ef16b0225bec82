// track_match.h — what the colour trackers share (track.hip: panoptic things, a byte map per retained frame; inst_track.hip: instance
// masks, packed words per retained frame; box_track.hip: instance boxes, four floats per live row): the limits of the live list and the one-block match / colour / compact step of detectron2's
// VideoVisualizer._assign_colors (the rule: include/odise_hip.h above odise_hip_track_frame; host restatement: odise_amd/video.py).
// Where the IoU comes from is the caller's business: it hands in a functor.  Behind the device code, the host half of the three files:
// the colour pool, the end of create / reset / destroy, the dump checks, the TrackMatchIo of a descriptor, the tail of a frame.
#pragma once
#include "common.h"
#include "rgb.h"

namespace odise {

constexpr int kTrackRing = 8;                                            // the largest ttl
constexpr int kTrackLiveCap = kTrackRing * ODISE_MAX_SEGMENTS;
constexpr int kTrackMatchThreads = 1024;                                 // >= kTrackLiveCap: a thread per live row
static_assert(kTrackMatchThreads >= kTrackLiveCap, "a thread per live row");

__device__ __forceinline__ int track_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the outline of a mask colour (visualize.instance_edge_colors): 3/10 of a light colour (channel sum >= 384), a dark one moved 7/10 of
// the way to white
__device__ __forceinline__ unsigned track_edge_rgb(unsigned c) {
    const unsigned r = c & 255u, g = (c >> 8) & 255u, b = (c >> 16) & 255u;
    if (r + g + b >= 384u) return (r * 3u / 10u) | ((g * 3u / 10u) << 8) | ((b * 3u / 10u) << 16);
    return (255u - (255u - r) * 3u / 10u) | ((255u - (255u - g) * 3u / 10u) << 8) | ((255u - (255u - b) * 3u / 10u) << 16);
}

struct TrackMatchIo {
    const uint8_t* pool; int n_pool, ttl;
    uint8_t* colors;             // [n][3], in/out: the rows of the frame's instances are written
    uint8_t* edge_colors;        // optional, as colors: track_edge_rgb of what is written there
    odise_track_row* live_out; int live_cap; int* n_live_out;
    double* iou_out; int iou_cap;
};
struct TrackMatched { int total, n_new; };   // rows of the list after the frame, instances that took a pool colour

// The IoU of two pixel counts and their common pixels, as the double division of the integers (the mask trackers)
__device__ __forceinline__ double track_count_iou(int area_o, int area_j, int in) { return (double)in / (double)((int64_t)area_o + area_j - in); }

// One block of kTrackMatchThreads, all of it.  tab / cat / inst / area [n] (LDS, complete and published by a barrier of the caller's): the
// id a fresh row gets, the category, inst > 0 = entry j is an instance of this frame, and the area its row carries (the mask trackers
// pass the pixels for both: area 0 = no instance).  live / live_aux [kTrackLiveCap]: the list before the frame -> after it (live_aux,
// optional: one int of the caller's per row, j for a fresh one).  n_live, frame and counter were read by the caller before any barrier.
// iou_of(o, row, aux, j) = the IoU (a double) of live row o and entry j; it is asked for instances of the row's category only.  A match
// needs an IoU above `threshold` (strict).  Returns the same to every thread; the caller stores the counts.
template <class Iou>
__device__ __forceinline__ TrackMatched track_match_block(int n, const int* tab, const int* cat, const int* inst, const int* area, odise_track_row* live,
                                                          int* live_aux, int n_live, int frame, int counter, const TrackMatchIo& io, double threshold,
                                                          Iou iou_of) {
    __shared__ int rank[ODISE_MAX_SEGMENTS];      // position of an entry among the frame's instances, -1 = no instance
    __shared__ int winner[ODISE_MAX_SEGMENTS];    // smallest list position of the live rows that chose the instance
    __shared__ int urank[ODISE_MAX_SEGMENTS];     // position among the instances that take a new colour
    __shared__ int rgb[ODISE_MAX_SEGMENTS];
    __shared__ int wave_sum[kTrackMatchThreads / 64];
    __shared__ int n_inst, n_new;
    const int tid = threadIdx.x;
    if (tid < n) winner[tid] = INT32_MAX;
    if (tid == 0) {
        int c = 0;
        for (int j = 0; j < n; ++j) rank[j] = inst[j] > 0 ? c++ : -1;
        n_inst = c;
    }
    __syncthreads();

    // a thread per live row: its iou row, the first maximum
    odise_track_row row = {};
    int my_aux = 0, choice = -1;
    if (tid < n_live) {
        row = live[tid];
        if (live_aux) my_aux = live_aux[tid];
        double best = 0.0;
        for (int j = 0; j < n; ++j) {
            if (rank[j] < 0) continue;
            double iou = 0.0;
            if (cat[j] == row.category) iou = iou_of(tid, row, my_aux, j);
            if (io.iou_out && tid < io.iou_cap) io.iou_out[(int64_t)tid * ODISE_MAX_SEGMENTS + rank[j]] = iou;
            if (iou > best) { best = iou; choice = j; }
        }
        if (best > threshold) atomicMin(&winner[choice], tid);
        else choice = -1;
    }
    __syncthreads();
    if (tid < n && rank[tid] >= 0 && winner[tid] != INT32_MAX) rgb[tid] = live[winner[tid]].rgb;   // read before the list is rewritten
    if (tid == 0) {
        int u = 0;
        for (int j = 0; j < n; ++j) urank[j] = (rank[j] >= 0 && winner[j] == INT32_MAX) ? u++ : -1;
        n_new = u;
    }
    __syncthreads();
    if (tid < n && rank[tid] >= 0) {
        if (urank[tid] >= 0) rgb[tid] = (int)rgb_load(io.pool + 3 * ((counter + urank[tid]) % io.n_pool));
        rgb_store(io.colors + 3 * tid, (unsigned)rgb[tid]);
        if (io.edge_colors) rgb_store(io.edge_colors + 3 * tid, track_edge_rgb((unsigned)rgb[tid]));
    }

    // the survivors keep their order behind the new instances: an exclusive block scan of the keep flags
    const bool matched = choice >= 0 && winner[choice] == tid;
    const int keep = (tid < n_live && !matched && row.ttl - 1 > 0) ? 1 : 0;
    const int lane = tid & 63, wave = tid >> 6;
    int inc = keep;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();   // also: every thread holds its row and the winners' colours are read, the list may be rewritten
    int before = 0, kept = 0;
    for (int v = 0; v < kTrackMatchThreads / 64; ++v) {
        const int s = wave_sum[v];
        if (v < wave) before += s;
        kept += s;
    }
    TrackMatched res;
    res.total = min(n_inst + kept, kTrackLiveCap);
    res.n_new = n_new;
    if (keep) {
        const int pos = n_inst + before + inc - 1;
        if (pos < kTrackLiveCap) {
            row.ttl -= 1;
            live[pos] = row;
            if (live_aux) live_aux[pos] = my_aux;
            if (io.live_out && pos < io.live_cap) io.live_out[pos] = row;
        }
    }
    if (tid < n && rank[tid] >= 0) {
        odise_track_row r;
        r.frame = frame; r.id = tab[tid]; r.category = cat[tid]; r.area = area[tid]; r.ttl = io.ttl; r.rgb = rgb[tid]; r.pad0 = 0; r.pad1 = 0;
        const int pos = rank[tid];
        live[pos] = r;
        if (live_aux) live_aux[pos] = tid;
        if (io.live_out && pos < io.live_cap) io.live_out[pos] = r;
    }
    if (tid == 0 && io.n_live_out) io.n_live_out[0] = res.total;
    return res;
}

// ---- the host half: what odise_hip_track_* / odise_hip_inst_track_* / odise_hip_box_track_* do alike.  `who` is the entry point's
// name, the front of every refusal.  A tracker keeps its own state struct, buffers, size checks, `clear` and `free`. ----

struct TrackPool {               // a tracker's share of TrackMatchIo: its colour pool on the device, and its ttl
    uint8_t* rgb = nullptr;      // [n][3]
    int n = 0, ttl = 0;
};

static inline int track_no_memory(const char* who, size_t bytes) {
    (void)hipGetLastError();
    set_error("%s: could not allocate %zu bytes", who, bytes);
    return ODISE_ERR_NOMEM;
}

static inline void track_pool_free(TrackPool* p) {
    if (p->rgb) (void)hipFree(p->rgb);
    p->rgb = nullptr;
}

// The limits of ttl and n_pool, then the pool: allocated and filled from pool_rgb (HOST [n_pool][3]) by a synchronous copy.  A pool
// that was refused holds nothing.
static inline int track_pool_create(const char* who, int ttl, const uint8_t* pool_rgb, int n_pool, TrackPool* p) {
    ODISE_REQUIRE(ttl >= 1 && ttl <= kTrackRing, "%s: ttl %d outside 1..%d", who, ttl, kTrackRing);
    ODISE_REQUIRE(n_pool >= 1 && n_pool <= (1 << 20), "%s: n_pool %d outside 1..2^20", who, n_pool);
    if (hipMalloc((void**)&p->rgb, (size_t)n_pool * 3) != hipSuccess) {
        p->rgb = nullptr;
        return track_no_memory(who, (size_t)n_pool * 3);
    }
    if (hipMemcpy(p->rgb, pool_rgb, (size_t)n_pool * 3, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        track_pool_free(p);
        set_error("%s: copying the colour pool failed", who);
        return ODISE_ERR_HIP;
    }
    p->n = n_pool;
    p->ttl = ttl;
    return ODISE_OK;
}

// The end of every *_create: rc = what allocating gave; a tracker that cannot be cleared is freed, one that can is handed out.
template <class T>
static int track_created(int rc, odise_hip_ctx* ctx, T* t, T** out, int (*clear)(odise_hip_ctx*, T*), void (*free_)(T*)) {
    if (rc == ODISE_OK) rc = clear(ctx, t);
    if (rc != ODISE_OK) {
        (void)hipGetLastError();
        free_(t);
        return rc;
    }
    *out = t;
    return ODISE_OK;
}

template <class T>
static int track_reset(const char* who, odise_hip_ctx* ctx, T* t, int (*clear)(odise_hip_ctx*, T*)) {
    ODISE_REQUIRE(ctx, "%s: null context", who);
    ODISE_REQUIRE(t, "%s: null tracker", who);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    return clear(ctx, t);
}

template <class T>
static int track_destroy(const char* who, odise_hip_ctx* ctx, T* t, void (*free_)(T*)) {
    ODISE_REQUIRE(ctx, "%s: null context", who);
    ODISE_REQUIRE(t, "%s: null tracker", who);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    ODISE_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // frames in flight read its memory
    free_(t);
    return ODISE_OK;
}

// The dump arguments of a frame descriptor (odise_track_desc, odise_inst_track_desc and odise_box_track_desc name them alike)
template <class Desc>
static int track_check_dumps(const char* who, const Desc* d) {
    ODISE_REQUIRE(d->live_cap >= 0 && d->iou_cap >= 0, "%s: negative cap (live_cap %d, iou_cap %d)", who, d->live_cap, d->iou_cap);
    ODISE_REQUIRE(!d->live || d->n_live, "%s: live without n_live", who);
    ODISE_REQUIRE((((uintptr_t)d->live | (uintptr_t)d->n_live) & 3) == 0 && ((uintptr_t)d->iou & 7) == 0,
                  "%s: live / n_live must be 4-byte aligned, iou 8-byte aligned", who);
    return ODISE_OK;
}

// edge_colors of a descriptor that has the member; odise_track_desc has none
template <class Desc>
static auto track_edge_colors(const Desc* d, int) -> decltype(d->edge_colors) { return d->edge_colors; }
template <class Desc>
static uint8_t* track_edge_colors(const Desc*, long) { return nullptr; }

template <class Desc>
static TrackMatchIo track_match_io(const TrackPool& p, const Desc* d) {
    TrackMatchIo io;
    io.pool = p.rgb; io.n_pool = p.n; io.ttl = p.ttl;
    io.colors = d->colors; io.edge_colors = track_edge_colors(d, 0);
    io.live_out = d->live; io.live_cap = d->live_cap; io.n_live_out = (int*)d->n_live;
    io.iou_out = d->iou; io.iou_cap = d->iou_cap;
    return io;
}

// After the match launch, the last of a frame.  When it failed to launch, nothing will clear what the launches before it counted
// (`counts`, zero between calls): that is done here.
static inline int track_match_launched(odise_hip_ctx* ctx, void* counts, size_t bytes) {
    const hipError_t launched = hipGetLastError();
    if (launched != hipSuccess) {
        if (bytes) (void)hipMemsetAsync(counts, 0, bytes, ctx->stream);
        ODISE_CHECK_HIP(launched);
    }
    return ODISE_OK;
}

}  // namespace odise
