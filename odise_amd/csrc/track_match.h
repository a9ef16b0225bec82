// track_match.h — what the colour trackers share (track.hip: panoptic things, a byte map per retained frame; inst_track.hip: instance
// masks, packed words per retained frame; box_track.hip: instance boxes, four floats per live row): the limits of the live list and the one-block match / colour / compact step of detectron2's
// VideoVisualizer._assign_colors (the rule: include/odise_hip.h above odise_hip_track_frame; host restatement: odise_amd/video.py).
// Where the IoU comes from is the caller's business: it hands in a functor.
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

}  // namespace odise
