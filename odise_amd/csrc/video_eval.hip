// video_eval.hip — video instance segmentation AP (YouTube-VIS) on the device: odise_hip_video_eval_reset / _frame / _finish, the
// evaluator of mask2former_video/data_video/ytvis_eval.py (datasets/ytvis_api/ytvoseval.py: COCOeval with the IoU of two tracks taken over
// the whole sequence and per-track mean areas).  Host restatement: odise_amd/video_eval.py.
//
//   frame    1. pack the detections into words and 2. decode / rasterise the frame's ground truth into the same words: inst_pack
//               and inst_gt_words (inst_words.h), the code of odise_hip_instance_eval.
//            3. video_inter_kernel: the tile loop of inst_inter_kernel (tile sizes and word split of inst_words.h) over the two sides;
//               its epilogue adds a partial count to inter[det_slot[d]][gt_slot[g]] with a 64-bit atomic.  The indirection costs two
//               loads per pair of masks at the very end, so no int32 [topk][n_gt] matrix is written and read again.
//            4. video_area_kernel: block_popcount of every mask, added to area_d / frames_d / area_g of its slot; one more block looks
//               for doubled slots (flag 16) and hands the flags of the frame to the caller.
//            The flags 1 / 4 / 8 of step 2 are read back ON THE DEVICE by steps 3 and 4: a frame that raised one adds nothing.
//   finish   inst_match_kernel (inst_match.h) over SeqIou: the IoU from the 64-bit sums, the crowd bit in the walk only, the area of an
//            unmatched track = area_d / frames_d against the video ranges.
// All sums are integers, so the bytes are the same from run to run whatever order the atomics arrive in.
#include "inst_match.h"

namespace odise {

constexpr int kVideoFlagSharedSlot = 16;

// ---- 3. intersections through the slot tables ---------------------------------------------------------------------------------------------
// inter[det_slot[d]][gt_slot[g]] += over the words [blockIdx.z * per, + per) of the masks; `per` is a multiple of kInterKC
__global__ void __launch_bounds__(256) video_inter_kernel(const u64* __restrict__ wd_d, const u64* __restrict__ wd_g, const int* __restrict__ inst_table,
                                                         int topk, int n_gt, int64_t nw, int64_t per, const int* __restrict__ det_slot,
                                                         const int* __restrict__ gt_slot, int max_tracks, int max_gt,
                                                         unsigned long long* __restrict__ inter, const int* __restrict__ status) {
    __shared__ u64 sd[kInterRows][kInterKC + 1];
    __shared__ u64 sg[kInterCols][kInterKC + 1];
    if (status[0]) return;   // the frame adds nothing
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n = inst_count(inst_table, topk);   // the words past it are unwritten
    const int d0 = blockIdx.x * kInterRows, g0 = blockIdx.y * kInterCols;
    if (d0 >= n) return;
    const int64_t k_begin = (int64_t)blockIdx.z * per, k_end = min(nw, k_begin + per);
    int acc[4][2] = {};   // a block sees at most `per` words of a mask: below 2^31 bits with h * w <= 2^30
    for (int64_t k0 = k_begin; k0 < k_end; k0 += kInterKC) {
        for (int e = tid; e < (kInterRows + kInterCols) * kInterKC; e += 256) {
            const int row = e / kInterKC, kk = e - row * kInterKC;
            const int64_t k = k0 + kk;
            if (row < kInterRows) sd[row][kk] = (d0 + row < n && k < k_end) ? wd_d[(int64_t)(d0 + row) * nw + k] : 0ull;
            else sg[row - kInterRows][kk] = (g0 + row - kInterRows < n_gt && k < k_end) ? wd_g[(int64_t)(g0 + row - kInterRows) * nw + k] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < kInterKC; ++kk) {
            const u64 b0 = sg[tx][kk], b1 = sg[tx + 16][kk];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u64 a = sd[ty + 16 * i][kk];
                acc[i][0] += __popcll(a & b0);
                acc[i][1] += __popcll(a & b1);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int d = d0 + ty + 16 * i, g = g0 + tx + 16 * j;
            if (d < n && g < n_gt && acc[i][j]) {
                const int s = det_slot[d], t = gt_slot[g];
                if ((unsigned)s < (unsigned)max_tracks && (unsigned)t < (unsigned)max_gt)
                    atomicAdd(&inter[(int64_t)s * max_gt + t], (unsigned long long)acc[i][j]);
            }
        }
}

// ---- 4. areas, doubled slots, flags ---------------------------------------------------------------------------------------------------
// block i < topk: detection i; block topk + j: ground truth j; the last block: flag 16 and the flags of the frame
__global__ void __launch_bounds__(256) video_area_kernel(const u64* __restrict__ words, const int* __restrict__ inst_table, int topk, int n_gt,
                                                        int64_t nw, const int* __restrict__ det_slot, const int* __restrict__ gt_slot, int max_tracks,
                                                        int max_gt, unsigned long long* __restrict__ area_d, unsigned long long* __restrict__ area_g,
                                                        int* __restrict__ frames_d, const int* __restrict__ status, int* __restrict__ flags) {
    __shared__ unsigned seen[kInstMaxGt / 32];
    __shared__ int dup;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int n = inst_count(inst_table, topk);
    if (i == topk + n_gt) {
        if (tid == 0) dup = 0;
        for (int side = 0; side < 2; ++side) {
            const int cnt = side ? n_gt : n, lim = side ? max_gt : max_tracks;
            const int* slot = side ? gt_slot : det_slot;
            for (int k = tid; k < kInstMaxGt / 32; k += 256) seen[k] = 0u;
            __syncthreads();
            for (int k = tid; k < cnt; k += 256) {
                const int s = slot[k];
                if ((unsigned)s < (unsigned)lim && (atomicOr(&seen[s >> 5], 1u << (s & 31)) >> (s & 31)) & 1u) dup = 1;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int f = status[0] | (dup ? kVideoFlagSharedSlot : 0);
            if (f) atomicOr(flags, f);
        }
        return;
    }
    if (status[0]) return;   // the frame adds nothing
    const bool det = i < topk;
    if (det && i >= n) return;   // its words are unwritten
    const int s = det ? det_slot[i] : gt_slot[i - topk];
    if ((unsigned)s >= (unsigned)(det ? max_tracks : max_gt)) return;
    const long long a = block_popcount(words + (int64_t)i * nw, nw);
    if (tid == 0 && a > 0) {
        if (det) {
            atomicAdd(&area_d[s], (unsigned long long)a);
            atomicAdd(&frames_d[s], 1);
        } else {
            atomicAdd(&area_g[s], (unsigned long long)a);
        }
    }
}

// ---- finish: the IoU of two tracks and the mean area of one ----------------------------------------------------------------------------------
struct VideoSums {
    const long long* inter;      // [max_tracks][max_gt]
    const long long* area_d;     // [max_tracks]
    const long long* area_g;     // [max_gt]
    const int* frames_d;         // [max_tracks]
    int max_gt;
    __device__ double iou(int s, int j) const {
        const long long in = inter[(int64_t)s * max_gt + j], u = area_d[s] + area_g[j] - in;
        return u != 0 ? (double)in / (double)u : 0.0;
    }
    __device__ double avg_area(int s) const { return frames_d[s] != 0 ? (double)area_d[s] / (double)frames_d[s] : 0.0; }
};

__device__ __forceinline__ bool video_area_outside(double area, int a) {   // [0, 1e10], [0, 128^2], [128^2, 256^2], [256^2, 1e10], ends included
    const double lo = a == 2 ? 16384.0 : a == 3 ? 65536.0 : 0.0, hi = a == 1 ? 16384.0 : a == 2 ? 65536.0 : 1e10;
    return area < lo || area > hi;
}

struct SeqIou {    // ytvoseval.py iou_seq on the sums of a video; a "detection" is a predicted track, a ground truth a ground-truth track
    static constexpr int kStatusMask = ~0;
    static constexpr bool kPublish = false;
    VideoSums v;
    __device__ int det_area(int i) const {   // what a row shows: the mean, truncated and clamped
        const double m = v.avg_area(i);
        return m >= 2147483647.0 ? 2147483647 : (int)m;
    }
    __device__ int gt_area(int) const { return 0; }
    __device__ int gt_check(int) const { return 0; }
    __device__ bool det_outside(int d, int, int a) const { return video_area_outside(v.avg_area(d), a); }
    __device__ double operator()(int d, int j, int, int, bool) const { return v.iou(d, j); }   // the crowd bit acts in the walk only
};

__global__ void __launch_bounds__(256) video_dump_kernel(VideoSums v, int n_tracks, int n_gt, double* __restrict__ iou, double* __restrict__ avg_area) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (iou && i < (int64_t)n_tracks * n_gt) {
        const int s = (int)(i / n_gt);
        iou[i] = v.iou(s, (int)(i - (int64_t)s * n_gt));
    }
    if (avg_area && i < n_tracks) avg_area[i] = v.avg_area((int)i);
}

static int video_state_check(const char* what, const odise_video_eval_state* st) {
    ODISE_REQUIRE(st, "%s: null state", what);
    ODISE_REQUIRE(st->max_tracks >= 1 && st->max_tracks <= kInstMaxTopk, "%s: max_tracks %d (1..%d)", what, st->max_tracks, kInstMaxTopk);
    ODISE_REQUIRE(st->max_gt >= 0 && st->max_gt <= kInstMaxGt, "%s: max_gt %d (0..%d)", what, st->max_gt, kInstMaxGt);
    ODISE_REQUIRE(st->area_d && st->frames_d && (st->max_gt == 0 || (st->inter && st->area_g)), "%s: null accumulator", what);
    ODISE_REQUIRE((((uintptr_t)st->inter | (uintptr_t)st->area_d | (uintptr_t)st->area_g) & 7) == 0 && ((uintptr_t)st->frames_d & 3) == 0,
                  "%s: accumulators must be aligned to their elements", what);
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_video_eval_reset(odise_hip_ctx* ctx, const odise_video_eval_state* st) {
    ODISE_REQUIRE(ctx, "video_eval_reset: null context");
    ODISE_TRY(video_state_check("video_eval_reset", st));
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    if (st->max_gt) {
        ODISE_CHECK_HIP(hipMemsetAsync(st->inter, 0, (size_t)st->max_tracks * st->max_gt * 8, ctx->stream));
        ODISE_CHECK_HIP(hipMemsetAsync(st->area_g, 0, (size_t)st->max_gt * 8, ctx->stream));
    }
    ODISE_CHECK_HIP(hipMemsetAsync(st->area_d, 0, (size_t)st->max_tracks * 8, ctx->stream));
    ODISE_CHECK_HIP(hipMemsetAsync(st->frames_d, 0, (size_t)st->max_tracks * 4, ctx->stream));
    return ODISE_OK;
}

extern "C" int odise_hip_video_eval_frame(odise_hip_ctx* ctx, const odise_video_frame_desc* d) {
    ODISE_REQUIRE(ctx && d, "video_eval_frame: null argument");
    const odise_video_eval_state* st = d->st;
    ODISE_TRY(video_state_check("video_eval_frame", st));
    ODISE_REQUIRE(d->flags && d->det_slot, "video_eval_frame: null flags / det_slot");
    const InstSource src = inst_source(*d);
    ODISE_TRY(inst_source_check("video_eval_frame", src, false, kRleMaxPixels));
    ODISE_REQUIRE(d->n_gt >= 0 && d->n_gt <= kInstMaxGt, "video_eval_frame: %d ground-truth masks (0..%d)", d->n_gt, kInstMaxGt);
    ODISE_REQUIRE(d->n_gt == 0 || (d->gt_runs && d->gt_offsets && d->gt_slot), "video_eval_frame: null ground truth");
    ODISE_REQUIRE(d->n_gt == 0 || st->max_gt > 0, "video_eval_frame: ground truth for a state without ground-truth tracks");
    ODISE_REQUIRE((((uintptr_t)d->det_slot | (uintptr_t)d->gt_slot | (uintptr_t)d->flags) & 3) == 0, "video_eval_frame: slots / flags must be 4-byte aligned");
    const odise_inst_poly_gt* p = d->polys;
    ODISE_REQUIRE(!p || p->n_poly >= 0, "video_eval_frame: %d polygons", p->n_poly);
    if (p && (d->n_gt == 0 || p->n_poly == 0)) p = nullptr;   // nothing to rasterise
    ODISE_REQUIRE(!p || (p->xy && p->poly_offsets && p->gt_polys), "video_eval_frame: null polygon ground truth");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "video_eval_frame", src, &ig));
    const RleGrid G = rle_grid(d->h, d->w);
    const int topk = d->topk, n_gt = d->n_gt;
    // scratch: words [topk + n_gt][nw] | toggle planes of the polygons [n_gt][nw] | the status of the frame
    const size_t wb = (size_t)round_up((int64_t)(topk + n_gt) * G.nw * 8, 256), tb = p ? (size_t)round_up((int64_t)n_gt * G.nw * 8, 256) : 0;
    ODISE_TRY(scratch_reserve(ctx->rle, wb + tb + 256, 8, drain_streams(ctx->stream), "rle"));
    u64* words = (u64*)ctx->rle.ptr;
    u64* words_g = words + (int64_t)topk * G.nw;
    u64* toggle = (u64*)((char*)ctx->rle.ptr + wb);
    int* status = (int*)((char*)ctx->rle.ptr + wb + tb);
    ODISE_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), ctx->stream));
    ODISE_TRY(inst_pack(ctx, src, ig, G, words));
    if (n_gt) {
        ODISE_TRY(inst_gt_words(ctx, d->gt_runs, d->gt_offsets, n_gt, G, words_g, toggle, status, p));
        const InterSplit sp = inst_inter_split(topk, n_gt, G.nw, 2 * ctx->cu_count);
        hipLaunchKernelGGL(video_inter_kernel, sp.grid, dim3(256), 0, ctx->stream, words, words_g, src.inst_table, topk, n_gt, G.nw, sp.per,
                           (const int*)d->det_slot, (const int*)d->gt_slot, st->max_tracks, st->max_gt, (unsigned long long*)st->inter, status);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(video_area_kernel, dim3((unsigned)(topk + n_gt + 1)), dim3(256), 0, ctx->stream, words, src.inst_table, topk, n_gt, G.nw,
                       (const int*)d->det_slot, (const int*)d->gt_slot, st->max_tracks, st->max_gt, (unsigned long long*)st->area_d,
                       (unsigned long long*)st->area_g, (int*)st->frames_d, status, (int*)d->flags);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_video_eval_finish(odise_hip_ctx* ctx, const odise_video_finish_desc* d) {
    ODISE_REQUIRE(ctx && d, "video_eval_finish: null argument");
    const odise_video_eval_state* st = d->st;
    ODISE_TRY(video_state_check("video_eval_finish", st));
    ODISE_REQUIRE(d->iou_thresholds && d->flags, "video_eval_finish: null iou_thresholds / flags");
    ODISE_REQUIRE(d->n_tracks >= 0 && d->n_tracks <= st->max_tracks, "video_eval_finish: %d tracks (0..%d)", d->n_tracks, st->max_tracks);
    ODISE_REQUIRE(d->n_gt >= 0 && d->n_gt <= st->max_gt, "video_eval_finish: %d ground-truth tracks (0..%d)", d->n_gt, st->max_gt);
    ODISE_REQUIRE(d->n_tracks == 0 || (d->track_scores && d->track_category), "video_eval_finish: null track_scores / track_category");
    ODISE_REQUIRE(d->n_gt == 0 || d->gt_rows, "video_eval_finish: null gt_rows");
    ODISE_REQUIRE(d->num_categories >= 1, "video_eval_finish: num_categories %d", d->num_categories);
    ODISE_REQUIRE(!d->rows == !d->n_rows, "video_eval_finish: only one of rows / n_rows");
    ODISE_REQUIRE(d->rows || d->iou || d->avg_area, "video_eval_finish: no output");
    ODISE_REQUIRE((((uintptr_t)d->rows | (uintptr_t)d->iou | (uintptr_t)d->avg_area) & 7) == 0 &&
                      (((uintptr_t)d->track_scores | (uintptr_t)d->track_category | (uintptr_t)d->gt_rows | (uintptr_t)d->n_rows | (uintptr_t)d->flags) & 3) == 0,
                  "video_eval_finish: misaligned pointer");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const VideoSums v{(const long long*)st->inter, (const long long*)st->area_d, (const long long*)st->area_g, (const int*)st->frames_d, st->max_gt};
    if (d->rows) {
        InstMatchArgs A;
        A.inst_table = nullptr; A.det_cls = (const int*)d->track_category; A.inst_scores = d->track_scores; A.gt_rows = (const int*)d->gt_rows;
        A.status = nullptr; A.rows = d->rows; A.n_rows = (int*)d->n_rows; A.flags = (int*)d->flags;
        A.topk = st->max_tracks; A.n_det = d->n_tracks; A.n_gt = d->n_gt; A.num_categories = d->num_categories; A.image = d->video;
        for (int t = 0; t < 10; ++t) A.thr[t] = d->iou_thresholds[t];
        hipLaunchKernelGGL(inst_match_kernel<SeqIou>, dim3(1), dim3(kRleThreads), 0, ctx->stream, A, SeqIou{v});
        ODISE_CHECK_HIP(hipGetLastError());
    }
    const int64_t items = std::max<int64_t>((d->iou ? (int64_t)d->n_tracks * d->n_gt : 0), d->avg_area ? d->n_tracks : 0);
    if (items > 0) {
        hipLaunchKernelGGL(video_dump_kernel, dim3((unsigned)ceil_div(items, 256)), dim3(256), 0, ctx->stream, v, d->n_tracks, d->n_gt, d->iou, d->avg_area);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}
