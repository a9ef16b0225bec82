// inst_eval.hip — instance masks against ground truth on the device: odise_hip_mask_iou (pycocotools' mask.iou of dense masks against
// run-length masks) and odise_hip_instance_eval / odise_hip_instance_eval_poly (COCOeval.evaluateImg for iouType "segm", useCats = 1: the
// per-picture part of InstanceSegEvaluator / COCOEvaluator(tasks=("segm",)), odise/evaluation/d2_evaluator.py:29,104).  Host restatement:
// odise_amd/instance_eval.py.
//
//   1. pack     the detections into words [n][w][R] (inst_geom / inst_pack of inst_words.h: the kernels of rle.hip, the pixels of
//               odise_hip_instance_rle).
//   2. decode   the ground truth from uncompressed COCO run lengths into the same layout.  One block per mask walks its runs 1024 at a time:
//               a block scan gives the end position of every run of the chunk, then a thread per word of the chunk's span searches the first
//               run that reaches into its word and walks on from there.  Every position is clamped to h * w: counts that sum to anything
//               else raise flag 1 and never move a read or a write outside the mask.  A ground truth given as polygons
//               (odise_hip_instance_eval_poly) is left empty here and rasterised into the same words by poly.hip right behind.
//   3. inter    inter[d][g] = sum of popcount(words_d & words_g), tiled like a small GEMM: a block holds 32 words of 64 detections and 32
//               ground truths in LDS and a thread forms 4 x 2 pairs from them; the word axis is split over blockIdx.z (inst_inter_split
//               of inst_words.h, which also holds the tile sizes) and the partial counts meet in integer atomics (exact, and the same
//               from run to run).  inst_track_inter_kernel (inst_track.hip) is this loop over gathered rows; the two stay written out:
//               on one shared tile function this kernel took 3 to 5 us longer per call (profiles/README.md, inst_words_bench.json).
//               Areas are the popcounts of one side (block_popcount of inst_words.h).
//   4. iou      rleIou in double: inter == 0 -> 0, crowd -> inter / area_d, else inter / (area_d + area_g - inter).
//   5. match    one block.  Detections in descending score (ties keep table order), ground truths of a category in annotation order.  The 40
//               (area range, threshold) cells of a detection are the lanes 10 a + t of ONE wave, which walks the ground truths of the
//               detection's category once: a lane keeps the best available non-ignored one and the best available ignored one (>= on equal
//               values: the later one wins) and takes the second only when there is no first - evaluateImg's loop over the ground truths
//               sorted by ignore, with its break.  The IoUs of 64 ground truths are computed by the 64 lanes at once and handed round by
//               lane index.  Categories are independent, so the 16 waves of the block share the detections by category.  The matched /
//               ignored words of a row are the ballots of the wave.
// The walk is written once (inst_match.h, which odise_hip_video_eval_finish shares) and takes its IoU as a template argument: SegmIou is
// steps 3 and 4, BoxIou (odise_hip_instance_eval_bbox, iouType "bbox") is maskApi.c bbIou of the detections' boxes (inst_box.hip, from the
// words of step 1) against the annotations' boxes, BoundaryIou (odise_hip_instance_eval_boundary, Boundary AP) is the minimum of SegmIou
// and of the same rleIou on the boundaries of both sides (inst_boundary.hip, from the words of steps 1 and 2; step 3 runs once more on
// them).  All tasks of a picture run behind ONE pack and ONE decode.
#include "inst_match.h"

namespace odise {

// ---- 2. decode ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 bit_range(int a, int b) {   // bits a .. b - 1, 0 <= a < b <= 64
    const u64 m = b - a == 64 ? ~0ull : (1ull << (b - a)) - 1ull;
    return m << a;
}

__global__ void __launch_bounds__(kRleThreads) inst_decode_kernel(const uint32_t* __restrict__ runs, const long long* __restrict__ offsets,
                                                                 u64* __restrict__ words, RleGrid G, int* __restrict__ flag,
                                                                 const int* __restrict__ polys) {
    __shared__ long long ends[kRleThreads];
    __shared__ long long ls[kRleThreads / 64];
    const int tid = threadIdx.x;
    u64* wd = words + (int64_t)blockIdx.x * G.nw;
    for (int64_t i = tid; i < G.nw; i += kRleThreads) wd[i] = 0ull;
    const long long r0 = offsets[blockIdx.x];
    const bool poly = polys && polys[blockIdx.x + 1] > polys[blockIdx.x];   // the polygon kernel fills this mask (and checks that it has no runs)
    const long long m = poly ? 0ll : max(0ll, offsets[blockIdx.x + 1] - r0);
    const long long hw = (long long)G.h * G.w;
    long long carry = 0;   // positions before the chunk
    __syncthreads();
    for (long long c0 = 0; c0 < m; c0 += kRleThreads) {
        const long long v = c0 + tid < m ? (long long)runs[r0 + c0 + tid] : 0ll;
        long long total;
        const long long ex = block_scan_sum(v, ls, total);
        ends[tid] = carry + ex + v;   // run c0 + tid covers positions [carry + ex, ends[tid])
        __syncthreads();
        const long long A = carry, B = min(carry + total, hw);
        if (A < B) {   // the chunk covers positions [A, B) of the mask; ends[cl - 1] >= B
            const int cl = (int)min((long long)kRleThreads, m - c0);
            const int xa = (int)(A / G.h), xb = (int)((B - 1) / G.h);
            const int64_t wlo = (int64_t)xa * G.R + (((int)A - xa * G.h) >> 6), whi = (int64_t)xb * G.R + (((int)(B - 1) - xb * G.h) >> 6);
            for (int64_t wi = wlo + tid; wi <= whi; wi += kRleThreads) {
                const int x = (int)(wi / G.R), r = (int)(wi - (int64_t)x * G.R);
                const long long p0 = (long long)x * G.h + 64 * r, p1 = (long long)x * G.h + min(64 * r + 64, G.h);
                long long pos = max(p0, A);
                const long long pe = min(p1, B);
                int lo = 0, hi = cl - 1;   // the first run that ends behind pos
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ends[mid] > pos) hi = mid;
                    else lo = mid + 1;
                }
                u64 bits = 0ull;
                for (int k = lo; k < cl && pos < pe; ++k) {   // zero-length runs pass without a bit
                    const long long e = min(ends[k], pe);
                    if (e > pos) {
                        if ((c0 + k) & 1) bits |= bit_range((int)(pos - p0), (int)(e - p0));
                        pos = e;
                    }
                }
                if (bits) wd[wi] |= bits;   // a word on the edge of two chunks is written in both, a barrier apart
            }
        }
        carry += total;
        __syncthreads();
    }
    if (tid == 0 && carry != hw && !poly) atomicOr(flag, 1);
}

// ---- 3. intersections and areas -----------------------------------------------------------------------------------------------------------
// inter[n][n_gt] += over the words [blockIdx.z * per, + per) of the masks; `per` is a multiple of kInterKC
__global__ void __launch_bounds__(256) inst_inter_kernel(const u64* __restrict__ wd_d, const u64* __restrict__ wd_g, int n, int n_gt, int64_t nw,
                                                        int64_t per, int* __restrict__ inter) {
    __shared__ u64 sd[kInterRows][kInterKC + 1];
    __shared__ u64 sg[kInterCols][kInterKC + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int d0 = blockIdx.x * kInterRows, g0 = blockIdx.y * kInterCols;
    const int64_t k_begin = (int64_t)blockIdx.z * per, k_end = min(nw, k_begin + per);
    int acc[4][2] = {};
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
            if (d < n && g < n_gt && acc[i][j]) atomicAdd(&inter[(int64_t)d * n_gt + g], acc[i][j]);
        }
}

// area[row] = ones of a row of words; one block per row
__global__ void __launch_bounds__(256) inst_area_kernel(const u64* __restrict__ words, int64_t nw, long long* __restrict__ area) {
    const long long s = block_popcount(words + (int64_t)blockIdx.x * nw, nw);
    if (threadIdx.x == 0) area[blockIdx.x] = s;
}
int inst_area_launch(odise_hip_ctx* ctx, const u64* words, int n, int64_t nw, long long* area) {
    if (n <= 0) return ODISE_OK;
    hipLaunchKernelGGL(inst_area_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, words, nw, area);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

// ---- 4. iou (odise_hip_mask_iou) ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) inst_iou_kernel(const int* __restrict__ inter, const long long* __restrict__ area, int n, int n_gt,
                                                      const uint8_t* __restrict__ iscrowd, double* __restrict__ iou, int* __restrict__ inter_out,
                                                      long long* __restrict__ area_d, long long* __restrict__ area_g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * n_gt) return;
    const int d = (int)(i / n_gt), g = (int)(i - (int64_t)d * n_gt);
    const int in = inter[i];
    iou[i] = rle_iou(in, area[d], area[n + g], iscrowd && iscrowd[g] != 0);
    if (inter_out) inter_out[i] = in;
    if (area_d && g == 0) area_d[d] = area[d];
    if (area_g && d == 0) area_g[g] = area[n + g];
}
// odise_hip_mask_boundary_iou: the same on the boundaries' counts beside it, and the minimum of the two
__global__ void __launch_bounds__(256) inst_biou_kernel(const int* __restrict__ inter, const long long* __restrict__ area, const int* __restrict__ inter_b,
                                                       const long long* __restrict__ area_b, int n, int n_gt, const uint8_t* __restrict__ iscrowd,
                                                       double* __restrict__ iou, double* __restrict__ mask_iou, double* __restrict__ boundary_iou,
                                                       int* __restrict__ inter_out, long long* __restrict__ area_d, long long* __restrict__ area_g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * n_gt) return;
    const int d = (int)(i / n_gt), g = (int)(i - (int64_t)d * n_gt);
    const bool crowd = iscrowd && iscrowd[g] != 0;
    const double m = rle_iou(inter[i], area[d], area[n + g], crowd), b = rle_iou(inter_b[i], area_b[d], area_b[n + g], crowd);
    iou[i] = fmin(m, b);
    if (mask_iou) mask_iou[i] = m;
    if (boundary_iou) boundary_iou[i] = b;
    if (inter_out) inter_out[i] = inter[i];
    if (area_d && g == 0) area_d[d] = area[d];
    if (area_g && d == 0) area_g[g] = area[n + g];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
int inst_scratch(odise_hip_ctx* ctx, int n, int n_gt, const RleGrid& G, InstScratch* s, bool polygons, bool boxes, bool boundary,
                 size_t extra_bytes) {
    const size_t wb = (size_t)round_up((int64_t)(n + n_gt) * G.nw * 8, 256), ab = (size_t)round_up((int64_t)(n + n_gt) * 8, 256);
    s->inter_bytes = ((size_t)n * n_gt + 1) * sizeof(int);
    const size_t ib = (size_t)round_up((int64_t)s->inter_bytes, 256);
    const size_t bb = boxes ? (size_t)round_up((int64_t)n * 16, 256) : 0;
    const size_t tb = polygons ? (size_t)round_up((int64_t)n_gt * G.nw * 8, 256) : 0;
    const size_t db = boundary ? 2 * wb + ab + ib : 0;
    ODISE_TRY(scratch_reserve(ctx->rle, wb + ab + ib + bb + tb + db + extra_bytes, 8, drain_streams(ctx->stream), "rle"));
    char* p = (char*)ctx->rle.ptr;
    s->words_d = (u64*)p;
    s->words_g = s->words_d + (int64_t)n * G.nw;
    s->area = (long long*)(p + wb);
    s->inter = (int*)(p + wb + ab);
    s->boxes = (float*)(p + wb + ab + ib);
    s->toggle = (u64*)(p + wb + ab + ib + bb);
    char* q = p + wb + ab + ib + bb + tb;
    s->bwords = (u64*)q;
    s->btmp = (u64*)(q + wb);
    s->barea = (long long*)(q + 2 * wb);
    s->binter = (int*)(q + 2 * wb + ab);
    s->extra = q + db;
    return ODISE_OK;
}

// stage 3 on words [n + n_gt][G.nw], detections first: inter [n][n_gt] (zeroed by the caller) and area [n + n_gt]
static int inst_counts(odise_hip_ctx* ctx, const u64* words, const RleGrid& G, int n, int n_gt, int* inter, long long* area) {
    if (n_gt) {
        // split the word axis until the grid fills the chip about twice (at most 2 * cu_count ways: far below the grid's z limit)
        const InterSplit sp = inst_inter_split(n, n_gt, G.nw, 2 * ctx->cu_count);
        hipLaunchKernelGGL(inst_inter_kernel, sp.grid, dim3(256), 0, ctx->stream, words, words + (int64_t)n * G.nw, n, n_gt, G.nw, sp.per, inter);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return inst_area_launch(ctx, words, n + n_gt, G.nw, area);
}

// stage 2 (declared in inst_words.h): the words of the ground truth
int inst_gt_words(odise_hip_ctx* ctx, const uint32_t* gt_runs, const int64_t* gt_offsets, int n_gt, const RleGrid& G, u64* words_g, u64* toggle,
                  int* flag, const odise_inst_poly_gt* p) {
    hipLaunchKernelGGL(inst_decode_kernel, dim3((unsigned)n_gt), dim3(kRleThreads), 0, ctx->stream, gt_runs, (const long long*)gt_offsets, words_g, G,
                       flag, p ? (const int*)p->gt_polys : nullptr);
    ODISE_CHECK_HIP(hipGetLastError());
    if (p) ODISE_TRY(poly_fill_words(ctx, p->xy, p->poly_offsets, p->gt_polys, n_gt, p->n_poly, G, words_g, toggle, false, gt_offsets, flag));
    return ODISE_OK;
}

// stages 2 and 3 behind the packed detections (declared in inst_words.h)
int inst_overlaps(odise_hip_ctx* ctx, const InstScratch& s, const RleGrid& G, int n, const uint32_t* gt_runs, const int64_t* gt_offsets, int n_gt,
                  int* flag, const odise_inst_poly_gt* p) {
    if (n_gt) ODISE_TRY(inst_gt_words(ctx, gt_runs, gt_offsets, n_gt, G, s.words_g, s.toggle, flag, p));
    return inst_counts(ctx, s.words_d, G, n, n_gt, s.inter, s.area);
}

// the same counts of the boundaries of the words inst_overlaps left (binter is zeroed here).  The first n masks are the selection
// inst_table (nullptr: all n): the logits pack leaves the words past its count unwritten, and their boundaries are zeros.
static int inst_boundary_overlaps(odise_hip_ctx* ctx, const InstScratch& s, const RleGrid& G, int n, int n_gt, int radius, const int* inst_table) {
    ODISE_CHECK_HIP(hipMemsetAsync(s.binter, 0, std::max<size_t>(1, (size_t)n * n_gt) * sizeof(int), ctx->stream));
    ODISE_TRY(inst_boundary_words(ctx, s.words_d, n + n_gt, G, radius > 0 ? radius : odise_hip_boundary_radius(G.h, G.w), inst_table, n, s.bwords, s.btmp));
    return inst_counts(ctx, s.bwords, G, n, n_gt, s.binter, s.barea);
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_mask_iou(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, const uint32_t* gt_runs,
                                  const int64_t* gt_offsets, int n_gt, const uint8_t* iscrowd, double* iou, int32_t* inter, int64_t* area_d,
                                  int64_t* area_g, int32_t* flags) {
    ODISE_REQUIRE(ctx && flags, "mask_iou: null argument");
    ODISE_REQUIRE(n >= 0 && n <= 65535 && n_gt >= 0 && n_gt <= 65535 && (int64_t)n * n_gt <= (1 << 26), "mask_iou: %d x %d masks out of range", n, n_gt);
    ODISE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kRleMaxPixels, "mask_iou: mask size %dx%d out of range", h, w);
    ODISE_REQUIRE(dtype == ODISE_F32 || dtype == ODISE_U8, "mask_iou: dtype %d (ODISE_F32 or ODISE_U8)", dtype);
    if (n == 0 || n_gt == 0) return ODISE_OK;
    ODISE_REQUIRE(masks && gt_runs && gt_offsets && iou, "mask_iou: null argument");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const RleGrid G = rle_grid(h, w);
    InstScratch s;
    ODISE_TRY(inst_scratch(ctx, n, n_gt, G, &s));
    ODISE_CHECK_HIP(hipMemsetAsync(s.inter, 0, s.inter_bytes, ctx->stream));
    ODISE_TRY(rle_pack_dense(ctx, masks, dtype, n, G, s.words_d));
    ODISE_TRY(inst_overlaps(ctx, s, G, n, gt_runs, gt_offsets, n_gt, (int*)flags));
    hipLaunchKernelGGL(inst_iou_kernel, dim3((unsigned)ceil_div((int64_t)n * n_gt, 256)), dim3(256), 0, ctx->stream, (const int*)s.inter,
                       (const long long*)s.area, n, n_gt, iscrowd, iou, (int*)inter, (long long*)area_d, (long long*)area_g);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_mask_boundary_iou(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, const uint32_t* gt_runs,
                                           const int64_t* gt_offsets, int n_gt, const uint8_t* iscrowd, int radius, double* iou, double* mask_iou,
                                           double* boundary_iou, int32_t* inter, int64_t* area_d, int64_t* area_g, int32_t* flags) {
    ODISE_REQUIRE(ctx && flags, "mask_boundary_iou: null argument");
    ODISE_REQUIRE(n >= 0 && n <= 65535 && n_gt >= 0 && n_gt <= 65535 && (int64_t)n * n_gt <= (1 << 26), "mask_boundary_iou: %d x %d masks out of range", n,
                  n_gt);
    ODISE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kRleMaxPixels, "mask_boundary_iou: mask size %dx%d out of range", h, w);
    ODISE_REQUIRE(dtype == ODISE_F32 || dtype == ODISE_U8, "mask_boundary_iou: dtype %d (ODISE_F32 or ODISE_U8)", dtype);
    if (n == 0 || n_gt == 0) return ODISE_OK;
    ODISE_REQUIRE(masks && gt_runs && gt_offsets && iou, "mask_boundary_iou: null argument");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const RleGrid G = rle_grid(h, w);
    InstScratch s;
    ODISE_TRY(inst_scratch(ctx, n, n_gt, G, &s, false, false, true));
    ODISE_CHECK_HIP(hipMemsetAsync(s.inter, 0, s.inter_bytes, ctx->stream));
    ODISE_TRY(rle_pack_dense(ctx, masks, dtype, n, G, s.words_d));
    ODISE_TRY(inst_overlaps(ctx, s, G, n, gt_runs, gt_offsets, n_gt, (int*)flags));
    ODISE_TRY(inst_boundary_overlaps(ctx, s, G, n, n_gt, radius, nullptr));
    hipLaunchKernelGGL(inst_biou_kernel, dim3((unsigned)ceil_div((int64_t)n * n_gt, 256)), dim3(256), 0, ctx->stream, (const int*)s.inter,
                       (const long long*)s.area, (const int*)s.binter, (const long long*)s.barea, n, n_gt, iscrowd, iou, mask_iou, boundary_iou,
                       (int*)inter, (long long*)area_d, (long long*)area_g);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

// evaluateImg of one picture for "segm" (d->rows), "bbox" (bb), "boundary" (bd), or any of them from one pack of the detections
static int inst_eval_run(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p, const odise_inst_bbox_task* bb, bool want_bbox,
                         const odise_inst_boundary_task* bd = nullptr) {
    ODISE_REQUIRE(ctx && d, "instance_eval: null argument");
    ODISE_REQUIRE(!want_bbox || (bb && bb->rows && bb->n_rows), "instance_eval: null bbox task");
    ODISE_REQUIRE(!bd || (bd->rows && bd->n_rows), "instance_eval: null boundary task");
    const bool segm_rows = !(want_bbox || bd) || d->rows || d->n_rows;   // beside another task the segm rows are skipped when they have nowhere to go
    const bool segm = segm_rows || bd;                                   // the boundary task needs the masks' counts too
    ODISE_REQUIRE(d->iou_thresholds && d->flags && (!segm_rows || (d->rows && d->n_rows)), "instance_eval: null pointer");
    const InstSource src = inst_source(*d);
    ODISE_TRY(inst_source_check("instance_eval", src, true, kRleMaxPixels));   // the match step reads the table and the scores of dense masks too
    ODISE_REQUIRE(d->n_gt >= 0 && d->n_gt <= kInstMaxGt, "instance_eval: %d ground-truth masks (0..%d)", d->n_gt, kInstMaxGt);
    ODISE_REQUIRE(d->n_gt == 0 || (d->gt_rows && (!segm || (d->gt_runs && d->gt_offsets)) && (!want_bbox || bb->gt_boxes)),
                  "instance_eval: null ground truth");
    if (!segm) p = nullptr;
    ODISE_REQUIRE(!p || p->n_poly >= 0, "instance_eval: %d polygons", p->n_poly);
    if (p && (d->n_gt == 0 || p->n_poly == 0)) p = nullptr;   // nothing to rasterise
    ODISE_REQUIRE(!p || (p->xy && p->poly_offsets && p->gt_polys), "instance_eval: null polygon ground truth");
    ODISE_REQUIRE(d->num_categories >= 1, "instance_eval: num_categories %d", d->num_categories);
    ODISE_REQUIRE(!want_bbox || (((uintptr_t)bb->gt_boxes & 7) == 0 && ((uintptr_t)bb->boxes & 3) == 0), "instance_eval: gt_boxes / boxes misaligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "instance_eval", src, &ig));
    const RleGrid G = rle_grid(d->h, d->w);
    InstScratch s;
    ODISE_TRY(inst_scratch(ctx, d->topk, d->n_gt, G, &s, p != nullptr, want_bbox && !bb->boxes, bd != nullptr));
    ODISE_CHECK_HIP(hipMemsetAsync(s.inter, 0, s.inter_bytes, ctx->stream));
    int* status = s.inter + (size_t)d->topk * d->n_gt;
    ODISE_TRY(inst_pack(ctx, src, ig, G, s.words_d));
    if (segm) ODISE_TRY(inst_overlaps(ctx, s, G, d->topk, d->gt_runs, d->gt_offsets, d->n_gt, status, p));
    if (bd) ODISE_TRY(inst_boundary_overlaps(ctx, s, G, d->topk, d->n_gt, bd->radius, src.inst_table));
    InstMatchArgs A;
    A.inst_table = (const int*)d->inst_table; A.det_cls = A.inst_table + 1 + d->topk; A.inst_scores = d->inst_scores; A.gt_rows = (const int*)d->gt_rows;
    A.status = status; A.flags = (int*)d->flags;
    A.topk = d->topk; A.n_det = 0; A.n_gt = d->n_gt; A.num_categories = d->num_categories; A.image = d->image;
    for (int t = 0; t < 10; ++t) A.thr[t] = d->iou_thresholds[t];
    if (want_bbox) {   // first: a flag it raises (2, 4) is in `status` when the segm match reads it
        float* boxes = bb->boxes ? bb->boxes : s.boxes;
        ODISE_TRY(inst_boxes_launch(ctx, s.words_d, G, src.inst_table, d->topk, boxes));
        A.rows = bb->rows; A.n_rows = (int*)bb->n_rows;
        hipLaunchKernelGGL(inst_match_kernel<BoxIou>, dim3(1), dim3(kRleThreads), 0, ctx->stream, A, BoxIou{boxes, bb->gt_boxes});
        ODISE_CHECK_HIP(hipGetLastError());
    }
    const SegmIou mask_iou{s.inter, s.area, d->topk, d->n_gt};
    if (segm_rows) {
        A.rows = d->rows; A.n_rows = (int*)d->n_rows;
        hipLaunchKernelGGL(inst_match_kernel<SegmIou>, dim3(1), dim3(kRleThreads), 0, ctx->stream, A, mask_iou);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    if (bd) {
        A.rows = bd->rows; A.n_rows = (int*)bd->n_rows;
        hipLaunchKernelGGL(inst_match_kernel<BoundaryIou>, dim3(1), dim3(kRleThreads), 0, ctx->stream, A,
                           BoundaryIou{mask_iou, SegmIou{s.binter, s.barea, d->topk, d->n_gt}});
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

extern "C" int odise_hip_instance_eval(odise_hip_ctx* ctx, const odise_inst_eval_desc* d) { return inst_eval_run(ctx, d, nullptr, nullptr, false); }

extern "C" int odise_hip_instance_eval_poly(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p) {
    return inst_eval_run(ctx, d, p, nullptr, false);
}

extern "C" int odise_hip_instance_eval_bbox(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p,
                                            const odise_inst_bbox_task* bb) {
    return inst_eval_run(ctx, d, p, bb, true);
}

extern "C" int odise_hip_instance_eval_boundary(odise_hip_ctx* ctx, const odise_inst_eval_desc* d, const odise_inst_poly_gt* p,
                                                const odise_inst_bbox_task* bb, const odise_inst_boundary_task* bd) {
    return inst_eval_run(ctx, d, p, bb, bb != nullptr, bd);
}
