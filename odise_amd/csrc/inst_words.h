// inst_words.h — "the instance masks of a picture" as the bit-packed words of rle_pack.h, written once for the entry points that
// take them: odise_hip_instance_eval(_poly, _bbox) (inst_eval.hip), odise_hip_instance_draw (vis_inst.hip), odise_hip_inst_track_frame
// (inst_track.hip), odise_hip_instance_boxes (inst_box.hip), odise_hip_mask_boundary (inst_boundary.hip) and odise_hip_instance_rle
// (rle.hip, which also compiles inst_source_check, inst_geom and inst_pack).
//   host    InstSource (the detection fields the three public descriptors share), its check, the geometry lookup and the pack launch,
//           the split of the word axis of the intersection kernels
//   device  the clamped count of a selection and the candidate rule, the block popcount of a row of words, the tile sizes of the
//           intersection kernels
#pragma once
#include <algorithm>

#include "rle_pack.h"

namespace odise {

typedef unsigned long long u64;

constexpr int kInstMaxTopk = 100;   // the instance head keeps, and the evaluator looks at, no more than 100 detections per picture
static_assert(kInstMaxTopk <= ODISE_MAX_SEGMENTS, "the shared match step holds ODISE_MAX_SEGMENTS entries");

// The detections of a picture: dense masks [topk, h, w] (ODISE_F32 / ODISE_U8), or masks == nullptr = the selection inst_table /
// inst_scores of image b of the last head forward, sampled from its mask logits.
struct InstSource {
    int h, w;
    const void* masks;
    int dtype, b, pad_h, pad_w, img_h, img_w;
    const int* inst_table;
    const float* inst_scores;
    int topk;
};
template <class Desc>
static inline InstSource inst_source(const Desc& d) {   // odise_inst_eval_desc, odise_inst_draw_desc, odise_inst_track_desc
    return InstSource{d.h, d.w, d.masks, d.dtype, d.b, d.pad_h, d.pad_w, d.img_h, d.img_w, (const int*)d.inst_table, d.inst_scores, d.topk};
}
// What can be refused without the model (the errors carry `what`).  need_table: the caller reads inst_table and inst_scores with dense
// masks too; max_pixels: the caller's bound on h * w.
// max_topk: the caller's bound on topk (odise_hip_lvis_eval looks at 300 detections, lvis_eval.hip).
int inst_source_check(const char* what, const InstSource& s, bool need_table, int64_t max_pixels, int max_topk = kInstMaxTopk);
// The sampling geometry and the mask logits of a source without dense masks (unused with them): image b of the last head forward, its
// geometry checked (the errors carry `what`).  Enqueues nothing and touches no scratch, so a caller runs it before it reserves any.
struct InstGeom {
    PostGeom g;
    const f16* logits;
};
int inst_geom(odise_hip_ctx* ctx, const char* what, const InstSource& s, InstGeom* ig);
// words [topk][G.nw] of the source: the dense pack, or the logits pack, which leaves the masks past the count of the table unwritten
int inst_pack(odise_hip_ctx* ctx, const InstSource& s, const InstGeom& ig, const RleGrid& G, u64* words);
// words_g [n_gt][G.nw] of a picture's ground truth (inst_eval.hip): every mask is zeroed and decoded from its run lengths; with p, one
// that has polygons is rasterised instead (poly.hip; toggle: [n_gt][G.nw] words of scratch).  flag (device int [1]) collects 1 (runs
// that do not sum to h * w), 4 (runs AND polygons on one ground truth) and 8 (a bad polygon).  n_gt >= 1.
int inst_gt_words(odise_hip_ctx* ctx, const uint32_t* gt_runs, const int64_t* gt_offsets, int n_gt, const RleGrid& G, u64* words_g, u64* toggle,
                  int* flag, const odise_inst_poly_gt* p);

// The scratch of one picture's evaluation (inst_eval.hip; lvis_eval.hip takes the same) and stages 2 and 3 behind the packed detections.
struct InstScratch {
    u64 *words_d, *words_g;
    long long* area;   // [n + n_gt]
    int* inter;        // [n][n_gt], then one int: the status of the call
    size_t inter_bytes;
    u64* toggle;       // with polygon ground truth: the toggle planes of poly.hip, [n_gt] masks
    float* boxes;      // the bbox task without an output for them: [n][4]
    // the boundary task: the boundaries of all n + n_gt masks (detections first, like the words they come from), the temporary of
    // inst_boundary_words, their areas [n + n_gt] and intersections [n][n_gt]
    u64 *bwords, *btmp;
    long long* barea;
    int* binter;
    char* extra;       // extra_bytes of the caller's own, 256-byte aligned
};
int inst_scratch(odise_hip_ctx* ctx, int n, int n_gt, const RleGrid& G, InstScratch* s, bool polygons = false, bool boxes = false,
                 bool boundary = false, size_t extra_bytes = 0);
// ground-truth words, inter [n][n_gt] (zeroed by the caller) and area [n + n_gt] of s.words_d; flag 1 (and 4, 8 of polygon ground truth)
// goes to `flag`
int inst_overlaps(odise_hip_ctx* ctx, const InstScratch& s, const RleGrid& G, int n, const uint32_t* gt_runs, const int64_t* gt_offsets, int n_gt,
                  int* flag, const odise_inst_poly_gt* p = nullptr);

// ---- device: count, candidates, area -------------------------------------------------------------------------------------------------
// the instances of a selection: table[0] clamped to 0..topk; no table = all topk
__device__ __forceinline__ int inst_count(const int* __restrict__ table, int topk) {
    if (!table) return topk;
    const int n = table[0];
    return n < 0 ? 0 : (n > topk ? topk : n);
}
// table index i is a candidate: below the count, and its score passes.  A candidate with a pixel is `kept`.
__device__ __forceinline__ bool inst_candidate(const int* __restrict__ table, const float* __restrict__ scores, int topk, float min_score, int i) {
    return i < inst_count(table, topk) && (!scores || scores[i] >= min_score);
}
// ones of nw words, summed over a block of 256 threads (shuffles, then the four wave partials through LDS); ends in a barrier
__device__ __forceinline__ long long block_popcount(const u64* __restrict__ wd, int64_t nw) {
    __shared__ long long part[4];
    long long s = 0;
    for (int64_t i = threadIdx.x; i < nw; i += 256) s += __popcll(wd[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// ---- boxes (inst_box.hip) ---------------------------------------------------------------------------------------------------------------
// boxes float [topk][4] XYXY of words [topk][G.nw] (BitMasks.get_bounding_boxes); rows past the count of inst_table (nullptr: none) are
// zeros and their words are not read
int inst_boxes_launch(odise_hip_ctx* ctx, const u64* words, const RleGrid& G, const int* inst_table, int topk, float* boxes);
// maskApi.c bbIou of two XYWH boxes, every product and sum rounded on its own: contraction is off inside (as poly.hip has it for its
// whole file), since the compiler would fuse da + ga - i and the like into multiply-adds, which the host restatement
// (instance_eval.box_iou) does not have.  The rounding intrinsics (__dmul_rn ..) are plain operators in this toolchain and fuse as well.
__device__ __forceinline__ double bb_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw, double gh, bool crowd) {
#pragma clang fp contract(off)
    const double da = dw * dh, ga = gw * gh;
    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
    if (w <= 0.0) return 0.0;
    const double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
    if (h <= 0.0) return 0.0;
    const double i = w * h;
    const double u = crowd ? da : da + ga - i;
    return i / u;
}

// ---- areas and boundaries (inst_eval.hip, inst_boundary.hip) ------------------------------------------------------------------------------
// area[i] = the ones of words [n][nw] (inst_area_kernel: block_popcount, one block per mask)
int inst_area_launch(odise_hip_ctx* ctx, const u64* words, int n, int64_t nw, long long* area);
// words_out [n][G.nw] = words_in & ~erode(words_in), the (2 r + 1)^2 erosion that sees zeros outside the picture (r >= 1).  The first
// topk masks are a selection: those past the count of inst_table (nullptr: none) are not read and their output is zeros.  words_tmp:
// [n][G.nw] words of scratch.  The padding bits past row h of words_in must be zero (every producer of these words leaves them so).
int inst_boundary_words(odise_hip_ctx* ctx, const u64* words_in, int n, const RleGrid& G, int r, const int* inst_table, int topk, u64* words_out,
                        u64* words_tmp);

// ---- the intersection kernels (inst_inter_kernel, inst_track_inter_kernel) --------------------------------------------------------------
// A block of 256 threads counts popcount(a & b) for kInterRows x kInterCols pairs of masks, tiled like a small GEMM: kInterKC words of
// every row in LDS (padded rows), a thread forms 4 x 2 pairs from them.  The loop itself is written out in both kernels.
constexpr int kInterRows = 64, kInterCols = 32, kInterKC = 32;

// The grid of an intersection kernel over rows x cols masks of nw words: the word axis is split over blockIdx.z until the grid has about
// target_blocks blocks; a block takes `per` words, a multiple of kInterKC.
struct InterSplit {
    int64_t per;
    dim3 grid;
};
static inline InterSplit inst_inter_split(int64_t rows, int64_t cols, int64_t nw, int64_t target_blocks) {
    const int64_t rt = ceil_div(rows, kInterRows), ct = ceil_div(cols, kInterCols), steps = ceil_div(nw, kInterKC);
    const int64_t kz = std::max<int64_t>(1, std::min<int64_t>(steps, target_blocks / (rt * ct)));
    InterSplit s;
    s.per = ceil_div(steps, kz) * kInterKC;
    s.grid = dim3((unsigned)rt, (unsigned)ct, (unsigned)ceil_div(nw, s.per));
    return s;
}

}  // namespace odise
