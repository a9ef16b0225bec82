// rle_pack.h — what rle.hip (COCO RLE strings), inst_eval.hip (mask IoU and segm matching), poly.hip (polygon rasterisation), sem_rle.hip
// (per-class strings of a label map), vis_inst.hip (drawing) and inst_track.hip (colours across frames) share: the
// bit-packed mask layout, the block scan, the launchers of the dense pack kernel and the string passes (defined in rle.hip, compiled once)
// and the launcher of the polygon kernel (poly.hip).  What the users of INSTANCE masks share on top of it is in inst_words.h.
//   word (x, r) of a mask holds pixels (64 r .. 64 r + 63, x), bit k = row 64 r + k, stored [n][w][R], R = ceil(h / 64): the words of a
//   mask are consecutive pieces of the column-major order j = x * h + y.
#pragma once
#include "engine.h"
#include "post_sample.h"

namespace odise {

constexpr int kRleThreads = 1024;          // one block per mask (16 waves)
constexpr int64_t kRleMaxPixels = 1 << 30; // per mask (the post-processing's own output limit); positions stay in int

struct RleGrid {
    int h, w, R;      // mask size, words per column
    int64_t nw;       // words per mask = w * R
};
static inline RleGrid rle_grid(int h, int w) {
    RleGrid G;
    G.h = h; G.w = w; G.R = (int)ceil_div(h, 64);
    G.nw = (int64_t)w * G.R;
    return G;
}

// exclusive block scan of a sum over kRleThreads threads (wave scan by shuffles, then the 16 wave totals through LDS); ends in a barrier
__device__ inline long long block_scan_sum(long long v, long long* lds, long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    long long pre = 0;
    total = 0;
    for (int k = 0; k < kRleThreads / 64; ++k) {
        if (k < wave) pre += lds[k];
        total += lds[k];
    }
    __syncthreads();
    return pre + inc - v;
}

// words [n][G.nw] of n dense masks [n, h, w] (ODISE_F32 / ODISE_U8; any nonzero value is 1), on the context's stream
int rle_pack_dense(odise_hip_ctx* ctx, const void* masks, int dtype, int n, const RleGrid& G, unsigned long long* words);

// The context's scratch of the string passes for n masks (grown on demand; earlier calls on the stream may still read the old buffer) and
// `extra` bytes behind it for the caller.
struct RleState;
struct RleScratch {
    unsigned long long* words;
    RleState* state;
    long long* len;
    void* extra;
};
int rle_scratch(odise_hip_ctx* ctx, int n, const RleGrid& G, RleScratch* s, size_t extra = 0);
// count -> offsets -> write, after the words of n masks are packed
int rle_finish(odise_hip_ctx* ctx, const RleScratch& s, const RleGrid& G, int n, void* rle, int64_t capacity, int64_t* offsets, int64_t* area,
               const int* n_dev);

// words [n_ann][G.nw] of polygon annotations (poly.hip): annotation a is the OR of the rasterised polygons [ann_polys[a], ann_polys[a + 1]).
// toggle: [n_ann][G.nw] words of scratch.  fill_empty: an annotation without polygons gets the empty mask (otherwise its words are left as
// they are).  run_offsets (optional, [n_ann + 1]): an annotation with polygons AND a non-empty range here raises flag 4.  Flag 8: a bad polygon.
int poly_fill_words(odise_hip_ctx* ctx, const double* xy, const int64_t* poly_offsets, const int32_t* ann_polys, int n_ann, int n_poly,
                    const RleGrid& G, unsigned long long* words, unsigned long long* toggle, bool fill_empty, const int64_t* run_offsets, int* flag);

// Per-class strings of a semantic label map (sem_rle.hip; the RLE half of odise_hip_semantic_eval in eval_ops.hip).  The scratch is the
// context's RLE scratch for nmask masks (0 = no strings wanted) with, behind it, an int32 [h * w] label map of the call's own
// (own_labels: the arg-max of a score tensor is taken once, into it), the class counts [K], the class -> slot table [K] and the number of
// masks encoded.
struct SemRleScratch {
    RleScratch rle;
    int* labels;
    unsigned* counts;
    unsigned short* slot;
    int* n_enc;
};
int sem_rle_scratch(odise_hip_ctx* ctx, int nmask, const RleGrid& G, int K, bool own_labels, SemRleScratch* s);
// classes [max_classes] (ascending, -1 past the count), n_classes [1] (all present classes), the strings of the first nmask =
// min(max_classes, K) at most, offsets [max_classes + 1], area [max_classes] (optional); flag 1 = a label outside [0, K)
int sem_rle_encode(odise_hip_ctx* ctx, const SemRleScratch& s, const RleGrid& G, const int* labels, int K, int nmask, int max_classes, int* classes,
                   int* n_classes, void* rle, int64_t capacity, int64_t* offsets, int64_t* area, int* flags);

}  // namespace odise
