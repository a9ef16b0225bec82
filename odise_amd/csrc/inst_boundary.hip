// inst_boundary.hip — the boundaries of instance masks on the device, on the packed words of rle_pack.h / inst_words.h: inst_boundary_words
// (words -> words & ~erode(words), the rule of Boundary IoU: Cheng et al., CVPR 2021; detectron2's _mask_to_boundary on a binary mask) and
// odise_hip_mask_boundary (dense masks in, dense boundaries out).  Host restatement: odise_amd/instance_eval.py mask_boundary.  The users
// of the words are odise_hip_mask_boundary_iou and odise_hip_instance_eval_boundary (inst_eval.hip).
//
// The erosion is the (2 r + 1)^2 minimum that sees zeros outside the picture, i.e. an AND over a window.  With a[x][y] = AND of the mask
// over the square [x, x + s) x [y, y + s), the square doubles by
//     a'[x][y] = a[x][y] & a[x + k][y] & a[x][y + k] & a[x + k][y + k]          (side s -> s + k, k <= s)
// so the levels k = 1, 2, 4, .. while 2 k <= L = 2 r + 1 reach side k, one level with the step L - k reaches L, and
// erode[x][y] = a[x - r][y - r].  The last level, the recentring and the subtraction from the mask are one kernel.
//   along y   the column of a word's x is a bit string of 64 R bits (word (x, q) holds rows 64 q .. 64 q + 63): "a[x][y + k]" for the 64
//             rows of a word is a 64-bit funnel shift over the two words that hold bits 64 q + k .. 64 q + k + 63 (col_bits).  k >= 64
//             moves whole words; positions outside [0, 64 R) read as zero.
//   along x   "a[x + k]" is the word k R further on; columns outside [0, w) read as zero.
// A level is one launch, a thread per word: at most 8 word loads (4 funnel shifts), 3 ANDs and one store per 64 pixels, and there are
// ceil(log2 L) + 1 levels at most - O(log r) per word, whatever r: no tile, so no radius is too large for one.  A level reads its input
// from another buffer than it writes (the levels alternate between the output and one temporary of the same size, the last one lands
// in the output); the neighbours of a word are a few words and k R words away, so of the loads of a level all but the first touch of a
// line hit L2: a mask's words come from memory once per level and are written once per level.
// Bits at or beyond row h in the last word of a column must be zero in the input: they stand for "outside the picture".  Every
// producer guarantees it - rle_pack_dense_kernel, rle_pack_x4_kernel and rle_pack_generic_kernel (rle.hip) set bit k of such a word
// only for k < h - 64 r, inst_decode_kernel (inst_eval.hip) clamps the bits it sets to p1 = x h + min(64 r + 64, h), and the polygon
// fill (poly_fill_kernel, poly.hip) masks the last word of a column to its h % 64 bits (inst_area_kernel and inst_box_kernel rely on the same).
// The levels keep them zero (they only AND), and the output is a subset of the input.
// 2 r + 1 > min(h, w): every window reaches outside, everything erodes, the boundary is the mask itself (one copying launch).
#include "inst_words.h"

namespace odise {

// bits p .. p + 63 of a column of R words (p of any sign); zero outside [0, 64 R)
__device__ __forceinline__ u64 col_bits(const u64* __restrict__ col, int R, long long p) {
    const long long q = p >> 6;   // floor
    const int s = (int)(p & 63);
    const u64 lo = (q >= 0 && q < R) ? col[q] : 0ull;
    if (s == 0) return lo;
    const u64 hi = (q + 1 >= 0 && q + 1 < R) ? col[q + 1] : 0ull;
    return (lo >> s) | (hi << (64 - s));
}
// the 64 rows from p on of a[x] & a[x + k] & a[x][. + k] & a[x + k][. + k]; zero when a column lies outside [0, w)
__device__ __forceinline__ u64 window4(const u64* __restrict__ a, const RleGrid& G, long long x, long long p, int k) {
    if (x < 0 || x + k >= G.w) return 0ull;
    const u64 *c0 = a + x * G.R, *c1 = a + (x + k) * G.R;
    u64 v = col_bits(c0, G.R, p) & col_bits(c1, G.R, p);
    if (v) v &= col_bits(c0, G.R, p + k) & col_bits(c1, G.R, p + k);
    return v;
}

// which mask and word a thread has; false: nothing to do.  The first topk masks are a selection: those past its count are `skipped`.
__device__ __forceinline__ bool boundary_word(const RleGrid& G, long long bpm, const int* __restrict__ inst_table, int topk, long long& i,
                                              long long& t, bool& skipped) {
    i = (long long)blockIdx.x / bpm;
    t = ((long long)blockIdx.x - i * bpm) * 256 + threadIdx.x;
    skipped = i < topk && i >= inst_count(inst_table, topk);
    return t < G.nw;
}

__global__ void __launch_bounds__(256) inst_erode_level_kernel(const u64* __restrict__ in, u64* __restrict__ out, RleGrid G, int k, long long bpm,
                                                              const int* __restrict__ inst_table, int topk) {
    long long i, t;
    bool skipped;
    if (!boundary_word(G, bpm, inst_table, topk, i, t, skipped) || skipped) return;
    const long long x = t / G.R, q = t - x * G.R;
    out[i * G.nw + t] = window4(in + i * G.nw, G, x, 64 * q, k);
}

// out = src & ~erode, erode[x][y] = the last level (step k) of `a` at (x - r, y - r); all: everything erodes (a is not read)
__global__ void __launch_bounds__(256) inst_boundary_last_kernel(const u64* __restrict__ src, const u64* __restrict__ a, u64* __restrict__ out, RleGrid G,
                                                                int k, int r, bool all, long long bpm, const int* __restrict__ inst_table, int topk) {
    long long i, t;
    bool skipped;
    if (!boundary_word(G, bpm, inst_table, topk, i, t, skipped)) return;
    if (skipped) {
        out[i * G.nw + t] = 0ull;
        return;
    }
    const u64 m = src[i * G.nw + t];
    u64 e = 0ull;
    if (!all && m) {
        const long long x = t / G.R, q = t - x * G.R;
        e = window4(a + i * G.nw, G, x - r, 64 * q - r, k);
    }
    out[i * G.nw + t] = m & ~e;
}

int inst_boundary_words(odise_hip_ctx* ctx, const u64* words_in, int n, const RleGrid& G, int r, const int* inst_table, int topk, u64* words_out,
                        u64* words_tmp) {
    if (n <= 0) return ODISE_OK;
    ODISE_REQUIRE(r >= 1, "boundary: radius %d", r);
    const long long bpm = ceil_div(G.nw, 256);
    ODISE_REQUIRE(bpm * n <= 0x7fffffffll, "boundary: %d masks of %lld words are too many for one grid", n, (long long)G.nw);
    const dim3 grid((unsigned)(bpm * n));
    const bool all = r > (std::min(G.h, G.w) - 1) / 2;
    int levels = 0;   // the doubling levels in front of the last one
    if (!all)
        for (int k = 1; 2ll * k <= 2ll * r + 1; k <<= 1) ++levels;
    const u64* cur = words_in;
    int k = 1;
    for (int j = 0; j < levels; ++j, k <<= 1) {   // level `levels - 1` writes the temporary, the one before it the output, ..
        u64* dst = ((levels - 1 - j) & 1) ? words_out : words_tmp;
        hipLaunchKernelGGL(inst_erode_level_kernel, grid, dim3(256), 0, ctx->stream, cur, dst, G, k, bpm, inst_table, topk);
        ODISE_CHECK_HIP(hipGetLastError());
        cur = dst;
    }
    hipLaunchKernelGGL(inst_boundary_last_kernel, grid, dim3(256), 0, ctx->stream, words_in, cur, words_out, G, all ? 0 : 2 * r + 1 - k, r, all, bpm,
                       inst_table, topk);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

// dense uint8 [n, h, w] of words [n][G.nw]: the pack of rle_pack_dense_kernel backwards, a thread per word (r, x), x fastest
__global__ void __launch_bounds__(256) inst_unpack_kernel(const u64* __restrict__ words, uint8_t* __restrict__ out, RleGrid G) {
    const int i = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= G.nw) return;
    const int r = (int)(t / G.w), x = (int)(t - (int64_t)r * G.w);
    const u64 v = words[(int64_t)i * G.nw + (int64_t)x * G.R + r];
    uint8_t* dst = out + (int64_t)i * G.h * G.w + (int64_t)64 * r * G.w + x;
    const int rows = min(64, G.h - 64 * r);
    for (int k = 0; k < rows; ++k) dst[(int64_t)k * G.w] = (uint8_t)((v >> k) & 1ull);
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_sizeof_inst_boundary_task(void) { return (int)sizeof(odise_inst_boundary_task); }

extern "C" int odise_hip_mask_boundary(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, int radius, uint8_t* boundary,
                                       int64_t* area) {
    ODISE_REQUIRE(ctx, "mask_boundary: null argument");
    ODISE_REQUIRE(n >= 0 && n <= 65535, "mask_boundary: %d masks (0..65535)", n);
    ODISE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kRleMaxPixels, "mask_boundary: mask size %dx%d out of range", h, w);
    ODISE_REQUIRE(dtype == ODISE_F32 || dtype == ODISE_U8, "mask_boundary: dtype %d (ODISE_F32 or ODISE_U8)", dtype);
    if (n == 0) return ODISE_OK;
    ODISE_REQUIRE(masks && boundary, "mask_boundary: null argument");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const RleGrid G = rle_grid(h, w);
    const size_t wb = (size_t)round_up((int64_t)n * G.nw * 8, 256);
    ODISE_TRY(scratch_reserve(ctx->rle, 3 * wb, 8, drain_streams(ctx->stream), "rle"));
    u64 *words = (u64*)ctx->rle.ptr, *bwords = (u64*)((char*)ctx->rle.ptr + wb), *tmp = (u64*)((char*)ctx->rle.ptr + 2 * wb);
    ODISE_TRY(rle_pack_dense(ctx, masks, dtype, n, G, words));
    ODISE_TRY(inst_boundary_words(ctx, words, n, G, radius > 0 ? radius : odise_hip_boundary_radius(h, w), nullptr, 0, bwords, tmp));
    hipLaunchKernelGGL(inst_unpack_kernel, dim3((unsigned)ceil_div(G.nw, 256), (unsigned)n), dim3(256), 0, ctx->stream, (const u64*)bwords, boundary, G);
    ODISE_CHECK_HIP(hipGetLastError());
    if (area) ODISE_TRY(inst_area_launch(ctx, bwords, n, G.nw, (long long*)area));
    return ODISE_OK;
}
