// rle.hip — COCO compressed RLE of binary masks on the device, for the segm evaluators of the reference's evaluation configs
// (configs/common/data/pano_open_d2_eval.py: COCOEvaluator / InstanceSegEvaluator(tasks=("segm",)) -> detectron2 instances_to_coco_json ->
// pycocotools mask.encode(np.array(mask[:, :, None], order="F", dtype="uint8")), counts.decode("utf-8")).  The string is maskApi.c's
// rleEncode + rleToString byte for byte:
//   runs over the column-major order j = x * h + y, cnts[0] = leading zeros (may be 0), then alternating runs of ones and zeros;
//   character stream: x = cnts[i] - (i > 2 ? cnts[i - 2] : 0), 5 bits per character low first, bit 0x20 = more follows, + 48.
//
//   1. pack    word (x, r) of a mask holds pixels (64 r .. 64 r + 63, x), bit k = row 64 r + k: the words of a column are consecutive runs of
//              the Fortran order, stored [n][w][R], R = ceil(h / 64).  A thread packs one word, consecutive threads take consecutive columns
//              (coalesced row reads).  odise_hip_instance_rle samples the pixels from the mask logits with the taps of
//              instance_masks(_x4)_kernel (post_sample.h): the fp32 [topk, oh, ow] tensor is never written.
//   2. count   one block per mask; thread t owns a contiguous range of words.  A transition is a pixel j whose value differs from pixel j - 1
//              (pixel -1 = 0); with P[0] = 0, the transitions P[1..T] and P[T+1] = h * w, cnts[i] = P[i+1] - P[i].  Character group i needs
//              cnts[i] and cnts[i-2], i.e. P[i-2 .. i+1], and is emitted by the thread that owns P[i+1]: a block scan of (transition count,
//              last three positions) gives each thread the three boundaries before its range, a second pass over the range sums the bytes of
//              the groups it emits, and a block scan of those gives its first byte in the mask's string.  Per-thread state is kept for 4.
//   3. offsets exclusive scan of the string lengths over the masks (one block).
//   4. write   when offsets[n] <= capacity, every thread writes the characters of its groups at offsets[i] + its first byte.
// Integer scans only, no atomics: the output is deterministic.
#include <string.h>

#include "inst_words.h"   // rle_pack.h (RleGrid, kRleThreads, block_scan_sum) and InstSource, whose check and pack launch live here

namespace odise {

struct RleTail {      // transitions of a range of words and the last three of their positions (q2 the newest; -1 where fewer)
    int c, q0, q1, q2;
};
struct RleState {     // a thread's view for the write pass: the boundaries before its range (P[0] included), its first byte in the string
    RleTail pre;
    long long byte0;
};

__device__ __forceinline__ RleTail tail_cat(const RleTail& l, const RleTail& r) {
    RleTail o;
    o.c = l.c + r.c;
    o.q2 = r.c >= 1 ? r.q2 : l.q2;
    o.q1 = r.c >= 2 ? r.q1 : r.c == 1 ? l.q2 : l.q1;
    o.q0 = r.c >= 3 ? r.q0 : r.c == 2 ? l.q2 : r.c == 1 ? l.q1 : l.q0;
    return o;
}

// exclusive block scan over the 1024 threads (wave scan by shuffles, then the 16 wave totals through LDS); the sum form is in rle_pack.h
__device__ RleTail block_scan_tail(const RleTail& v, RleTail* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    RleTail inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        RleTail u;
        u.c = __shfl_up(inc.c, o); u.q0 = __shfl_up(inc.q0, o); u.q1 = __shfl_up(inc.q1, o); u.q2 = __shfl_up(inc.q2, o);
        if (lane >= o) inc = tail_cat(u, inc);
    }
    RleTail ex;
    ex.c = __shfl_up(inc.c, 1); ex.q0 = __shfl_up(inc.q0, 1); ex.q1 = __shfl_up(inc.q1, 1); ex.q2 = __shfl_up(inc.q2, 1);
    if (lane == 0) ex = RleTail{0, -1, -1, -1};
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    RleTail pre = RleTail{0, -1, -1, -1};
    for (int k = 0; k < wave; ++k) pre = tail_cat(pre, lds[k]);
    __syncthreads();
    return tail_cat(pre, ex);
}
// f(position) for every transition in words [a, b) of one mask, in order; returns the ones in the range.  The words are loaded kRleBatch at a
// time (independent loads in flight): one load per loop trip made the walk a chain of memory latencies.
constexpr int kRleBatch = 8;
template <class F>
__device__ __forceinline__ long long rle_walk(const unsigned long long* __restrict__ wd, int64_t a, int64_t b, const RleGrid& G, F&& f) {
    if (a >= b) return 0;
    int x = (int)(a / G.R), r = (int)(a - (int64_t)x * G.R);
    const int hl = G.h - 64 * (G.R - 1);   // rows in the last word of a column
    const unsigned long long last = hl == 64 ? ~0ull : (1ull << hl) - 1ull;
    unsigned long long prev = a > 0 ? wd[a - 1] : 0ull;
    long long ones = 0;
    for (int64_t k0 = a; k0 < b; k0 += kRleBatch) {
        unsigned long long v[kRleBatch];
#pragma unroll
        for (int j = 0; j < kRleBatch; ++j) v[j] = k0 + j < b ? wd[k0 + j] : 0ull;
#pragma unroll
        for (int j = 0; j < kRleBatch; ++j) {
            if (k0 + j >= b) break;
            const unsigned long long carry = k0 + j == 0 ? 0ull : r > 0 ? prev >> 63 : (prev >> (hl - 1)) & 1ull;   // the pixel before bit 0
            unsigned long long tr = (v[j] ^ ((v[j] << 1) | carry)) & (r == G.R - 1 ? last : ~0ull);
            const int base = x * G.h + 64 * r;
            while (tr) {
                f(base + __ffsll((long long)tr) - 1);
                tr &= tr - 1ull;
            }
            ones += __popcll(v[j]);
            prev = v[j];
            if (++r == G.R) { r = 0; ++x; }
        }
    }
    return ones;
}

// the value rleToString encodes for the run that ends at each successive boundary
struct RleEmit {
    int a, b, c, k;   // P[k-3], P[k-2], P[k-1]; k = index of the next boundary
    __device__ explicit RleEmit(const RleTail& pre) : a(pre.q0), b(pre.q1), c(pre.q2), k(pre.c) {}
    __device__ long long next(int pos) {
        const int i = k - 1;   // cnts[i] = pos - P[k-1]
        long long x = (long long)pos - c;
        if (i > 2) x -= (long long)b - a;   // cnts[i-2] = P[k-2] - P[k-3]
        a = b; b = c; c = pos; ++k;
        return x;
    }
};
__device__ __forceinline__ int rle_chars(long long x) {
    int n = 0;
    bool more;
    do {
        const int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        ++n;
    } while (more);
    return n;
}
__device__ __forceinline__ char* rle_put(char* o, long long x) {
    bool more;
    do {
        int ch = (int)(x & 0x1f);
        x >>= 5;
        more = (ch & 0x10) ? x != -1 : x != 0;
        if (more) ch |= 0x20;
        *o++ = (char)(ch + 48);
    } while (more);
    return o;
}

// ---- 1. pack ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) rle_pack_dense_kernel(const T* __restrict__ m, unsigned long long* __restrict__ words, RleGrid G) {
    const int i = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (r, x), x fastest
    if (t >= G.nw) return;
    const int r = (int)(t / G.w), x = (int)(t - (int64_t)r * G.w);
    const T* src = m + (int64_t)i * G.h * G.w + (int64_t)64 * r * G.w + x;
    const int rows = min(64, G.h - 64 * r);
    unsigned long long v = 0ull;
    for (int k = 0; k < rows; ++k) v |= (unsigned long long)(src[(int64_t)k * G.w] != (T)0) << k;
    words[(int64_t)i * G.nw + (int64_t)x * G.R + r] = v;
}

// instance masks, x4 geometry: a thread packs the four columns of a cell column (the six taps of instance_masks_x4_kernel per row)
__global__ void __launch_bounds__(256) rle_pack_x4_kernel(const f16* __restrict__ logits, const int* __restrict__ idx, unsigned long long* __restrict__ words,
                                                         PostGeom g, RleGrid G, const int* __restrict__ n_dev) {
    const int i = blockIdx.y;
    if (n_dev && i >= *n_dev) return;
    const int cw = g.ow >> 2;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G.R * cw) return;
    const int r = t / cw, cx = t - r * cw;
    int cl, cr;
    x4_cols(g, cx, cl, cr);
    const f16* lr = logits + (int64_t)idx[i] * g.h4 * g.w4;
    const int y0 = 64 * r, rows = min(64, g.oh - y0);
    unsigned long long v0 = 0ull, v1 = 0ull, v2 = 0ull, v3 = 0ull;
#pragma unroll 2
    for (int k = 0; k < rows; ++k) {
        int ra, rb;
        float ty;
        x4_rows(g, y0 + k, ra, rb, ty);
        const float al = (float)lr[ra * g.w4 + cl], ac = (float)lr[ra * g.w4 + cx], ar = (float)lr[ra * g.w4 + cr];
        const float bl = (float)lr[rb * g.w4 + cl], bc = (float)lr[rb * g.w4 + cx], br = (float)lr[rb * g.w4 + cr];
        v0 |= (unsigned long long)(x4_pixel(0, ty, al, ac, ar, bl, bc, br) > 0.f) << k;
        v1 |= (unsigned long long)(x4_pixel(1, ty, al, ac, ar, bl, bc, br) > 0.f) << k;
        v2 |= (unsigned long long)(x4_pixel(2, ty, al, ac, ar, bl, bc, br) > 0.f) << k;
        v3 |= (unsigned long long)(x4_pixel(3, ty, al, ac, ar, bl, bc, br) > 0.f) << k;
    }
    unsigned long long* o = words + (int64_t)i * G.nw + (int64_t)4 * cx * G.R + r;
    o[0] = v0; o[G.R] = v1; o[2 * G.R] = v2; o[3 * G.R] = v3;
}

// instance masks, any geometry: sample_mask per pixel (instance_masks_kernel)
__global__ void __launch_bounds__(256) rle_pack_generic_kernel(const f16* __restrict__ logits, const int* __restrict__ idx,
                                                              unsigned long long* __restrict__ words, PostGeom g, RleGrid G, const int* __restrict__ n_dev) {
    const int i = blockIdx.y;
    if (n_dev && i >= *n_dev) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G.nw) return;
    const int r = (int)(t / G.w), x = (int)(t - (int64_t)r * G.w);
    const f16* lr = logits + (int64_t)idx[i] * g.h4 * g.w4;
    const int y0 = 64 * r, rows = min(64, g.oh - y0);
    unsigned long long v = 0ull;
    for (int k = 0; k < rows; ++k) v |= (unsigned long long)(sample_mask(lr, g, y0 + k, x) > 0.f) << k;
    words[(int64_t)i * G.nw + (int64_t)x * G.R + r] = v;
}

// ---- 2. count -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRleThreads) rle_count_kernel(const unsigned long long* __restrict__ words, RleGrid G, RleState* __restrict__ state,
                                                               long long* __restrict__ len, long long* __restrict__ area, const int* __restrict__ n_dev) {
    __shared__ RleTail lt[kRleThreads / 64];
    __shared__ long long ls[kRleThreads / 64];
    const int i = blockIdx.x, t = threadIdx.x;
    if (n_dev && i >= *n_dev) {   // past the selection's count: an empty string
        if (t == 0) {
            len[i] = 0;
            if (area) area[i] = 0;
        }
        return;
    }
    const unsigned long long* wd = words + (int64_t)i * G.nw;
    const int64_t per = (G.nw + kRleThreads - 1) / kRleThreads;
    const int64_t a = min(G.nw, (int64_t)t * per), b = min(G.nw, a + per);
    RleTail own = RleTail{0, -1, -1, -1};
    const long long ones = rle_walk(wd, a, b, G, [&](int pos) { own.q0 = own.q1; own.q1 = own.q2; own.q2 = pos; ++own.c; });
    const RleTail pre = tail_cat(RleTail{1, -1, -1, 0}, block_scan_tail(own, lt));   // P[0] = 0 leads
    RleEmit e(pre);
    long long bytes = 0;
    rle_walk(wd, a, b, G, [&](int pos) { bytes += rle_chars(e.next(pos)); });
    if (t == kRleThreads - 1) bytes += rle_chars(e.next(G.h * G.w));   // the last run ends at h * w
    long long total_bytes, total_ones;
    const long long byte0 = block_scan_sum(bytes, ls, total_bytes);
    (void)block_scan_sum(ones, ls, total_ones);
    state[(int64_t)i * kRleThreads + t] = RleState{pre, byte0};
    if (t == 0) {
        len[i] = total_bytes;
        if (area) area[i] = total_ones;
    }
}

// ---- 3. offsets ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRleThreads) rle_offsets_kernel(const long long* __restrict__ len, long long* __restrict__ offsets, int n) {
    __shared__ long long ls[kRleThreads / 64];
    long long carry = 0;
    for (int base = 0; base < n; base += kRleThreads) {
        const int i = base + threadIdx.x;
        long long total;
        const long long ex = block_scan_sum(i < n ? len[i] : 0ll, ls, total);
        if (i < n) offsets[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) offsets[n] = carry;
}

// ---- 4. write -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRleThreads) rle_write_kernel(const unsigned long long* __restrict__ words, RleGrid G, const RleState* __restrict__ state,
                                                               const long long* __restrict__ offsets, int n, char* __restrict__ out, long long capacity,
                                                               const int* __restrict__ n_dev) {
    const int i = blockIdx.x, t = threadIdx.x;
    if (n_dev && i >= *n_dev) return;
    if (offsets[n] > capacity) return;   // all or nothing: the caller retries with capacity >= offsets[n]
    const unsigned long long* wd = words + (int64_t)i * G.nw;
    const int64_t per = (G.nw + kRleThreads - 1) / kRleThreads;
    const int64_t a = min(G.nw, (int64_t)t * per), b = min(G.nw, a + per);
    const RleState s = state[(int64_t)i * kRleThreads + t];
    RleEmit e(s.pre);
    char* o = out + offsets[i] + s.byte0;
    rle_walk(wd, a, b, G, [&](int pos) { o = rle_put(o, e.next(pos)); });
    if (t == kRleThreads - 1) rle_put(o, e.next(G.h * G.w));
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
int rle_pack_dense(odise_hip_ctx* ctx, const void* masks, int dtype, int n, const RleGrid& G, unsigned long long* words) {
    const dim3 grid((unsigned)ceil_div(G.nw, 256), (unsigned)n);
    if (dtype == ODISE_F32) hipLaunchKernelGGL(rle_pack_dense_kernel<float>, grid, dim3(256), 0, ctx->stream, (const float*)masks, words, G);
    else hipLaunchKernelGGL(rle_pack_dense_kernel<uint8_t>, grid, dim3(256), 0, ctx->stream, (const uint8_t*)masks, words, G);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

int inst_geom(odise_hip_ctx* ctx, const char* what, const InstSource& s, InstGeom* ig) {
    ig->logits = nullptr;
    if (s.masks) return ODISE_OK;
    const int b = s.b, pad_h = s.pad_h, pad_w = s.pad_w, img_h = s.img_h, img_w = s.img_w, out_h = s.h, out_w = s.w;
    PostGeom* g = &ig->g;
    ModelStore* ms = store_of(ctx);
    HeadOutputs ho;
    ODISE_TRY(head_outputs(ms, &ho));
    ODISE_REQUIRE(b >= 0 && b < ho.B, "%s: image index %d out of range", what, b);
    ODISE_REQUIRE(pad_h == 4 * ho.h4 && pad_w == 4 * ho.w4, "%s: padded size %dx%d does not match the mask logits (%dx%d x 4)", what, pad_h, pad_w,
                  ho.h4, ho.w4);
    ODISE_REQUIRE(img_h >= 1 && img_w >= 1 && img_h <= pad_h && img_w <= pad_w && out_h >= 1 && out_w >= 1 && (int64_t)out_h * out_w <= kRleMaxPixels,
                  "%s: bad geometry (image %dx%d, padded %dx%d, output %dx%d)", what, img_h, img_w, pad_h, pad_w, out_h, out_w);
    g->h4 = ho.h4; g->w4 = ho.w4; g->ph = pad_h; g->pw = pad_w; g->ih = img_h; g->iw = img_w; g->oh = out_h; g->ow = out_w;
    g->Q = ho.Q; g->Qpad = (int)round_up(ho.Q, 8);
    ig->logits = ho.pred_masks + (size_t)b * ho.Q * ho.h4 * ho.w4;
    return ODISE_OK;
}

// words [topk][G.nw] of the selection inst_table = n | query index [topk] | .., sampled from the mask logits with the taps of
// instance_masks(_x4)_kernel; masks past the count n (read on the device) are not written
static int rle_pack_logits(odise_hip_ctx* ctx, const f16* logits, const int* inst_table, int topk, const PostGeom& g, const RleGrid& G,
                           unsigned long long* words) {
    if (instance_masks_x4(g)) {
        const dim3 grid((unsigned)ceil_div((int64_t)G.R * (g.ow / 4), 256), (unsigned)topk);
        hipLaunchKernelGGL(rle_pack_x4_kernel, grid, dim3(256), 0, ctx->stream, logits, inst_table + 1, words, g, G, inst_table);
    } else {
        const dim3 grid((unsigned)ceil_div(G.nw, 256), (unsigned)topk);
        hipLaunchKernelGGL(rle_pack_generic_kernel, grid, dim3(256), 0, ctx->stream, logits, inst_table + 1, words, g, G, inst_table);
    }
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

int inst_source_check(const char* what, const InstSource& s, bool need_table, int64_t max_pixels, int max_topk) {
    ODISE_REQUIRE((s.inst_table && s.inst_scores) || (s.masks && !need_table), "%s: null inst_table / inst_scores (optional only with dense masks)", what);
    ODISE_REQUIRE(s.topk >= 1 && s.topk <= max_topk, "%s: topk %d (1..%d)", what, s.topk, max_topk);
    ODISE_REQUIRE(s.h >= 1 && s.w >= 1 && (int64_t)s.h * s.w <= max_pixels, "%s: mask size %dx%d out of range", what, s.h, s.w);
    ODISE_REQUIRE(!s.masks || s.dtype == ODISE_F32 || s.dtype == ODISE_U8, "%s: dtype %d (ODISE_F32 or ODISE_U8)", what, s.dtype);
    ODISE_REQUIRE((((uintptr_t)s.inst_table | (uintptr_t)s.inst_scores) & 3) == 0, "%s: inst_table / inst_scores must be 4-byte aligned", what);
    return ODISE_OK;
}

int inst_pack(odise_hip_ctx* ctx, const InstSource& s, const InstGeom& ig, const RleGrid& G, u64* words) {
    if (s.masks) return rle_pack_dense(ctx, s.masks, s.dtype, s.topk, G, words);
    return rle_pack_logits(ctx, ig.logits, s.inst_table, s.topk, ig.g, G, words);
}

int rle_scratch(odise_hip_ctx* ctx, int n, const RleGrid& G, RleScratch* s, size_t extra) {
    const size_t wb = (size_t)round_up((int64_t)n * G.nw * 8, 256), sb = (size_t)round_up((int64_t)n * kRleThreads * sizeof(RleState), 256);
    const size_t lb = (size_t)round_up((int64_t)n * 8, 256);
    ODISE_TRY(scratch_reserve(ctx->rle, wb + sb + lb + extra, 8, drain_streams(ctx->stream), "rle"));
    char* p = (char*)ctx->rle.ptr;
    s->words = (unsigned long long*)p;
    s->state = (RleState*)(p + wb);
    s->len = (long long*)(p + wb + sb);
    s->extra = p + wb + sb + lb;
    return ODISE_OK;
}

int rle_finish(odise_hip_ctx* ctx, const RleScratch& s, const RleGrid& G, int n, void* rle, int64_t capacity, int64_t* offsets, int64_t* area,
               const int* n_dev) {
    hipLaunchKernelGGL(rle_count_kernel, dim3((unsigned)n), dim3(kRleThreads), 0, ctx->stream, s.words, G, s.state, s.len, (long long*)area, n_dev);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rle_offsets_kernel, dim3(1), dim3(kRleThreads), 0, ctx->stream, s.len, (long long*)offsets, n);
    ODISE_CHECK_HIP(hipGetLastError());
    if (capacity > 0) {
        hipLaunchKernelGGL(rle_write_kernel, dim3((unsigned)n), dim3(kRleThreads), 0, ctx->stream, s.words, G, s.state, (const long long*)offsets, n,
                           (char*)rle, (long long)capacity, n_dev);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_rle_encode(odise_hip_ctx* ctx, const void* masks, int dtype, int n, int h, int w, void* rle, int64_t capacity, int64_t* offsets,
                                    int64_t* area) {
    ODISE_REQUIRE(ctx && offsets, "rle_encode: null argument");
    ODISE_REQUIRE(n >= 0 && n <= 65535, "rle_encode: %d masks (0..65535)", n);
    ODISE_REQUIRE(n == 0 || masks, "rle_encode: null masks");
    ODISE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kRleMaxPixels, "rle_encode: mask size %dx%d out of range", h, w);
    ODISE_REQUIRE(dtype == ODISE_F32 || dtype == ODISE_U8, "rle_encode: dtype %d (ODISE_F32 or ODISE_U8)", dtype);
    ODISE_REQUIRE(capacity >= 0 && (rle || capacity == 0), "rle_encode: capacity %lld without an output buffer", (long long)capacity);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    if (n == 0) {
        ODISE_CHECK_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), ctx->stream));
        return ODISE_OK;
    }
    const RleGrid G = rle_grid(h, w);
    RleScratch s;
    ODISE_TRY(rle_scratch(ctx, n, G, &s));
    ODISE_TRY(rle_pack_dense(ctx, masks, dtype, n, G, s.words));
    return rle_finish(ctx, s, G, n, rle, capacity, offsets, area, nullptr);
}

extern "C" int odise_hip_instance_rle(odise_hip_ctx* ctx, int b, const int* inst_table, int topk, int pad_h, int pad_w, int img_h, int img_w, int out_h,
                                      int out_w, void* rle, int64_t capacity, int64_t* offsets, int64_t* area) {
    ODISE_REQUIRE(ctx && inst_table && offsets, "instance_rle: null argument");
    ODISE_REQUIRE(topk >= 1 && topk <= 4096, "instance_rle: topk %d out of range", topk);
    ODISE_REQUIRE(capacity >= 0 && (rle || capacity == 0), "instance_rle: capacity %lld without an output buffer", (long long)capacity);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const InstSource src = {out_h, out_w, nullptr, 0, b, pad_h, pad_w, img_h, img_w, inst_table, nullptr, topk};
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, "instance_rle", src, &ig));
    const RleGrid G = rle_grid(out_h, out_w);
    RleScratch s;
    ODISE_TRY(rle_scratch(ctx, topk, G, &s));
    ODISE_TRY(inst_pack(ctx, src, ig, G, s.words));
    return rle_finish(ctx, s, G, topk, rle, capacity, offsets, area, inst_table);
}
