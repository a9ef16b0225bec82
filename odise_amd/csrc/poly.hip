// poly.hip — polygon annotations to bit-packed masks on the device: pycocotools' annToRLE (maskApi.c rleFrPoly for every polygon, rleMerge
// as a union), bit for bit.  odise_hip_polygon_rle hands the words to the string passes of rle.hip; odise_hip_instance_eval_poly
// (inst_eval.hip) rasterises polygon ground truth into the words its run-length decoder fills for the other masks.
//
// rleFrPoly, for k vertices on an h x w picture (doubles and ints, (int) truncates toward zero):
//   scale      X[j] = (int)(5 x_j + .5), Y[j] = (int)(5 y_j + .5), X[k] = X[0], Y[k] = Y[0]
//   walk       edge j: dx = |X[j+1] - X[j]|, dy = |Y[j] - Y[j+1]|; the ends are swapped when the edge runs backwards along its long axis
//              (flip); s = (ye - ys) / dx or (xe - xs) / dy; the edge emits max(dx, dy) + 1 points, point d at t = flip ? max - d : d:
//              (t + xs, (int)(ys + s t + .5)) or ((int)(xs + s t + .5), t + ys) - every edge from its first vertex to its second
//   crossings  for consecutive points of the list whose u differ: the column xd = ((u_i < u_p ? u_i : u_i - 1) + .5) / 5 - .5 when that is a
//              whole number in [0, w - 1], the row yd = ceil(clamp((min(v_i, v_p) + .5) / 5 - .5, 0, h)); position a = xd h + yd
//   runs       the sorted positions are the boundaries of the runs
// The mask is the parity of the crossings: pixel p of the column-major order is set iff an odd number of positions a <= p.  So nothing is
// sorted and no point list is stored:
//
//   One block works on one polygon at a time and walks the polygons of its annotation.
//   1. toggles  the edges are taken 1024 at a time: a block scan of the lengths max(dx, dy) + 1, then the threads stride over the flattened
//               point index of the chunk and search the edge that owns each point, so one long edge spreads over the whole block.  A point
//               recomputes its predecessor from the closed form.  The first point of an edge repeats the vertex the edge before ended
//               on (same u: never a crossing) and is passed over; so is the single point of a zero-length edge, whose slope would be 0 / 0.
//               A crossing is an atomic XOR of one bit of the block's toggle plane (exact and independent of order).  A crossing at y == h
//               belongs to (x + 1, 0) and is dropped in the last column.
//   2. parity   a thread owns a contiguous range of words: shift-XOR prefix inside a word, a block scan of the popcount parities of the
//               ranges in flat order for the carry (it runs across column boundaries); the last word of a column keeps its h % 64 bits.
//   3. union    the result is OR-ed into the annotation's words.
// The multiply and the add of ys + s t + .5 are rounded separately, as the x86 build of maskApi.c rounds them: contraction is off for the
// whole file (a fused multiply-add moves the truncation boundary on some inputs).
#include "rle_pack.h"

#pragma clang fp contract(off)

namespace odise {

typedef unsigned long long u64;

constexpr double kPolyScale = 5.0;
constexpr double kPolyMaxCoord = 67108864.0;   // 2^26: 5 x + .5 stays inside an int

struct PolyPoint { int u, v; };

// point d of the edge (x0, y0) -> (x1, y1), 0 <= d <= max(dx, dy), max(dx, dy) >= 1
__device__ __forceinline__ PolyPoint poly_point(int x0, int y0, int x1, int y1, int d) {
    int xs = x0, xe = x1, ys = y0, ye = y1;
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool wide = dx >= dy;
    const bool flip = (wide && xs > xe) || (!wide && ys > ye);
    if (flip) {
        int t;
        t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    const double s = wide ? (double)(ye - ys) / dx : (double)(xe - xs) / dy;
    const int t = flip ? (wide ? dx : dy) - d : d;
    PolyPoint p;
    if (wide) {
        p.u = t + xs;
        p.v = (int)(ys + s * t + .5);
    } else {
        p.v = t + ys;
        p.u = (int)(xs + s * t + .5);
    }
    return p;
}

__global__ void __launch_bounds__(kRleThreads) poly_fill_kernel(const double* __restrict__ xy, const long long* __restrict__ poly_offsets,
                                                               const int* __restrict__ ann_polys, int n_poly, RleGrid G, u64* __restrict__ words,
                                                               u64* __restrict__ toggle, int fill_empty, const long long* __restrict__ run_offsets,
                                                               int* __restrict__ flag) {
    __shared__ long long ends[kRleThreads];       // end of every edge of the chunk in the chunk's flattened point index
    __shared__ int sx[kRleThreads + 1], sy[kRleThreads + 1];
    __shared__ long long ls[kRleThreads / 64];
    const int tid = threadIdx.x, h = G.h, w = G.w;
    const int p_begin = min(max(ann_polys[blockIdx.x], 0), n_poly), p_end = min(max(ann_polys[blockIdx.x + 1], p_begin), n_poly);
    if (p_begin == p_end && !fill_empty) return;
    if (tid == 0 && p_begin < p_end && run_offsets && run_offsets[blockIdx.x + 1] > run_offsets[blockIdx.x]) atomicOr(flag, 4);
    u64* wd = words + (int64_t)blockIdx.x * G.nw;
    u64* tg = toggle + (int64_t)blockIdx.x * G.nw;
    const int64_t per = (G.nw + kRleThreads - 1) / kRleThreads;
    const int64_t wa = min(G.nw, (int64_t)tid * per), wb = min(G.nw, wa + per);   // the words this thread owns in steps 2 and 3
    for (int64_t i = wa; i < wb; ++i) wd[i] = 0ull;
    const int hl = h - 64 * (G.R - 1);   // rows in the last word of a column
    const u64 last = hl == 64 ? ~0ull : (1ull << hl) - 1ull;

    for (int p = p_begin; p < p_end; ++p) {
        const long long v0 = poly_offsets[p];
        const long long k = poly_offsets[p + 1] - v0;
        // a polygon that cannot be walked contributes nothing
        int bad = (v0 < 0 || k < 3) ? 1 : 0;
        if (!bad)
            for (long long j = tid; j < 2 * k; j += kRleThreads) {
                const double c = xy[2 * v0 + j];
                if (!(fabs(c) <= kPolyMaxCoord)) bad = 1;   // NaN fails the comparison too
            }
        if (__syncthreads_or(bad)) {
            if (tid == 0) atomicOr(flag, 8);
            continue;
        }
        for (int64_t i = wa; i < wb; ++i) tg[i] = 0ull;
        __syncthreads();
        // ---- 1. toggles
        for (long long c0 = 0; c0 < k; c0 += kRleThreads) {
            const int cl = (int)min((long long)kRleThreads, k - c0);   // edges c0 .. c0 + cl - 1, vertices c0 .. c0 + cl (vertex k = vertex 0)
            for (int j = tid; j <= cl; j += kRleThreads) {
                const long long vtx = c0 + j == k ? 0 : c0 + j;
                sx[j] = (int)(kPolyScale * xy[2 * (v0 + vtx)] + .5);
                sy[j] = (int)(kPolyScale * xy[2 * (v0 + vtx) + 1] + .5);
            }
            __syncthreads();
            const long long len = tid < cl ? (long long)max(abs(sx[tid + 1] - sx[tid]), abs(sy[tid + 1] - sy[tid])) + 1 : 0ll;
            long long total;
            const long long ex = block_scan_sum(len, ls, total);
            ends[tid] = ex + len;
            __syncthreads();
            for (long long q = tid; q < total; q += kRleThreads) {
                int lo = 0, hi = cl - 1;   // the edge that owns point q: the first whose end lies behind q
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ends[mid] > q) hi = mid;
                    else lo = mid + 1;
                }
                const int d = (int)(q - (lo ? ends[lo - 1] : 0ll));
                if (d == 0) continue;   // the vertex the edge before ended on, or a zero-length edge
                const PolyPoint a = poly_point(sx[lo], sy[lo], sx[lo + 1], sy[lo + 1], d - 1);
                const PolyPoint b = poly_point(sx[lo], sy[lo], sx[lo + 1], sy[lo + 1], d);
                if (a.u == b.u) continue;
                double xd = (double)(b.u < a.u ? b.u : b.u - 1);
                xd = (xd + .5) / kPolyScale - .5;
                if (floor(xd) != xd || xd < 0 || xd > w - 1) continue;
                double yd = (double)(b.v < a.v ? b.v : a.v);
                yd = (yd + .5) / kPolyScale - .5;
                if (yd < 0) yd = 0;
                else if (yd > h) yd = h;
                yd = ceil(yd);
                int x = (int)xd, y = (int)yd;   // 0 <= x <= w - 1, 0 <= y <= h
                if (y == h) {
                    if (x == w - 1) continue;
                    ++x;
                    y = 0;
                }
                atomicXor(&tg[(int64_t)x * G.R + (y >> 6)], 1ull << (y & 63));
            }
            __syncthreads();   // sx, sy, ends are rewritten by the next chunk
        }
        // ---- 2. parity, 3. union
        int par = 0;
        for (int64_t i = wa; i < wb; ++i) par ^= __popcll(__hip_atomic_load(&tg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 1;
        long long total;
        u64 carry = (block_scan_sum((long long)par, ls, total) & 1) ? ~0ull : 0ull;
        int r = wa < wb ? (int)(wa % G.R) : 0;
        for (int64_t i = wa; i < wb; ++i) {
            u64 v = __hip_atomic_load(&tg[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool odd = __popcll(v) & 1;
            v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16; v ^= v << 32;   // bit k = parity of bits 0 .. k
            v ^= carry;
            if (r == G.R - 1) v &= last;
            if (v) wd[i] |= v;
            if (odd) carry = ~carry;
            if (++r == G.R) r = 0;
        }
        __syncthreads();   // the toggle plane is zeroed for the next polygon
    }
}

int poly_fill_words(odise_hip_ctx* ctx, const double* xy, const int64_t* poly_offsets, const int32_t* ann_polys, int n_ann, int n_poly,
                    const RleGrid& G, unsigned long long* words, unsigned long long* toggle, bool fill_empty, const int64_t* run_offsets, int* flag) {
    hipLaunchKernelGGL(poly_fill_kernel, dim3((unsigned)n_ann), dim3(kRleThreads), 0, ctx->stream, xy, (const long long*)poly_offsets,
                       (const int*)ann_polys, n_poly, G, words, toggle, fill_empty ? 1 : 0, (const long long*)run_offsets, flag);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_polygon_rle(odise_hip_ctx* ctx, const double* xy, const int64_t* poly_offsets, const int32_t* ann_polys, int n_ann, int n_poly,
                                     int h, int w, void* rle, int64_t capacity, int64_t* offsets, int64_t* area, int32_t* flags) {
    ODISE_REQUIRE(ctx && offsets && flags, "polygon_rle: null argument");
    ODISE_REQUIRE(n_ann >= 0 && n_ann <= 65535, "polygon_rle: %d annotations (0..65535)", n_ann);
    ODISE_REQUIRE(n_poly >= 0, "polygon_rle: %d polygons", n_poly);
    ODISE_REQUIRE(n_ann == 0 || ann_polys, "polygon_rle: null annotation ranges");
    ODISE_REQUIRE(n_poly == 0 || (xy && poly_offsets), "polygon_rle: null polygons");
    ODISE_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kRleMaxPixels, "polygon_rle: mask size %dx%d out of range", h, w);
    ODISE_REQUIRE(capacity >= 0 && (rle || capacity == 0), "polygon_rle: capacity %lld without an output buffer", (long long)capacity);
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    if (n_ann == 0) {
        ODISE_CHECK_HIP(hipMemsetAsync(offsets, 0, sizeof(int64_t), ctx->stream));
        return ODISE_OK;
    }
    const RleGrid G = rle_grid(h, w);
    RleScratch s;
    ODISE_TRY(rle_scratch(ctx, n_ann, G, &s, (size_t)n_ann * G.nw * 8));
    ODISE_TRY(poly_fill_words(ctx, xy, poly_offsets, ann_polys, n_ann, n_poly, G, s.words, (u64*)s.extra, true, nullptr, (int*)flags));
    return rle_finish(ctx, s, G, n_ann, rle, capacity, offsets, area, nullptr);
}
