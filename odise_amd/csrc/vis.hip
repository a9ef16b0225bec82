// vis.hip — drawing a panoptic result: the pieces of a segment, where its label goes, the coloured picture
// (odise_hip_connected_components / odise_hip_segment_anchors / odise_hip_panoptic_overlay; host restatement: odise_amd/visualize.py).
//
// Connected components (8-connectivity, root = the smallest row-major index of the component) are a block-based union-find in three
// launches; the array being built is `roots` itself:
//
//   cc_tile_kernel     one block per 32 x 32 tile: labels and parents in LDS, every pixel is joined to its W / NW / N / NE neighbour of
//                      the tile by an LDS atomicMin union, then points at the tile-local root, written as a GLOBAL pixel index.
//   cc_merge_kernel    one thread per pixel of a tile's first column / first row: joined to its (up to three) neighbours across the
//                      border by the same union on `roots` - atomicMin for the links, agent-scope relaxed loads for the walks, so a
//                      walk never reads a line this CU cached before another CU's link.
//   cc_flatten_kernel  every pixel walks to its root.
//
// A parent is never larger than its child, so every walk strictly descends and ends; a link only ever replaces a root's own index by a
// smaller index of the same component, so the pixel of smallest index stays a root and is the only one: the result does not depend on
// the order the unions ran in.
//
// Anchors: areas of the components (integer atomics, a wave that lies in one component adds once), the best component of every stuff row
// (a 64-bit atomicMax of area | inverted root) and the area of every thing row from the root pixels, the list of (row, root, area) that
// the rules select, its order by counting smaller keys, then one pass that adds every pixel of an anchor to the anchor's column and row
// histogram, and a wave per (anchor, axis) that scans the histogram for the two middle elements and the first / last occupied bin.
#include <algorithm>

#include "common.h"
#include "record.h"     // the table of the record: rows, loader, search, a lane's last translation
#include "rgb.h"        // packed pixels and the blend: shared with vis_inst.hip
#include "vis_scan.h"   // vis_scan_middle, vis_anchor_row, vis_check_size: shared with vis_inst.hip

namespace odise {

constexpr int kCcTile = 32;                       // tile side
constexpr int kCcTilePix = kCcTile * kCcTile;
constexpr int kVisThreads = 256;

template <bool LDS>
__device__ __forceinline__ int cc_load(const int* p) {
    return LDS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root above x: strictly descending, so it ends on any memory content
template <bool LDS>
__device__ __forceinline__ int cc_find(const int* par, int x) {
    for (;;) {
        const int p = cc_load<LDS>(par + x);
        if (p >= x || p < 0) return x;
        x = p;
    }
}

// a and b are pixels of one component.  The larger root is linked below the smaller one; when the atomicMin finds that the larger one
// had been linked meanwhile, its former parent and b still have to meet.  a + b strictly decreases from round to round.
template <bool LDS>
__device__ __forceinline__ void cc_union(int* par, int a, int b) {
    for (;;) {
        a = cc_find<LDS>(par, a);
        b = cc_find<LDS>(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a || old < 0) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kVisThreads) cc_tile_kernel(const int* __restrict__ labels, int H, int W, int ntx, int* __restrict__ roots) {
    __shared__ int lab[kCcTilePix];
    __shared__ int par[kCcTilePix];
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int x0 = tx * kCcTile, y0 = ty * kCcTile;
    for (int li = threadIdx.x; li < kCcTilePix; li += kVisThreads) {
        const int gx = x0 + (li & (kCcTile - 1)), gy = y0 + (li >> 5);
        const int l = (gx < W && gy < H) ? labels[gy * W + gx] : 0;   // gy * W + gx < H * W <= 2^29 - 1
        lab[li] = l;
        par[li] = l > 0 ? li : -1;
    }
    __syncthreads();
    for (int li = threadIdx.x; li < kCcTilePix; li += kVisThreads) {
        const int l = lab[li];
        if (l <= 0) continue;
        const int lx = li & (kCcTile - 1), ly = li >> 5;
        if (lx > 0 && lab[li - 1] == l) cc_union<true>(par, li, li - 1);
        if (ly > 0) {
            if (lab[li - kCcTile] == l) cc_union<true>(par, li, li - kCcTile);
            if (lx > 0 && lab[li - kCcTile - 1] == l) cc_union<true>(par, li, li - kCcTile - 1);
            if (lx < kCcTile - 1 && lab[li - kCcTile + 1] == l) cc_union<true>(par, li, li - kCcTile + 1);
        }
    }
    __syncthreads();
    for (int li = threadIdx.x; li < kCcTilePix; li += kVisThreads) {
        const int gx = x0 + (li & (kCcTile - 1)), gy = y0 + (li >> 5);
        if (gx >= W || gy >= H) continue;
        int r = -1;
        if (lab[li] > 0) {
            const int t = cc_find<true>(par, li);   // local order = global order inside a tile: the local minimum is the global one
            r = (y0 + (t >> 5)) * W + x0 + (t & (kCcTile - 1));
        }
        roots[gy * W + gx] = r;
    }
}

__device__ __forceinline__ void cc_join(const int* __restrict__ labels, int* roots, int H, int W, int p, int l, int qx, int qy) {
    if (qx < 0 || qx >= W || qy < 0 || qy >= H) return;
    const int q = qy * W + qx;
    if (labels[q] == l) cc_union<false>(roots, p, q);
}

__global__ void __launch_bounds__(kVisThreads) cc_merge_kernel(const int* __restrict__ labels, int H, int W, int64_t n_vert, int64_t n_all, int* roots) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += stride) {
        if (i < n_vert) {                       // first column of tile column 1 + i / H
            const int bx = (int)(i / H), y = (int)(i - (int64_t)bx * H), x = (bx + 1) * kCcTile;
            const int p = y * W + x, l = labels[p];
            if (l <= 0) continue;
            cc_join(labels, roots, H, W, p, l, x - 1, y);
            cc_join(labels, roots, H, W, p, l, x - 1, y - 1);
            cc_join(labels, roots, H, W, p, l, x - 1, y + 1);
        } else {                                // first row of tile row 1 + j / W
            const int64_t j = i - n_vert;
            const int by = (int)(j / W), x = (int)(j - (int64_t)by * W), y = (by + 1) * kCcTile;
            const int p = y * W + x, l = labels[p];
            if (l <= 0) continue;
            cc_join(labels, roots, H, W, p, l, x, y - 1);
            cc_join(labels, roots, H, W, p, l, x - 1, y - 1);
            cc_join(labels, roots, H, W, p, l, x + 1, y - 1);
        }
    }
}

// Other threads store final roots while this one walks: a walk that meets one reads a root, which is where it was going.
__global__ void __launch_bounds__(kVisThreads) cc_flatten_kernel(int npix, int* roots) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const int r = cc_load<false>(roots + i);
        if (r < 0) continue;
        const int t = cc_find<false>(roots, r);
        if (t != r) __hip_atomic_store(roots + i, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static int cc_enqueue(odise_hip_ctx* ctx, const int* labels, int H, int W, int* roots) {
    const int ntx = (int)ceil_div(W, kCcTile), nty = (int)ceil_div(H, kCcTile);
    hipLaunchKernelGGL(cc_tile_kernel, dim3(ntx * nty), dim3(kVisThreads), 0, ctx->stream, labels, H, W, ntx, roots);
    ODISE_CHECK_HIP(hipGetLastError());
    const int64_t n_vert = (int64_t)(ntx - 1) * H, n_all = n_vert + (int64_t)(nty - 1) * W;
    if (n_all > 0) {
        hipLaunchKernelGGL(cc_merge_kernel, dim3(grid_blocks(ctx, n_all, kVisThreads)), dim3(kVisThreads), 0, ctx->stream, labels, H, W, n_vert, n_all, roots);
        ODISE_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_blocks(ctx, (int64_t)H * W, kVisThreads)), dim3(kVisThreads), 0, ctx->stream, H * W, roots);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

// ---- anchors ----------------------------------------------------------------------------------------------------------------------

struct VisState {                                        // zeroed at the start of every call
    unsigned long long best[ODISE_MAX_SEGMENTS];         // stuff row: max of (area << 32 | 0x7fffffff - root) over its components
    int seg_area[ODISE_MAX_SEGMENTS];                    // thing row: its pixels
    int thing_anchor[ODISE_MAX_SEGMENTS];                // thing row: 1 + its anchor
    int count;                                           // entries of the list
    int pad[3];
};
static_assert(sizeof(VisState) % 16 == 0, "the state is cleared together with the histograms behind it");

struct VisTable {   // the n rows of the record, by record_load
    int id[ODISE_MAX_SEGMENTS];
    int thing[ODISE_MAX_SEGMENTS];
};

// the first row that holds `id`; -1 for VOID (id <= 0) and for an id without a row
__device__ __forceinline__ int vis_row(const VisTable& T, int n, int id) { return id <= 0 ? -1 : record_find(T.id, n, id); }

// area[root] = pixels of the component.  A wave whose 64 pixels lie in one component adds once.
__global__ void __launch_bounds__(kVisThreads) vis_area_kernel(const int* __restrict__ roots, int npix, int* __restrict__ area) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npix; base += stride) {   // wave-uniform
        const int64_t p = base + lane;
        const int r = p < npix ? roots[p] : -1;
        const int r0 = __builtin_amdgcn_readfirstlane(r);
        if (__all(r == r0)) {
            if (lane == 0 && r0 >= 0) atomicAdd(area + r0, 64);
        } else if (r >= 0) {
            atomicAdd(area + r, 1);
        }
    }
}

__global__ void __launch_bounds__(kVisThreads) vis_root_kernel(const int* __restrict__ ids, const int* __restrict__ seg, const int* __restrict__ roots,
                                                              const int* __restrict__ area, int npix, VisState* __restrict__ st) {
    __shared__ VisTable T;
    const int n = record_rows(seg);
    record_load(seg, n, T.id, T.thing);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += stride) {
        if (roots[p] != (int)p) continue;
        const int s = vis_row(T, n, ids[p]);
        if (s < 0) continue;
        if (T.thing[s]) atomicAdd(&st->seg_area[s], area[p]);
        else atomicMax(&st->best[s], ((unsigned long long)(unsigned)area[p] << 32) | (unsigned)(0x7fffffff - (int)p));
    }
}

// list of int4 (row, root, area, 0): the selected components of the stuff rows and, from the n extra indices, the thing rows with a pixel
__global__ void __launch_bounds__(kVisThreads) vis_select_kernel(const int* __restrict__ ids, const int* __restrict__ seg, const int* __restrict__ roots,
                                                                const int* __restrict__ area, int npix, int small_area, int large_area,
                                                                VisState* __restrict__ st, int4* __restrict__ list, int list_cap) {
    __shared__ VisTable T;
    const int n = record_rows(seg);
    record_load(seg, n, T.id, T.thing);
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, total = (int64_t)npix + n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        int4 e;
        if (i < npix) {
            if (roots[i] != (int)i) continue;
            const int s = vis_row(T, n, ids[i]);
            if (s < 0 || T.thing[s]) continue;
            const unsigned long long b = st->best[s];
            const int best_area = (int)(b >> 32), best_root = 0x7fffffff - (int)(unsigned)b;
            const int a = area[i];
            if (best_area < small_area || !((int)i == best_root || a > large_area)) continue;
            e = make_int4(s, (int)i, a, 0);
        } else {
            const int s = (int)(i - npix);
            if (!T.thing[s] || st->seg_area[s] <= 0) continue;
            e = make_int4(s, 0, st->seg_area[s], 0);
        }
        const int k = atomicAdd(&st->count, 1);
        if (k < list_cap) list[k] = e;            // list_cap bounds the count (vis_list_cap): the test never fails
    }
}

// The place of an entry = the entries with a smaller (row, root).  Writes the head of its anchor row and tells the pixels of the anchor
// where to count: a thing row through thing_anchor, a component through area[root] = ~anchor (areas of the others stay positive).
__global__ void __launch_bounds__(kVisThreads) vis_rank_kernel(const int* __restrict__ seg, VisState* __restrict__ st, const int4* __restrict__ list,
                                                              int list_cap, int* __restrict__ area, odise_anchor_row* __restrict__ anchors, int cap,
                                                              int* __restrict__ n_anchors) {
    const int cnt = min(st->count, list_cap);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += stride) {
        const int4 e = list[i];
        const unsigned long long key = ((unsigned long long)(unsigned)e.x << 32) | (unsigned)e.y;
        int rank = 0;
        for (int j = 0; j < cnt; ++j) {
            const int4 f = list[j];
            rank += ((((unsigned long long)(unsigned)f.x << 32) | (unsigned)f.y) < key) ? 1 : 0;
        }
        if (record_isthing(seg, e.x)) st->thing_anchor[e.x] = rank + 1;
        else area[e.y] = ~rank;
        if (rank < cap) anchors[rank] = vis_anchor_row(e.x, e.z);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_anchors = cnt;
}

// hist [hcap][W + H]: columns, then rows, of the pixels of every anchor below hcap.  A wave that lies in one picture row of one anchor
// adds its 64 to the row bin once.
__global__ void __launch_bounds__(kVisThreads) vis_hist_kernel(const int* __restrict__ ids, const int* __restrict__ seg, const int* __restrict__ roots,
                                                              const int* __restrict__ area, const VisState* __restrict__ st, int H, int W, int hcap,
                                                              int* __restrict__ hist) {
    __shared__ VisTable T;
    const int n = record_rows(seg);
    record_load(seg, n, T.id, T.thing);
    __syncthreads();
    const int lane = threadIdx.x & 63, npix = H * W;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, bins = (int64_t)W + H;
    RecordMemo M = {0, -1};   // VOID has no row
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < npix; base += stride) {   // wave-uniform
        const int64_t p = base + lane;
        int a = -1, x = 0, y = -1;
        if (p < npix) {
            const int row = record_memo(M, ids[p], [&](int id) { return vis_row(T, n, id); });
            if (row >= 0) {
                if (T.thing[row]) a = st->thing_anchor[row] - 1;
                else { const int v = area[roots[p]]; a = v < 0 ? ~v : -1; }
                if (a >= hcap) a = -1;
            }
            y = (int)(p / W);
            x = (int)(p - (int64_t)y * W);
        }
        if (a >= 0) atomicAdd(hist + a * bins + x, 1);
        const int a0 = __builtin_amdgcn_readfirstlane(a), y0 = __builtin_amdgcn_readfirstlane(y);
        if (__all(a == a0 && y == y0)) {
            if (lane == 0 && a0 >= 0) atomicAdd(hist + a0 * bins + W + y0, 64);
        } else if (a >= 0) {
            atomicAdd(hist + a * bins + W + y, 1);
        }
    }
}

// One wave per (anchor, axis): the two middle elements of the sorted coordinates (twice the median is their sum) and the first / last
// occupied bin, by the scan of vis_scan.h.
__global__ void __launch_bounds__(64) vis_median_kernel(const VisState* __restrict__ st, const int* __restrict__ hist, int H, int W, int hcap, int cap,
                                                       odise_anchor_row* __restrict__ anchors) {
    const int a = blockIdx.x >> 1, axis = blockIdx.x & 1, lane = threadIdx.x;
    if (a >= st->count || a >= hcap || a >= cap) return;
    const int nb = axis ? H : W;
    const int* h = hist + (int64_t)a * ((int64_t)W + H) + (axis ? W : 0);
    int m1, m2, lo, hi;
    vis_scan_middle(h, nb, anchors[a].area, lane, m1, m2, lo, hi);   // vis_scan.h
    if (lane == 0) {
        if (axis) { anchors[a].y2 = m1 + m2; anchors[a].y0 = lo; anchors[a].y1 = hi; }
        else { anchors[a].x2 = m1 + m2; anchors[a].x0 = lo; anchors[a].x1 = hi; }
    }
}

// every selected component but the largest of its row has more than large_area pixels
static int64_t vis_list_cap(int64_t npix, int large_area) { return ODISE_MAX_SEGMENTS + npix / ((int64_t)std::max(large_area, 0) + 1); }

// ---- overlay ----------------------------------------------------------------------------------------------------------------------

struct OverlayTable {
    VisTable T;
    unsigned crb[ODISE_MAX_SEGMENTS], cg[ODISE_MAX_SEGMENTS];   // the colour of a row as blend_rgb takes it
};

// the pixel p = y * W + x with the bytes `in` (r | g << 8 | b << 16)
__device__ __forceinline__ unsigned overlay_pixel(const OverlayTable& S, int n, RecordMemo& M, const int* __restrict__ ids, int H, int W, int p, int x,
                                                  int y, unsigned in, int alpha, unsigned edge) {
    const int id = ids[p];
    const int s = record_memo(M, id, [&](int v) { return vis_row(S.T, n, v); });
    if (s < 0) return in;
    if ((x > 0 && ids[p - 1] != id) || (x < W - 1 && ids[p + 1] != id) || (y > 0 && ids[p - W] != id) || (y < H - 1 && ids[p + W] != id)) return edge;
    return blend_rgb(in, (unsigned)(256 - alpha), S.crb[s], S.cg[s]);
}

// vec != 0: image and out are 4-byte aligned and groups of four pixels travel as three dwords.  A lane reads its own pixels before it
// writes them and no other lane reads them, so out == image is safe.
__global__ void __launch_bounds__(kVisThreads) overlay_kernel(const uint8_t* image, const int* __restrict__ ids, const int* __restrict__ seg,
                                                             const uint8_t* __restrict__ colors, int H, int W, int alpha, unsigned edge, int vec,
                                                             uint8_t* out) {
    __shared__ OverlayTable S;
    const int n = record_rows(seg);
    record_load(seg, n, S.T.id, S.T.thing);
    for (int i = threadIdx.x; i < n; i += blockDim.x) blend_color(rgb_load(colors + 3 * i), (unsigned)alpha, S.crb[i], S.cg[i]);
    __syncthreads();
    RecordMemo M = {0, -1};   // VOID has no row
    const int npix = H * W, groups = vec ? npix >> 2 : 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += stride) {
        const unsigned* src = (const unsigned*)image + 3 * q;    // bytes 12 q .. 12 q + 11 < 3 npix
        unsigned px[4];
        rgb4_unpack(src[0], src[1], src[2], px);
        const int p0 = (int)(4 * q);
        int y = p0 / W, x = p0 - y * W;
        for (int k = 0; k < 4; ++k) {
            px[k] = overlay_pixel(S, n, M, ids, H, W, p0 + k, x, y, px[k], alpha, edge);
            if (++x == W) { x = 0; ++y; }
        }
        rgb4_pack(px, (unsigned*)out + 3 * q);
    }
    for (int64_t i = (int64_t)groups * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += stride) {
        const int p = (int)i, y = p / W, x = p - y * W;
        rgb_store(out + 3 * i, overlay_pixel(S, n, M, ids, H, W, p, x, y, rgb_load(image + 3 * i), alpha, edge));
    }
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_connected_components(odise_hip_ctx* ctx, const int32_t* labels, int H, int W, int32_t* roots) {
    ODISE_REQUIRE(ctx, "connected_components: null context");
    ODISE_REQUIRE(labels && roots, "connected_components: null pointer");
    ODISE_TRY(vis_check_size("connected_components", H, W));
    ODISE_REQUIRE((((uintptr_t)labels | (uintptr_t)roots) & 3) == 0, "connected_components: int32 buffers must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    return cc_enqueue(ctx, (const int*)labels, H, W, (int*)roots);
}

extern "C" int odise_hip_segment_anchors(odise_hip_ctx* ctx, const odise_anchor_desc* d) {
    ODISE_REQUIRE(ctx, "segment_anchors: null context");
    ODISE_REQUIRE(d, "segment_anchors: null descriptor");
    ODISE_REQUIRE(d->pred_ids && d->pred_segments && d->anchors && d->n_anchors, "segment_anchors: null pointer");
    ODISE_TRY(vis_check_size("segment_anchors", d->H, d->W));
    ODISE_REQUIRE(d->cap >= 0, "segment_anchors: cap %d", d->cap);
    ODISE_REQUIRE((((uintptr_t)d->pred_ids | (uintptr_t)d->pred_segments | (uintptr_t)d->anchors | (uintptr_t)d->n_anchors) & 3) == 0,
                  "segment_anchors: int32 buffers must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const int H = d->H, W = d->W, npix = H * W;
    const int64_t list_cap64 = vis_list_cap(npix, d->large_area);
    const int list_cap = (int)std::min<int64_t>(list_cap64, INT32_MAX);
    const int hcap = std::min(d->cap, list_cap);
    // [state | histograms | areas] are cleared together; [roots | list] are written before they are read
    const size_t hist_b = (size_t)round_up((int64_t)hcap * ((int64_t)W + H) * 4, 16), area_b = (size_t)round_up((int64_t)npix * 4, 16);
    const size_t clear_b = sizeof(VisState) + hist_b + area_b, list_b = (size_t)list_cap * sizeof(int4);
    ODISE_TRY(scratch_reserve(ctx->vis, clear_b + area_b + list_b, 8, drain_streams(ctx->stream), "segment_anchors"));
    char* base = (char*)ctx->vis.ptr;
    VisState* st = (VisState*)base;
    int* hist = (int*)(base + sizeof(VisState));
    int* area = (int*)(base + sizeof(VisState) + hist_b);
    int* roots = (int*)(base + clear_b);
    int4* list = (int4*)(base + clear_b + area_b);
    const int* ids = (const int*)d->pred_ids;
    const int* seg = (const int*)d->pred_segments;
    ODISE_CHECK_HIP(hipMemsetAsync(base, 0, clear_b, ctx->stream));
    ODISE_TRY(cc_enqueue(ctx, ids, H, W, roots));
    const int pb = grid_blocks(ctx, npix, kVisThreads);
    hipLaunchKernelGGL(vis_area_kernel, dim3(pb), dim3(kVisThreads), 0, ctx->stream, (const int*)roots, npix, area);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(vis_root_kernel, dim3(pb), dim3(kVisThreads), 0, ctx->stream, ids, seg, (const int*)roots, (const int*)area, npix, st);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(vis_select_kernel, dim3(grid_blocks(ctx, (int64_t)npix + ODISE_MAX_SEGMENTS, kVisThreads)), dim3(kVisThreads), 0, ctx->stream, ids, seg,
                       (const int*)roots, (const int*)area, npix, d->small_area, d->large_area, st, list, list_cap);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(vis_rank_kernel, dim3(grid_blocks(ctx, list_cap, kVisThreads)), dim3(kVisThreads), 0, ctx->stream, seg, st, (const int4*)list, list_cap, area,
                       d->anchors, d->cap, (int*)d->n_anchors);
    ODISE_CHECK_HIP(hipGetLastError());
    if (hcap > 0) {
        hipLaunchKernelGGL(vis_hist_kernel, dim3(pb), dim3(kVisThreads), 0, ctx->stream, ids, seg, (const int*)roots, (const int*)area,
                           (const VisState*)st, H, W, hcap, hist);
        ODISE_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(vis_median_kernel, dim3(2 * hcap), dim3(64), 0, ctx->stream, (const VisState*)st, (const int*)hist, H, W, hcap, d->cap,
                           d->anchors);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

extern "C" int odise_hip_panoptic_overlay(odise_hip_ctx* ctx, const odise_overlay_desc* d) {
    ODISE_REQUIRE(ctx, "panoptic_overlay: null context");
    ODISE_REQUIRE(d, "panoptic_overlay: null descriptor");
    ODISE_REQUIRE(d->image && d->pred_ids && d->pred_segments && d->colors && d->out, "panoptic_overlay: null pointer");
    ODISE_TRY(vis_check_size("panoptic_overlay", d->H, d->W));
    ODISE_REQUIRE(d->alpha256 >= 0 && d->alpha256 <= 256, "panoptic_overlay: alpha256 %d outside 0..256", d->alpha256);
    ODISE_REQUIRE((((uintptr_t)d->pred_ids | (uintptr_t)d->pred_segments) & 3) == 0, "panoptic_overlay: int32 buffers must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const int npix = d->H * d->W;
    const int vec = (((uintptr_t)d->image | (uintptr_t)d->out) & 3) == 0;
    const unsigned edge = (unsigned)d->edge_rgb[0] | ((unsigned)d->edge_rgb[1] << 8) | ((unsigned)d->edge_rgb[2] << 16);
    hipLaunchKernelGGL(overlay_kernel, dim3(grid_blocks(ctx, ceil_div(npix, 4), kVisThreads)), dim3(kVisThreads), 0, ctx->stream, (const uint8_t*)d->image,
                       (const int*)d->pred_ids, (const int*)d->pred_segments, (const uint8_t*)d->colors, d->H, d->W, d->alpha256, edge, vec,
                       (uint8_t*)d->out);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
