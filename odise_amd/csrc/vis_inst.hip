// vis_inst.hip — drawing instance and semantic results: the else branch of VisualizationDemo.run_on_image (demo/demo.py:173-199),
// detectron2 draw_instance_predictions / draw_sem_seg (odise_hip_instance_draw / odise_hip_semantic_record; host restatement:
// odise_amd/visualize.py).
//
// Instances overlap, so there is no label map: the masks are the bit-packed words of rle_pack.h ([n][w][R], word (x, r) = rows
// 64 r .. 64 r + 63 of column x), packed from the mask logits with the taps of odise_hip_instance_rle or from dense masks.
//
//   inst_col_kernel      count of column x = the popcounts of its R words
//   inst_row_kernel      a wave per (mask, r), lane = bit: count of row 64 r + lane = the columns whose word has the bit.  A lane loads
//                        the word of its own column and the wave walks the 64 loaded words by readlane.  No atomics in either.
//   inst_anchor_kernel   a wave per (mask, axis): area = the sum of the histogram, kept = in the table, score >= min_score and area > 0,
//                        then the scan of vis_scan.h for twice the median and the bounding box
//   inst_order_kernel    draw order = rank by (area descending, index ascending) among the kept, by counting; list[rank] = index
//   inst_overlay_kernel  one block per tile of 64 columns x 64 rows (one word row).  The kept masks are taken in draw order, kDrawChunk
//                        at a time: a thread fetches the words of four neighbouring columns of one mask (with the bits above and below
//                        and the columns left and right), works out which pixels have a 4-neighbour outside the mask, and leaves in LDS
//                        one dword per (mask, 4 rows, 4 columns): 16 mask bits and 16 edge bits.  That is the transpose: in the pixel
//                        phase a thread owns 4 x 4 pixels - four consecutive pixels of four rows, kept in registers over the whole walk -
//                        and reads one conflict-free dword per mask, which it skips when its mask bits are zero.  A row of four pixels
//                        travels as three dwords where its 12 bytes are 4-byte aligned in both pictures, byte by byte otherwise.
//
// With boxes (odise_hip_instance_draw_boxes: overlay_instances(boxes=, masks=)) inst_box_anchor_kernel stands in for inst_anchor_kernel
// (kept also asks for a box with an area; the anchors are the box and its corner), inst_order_kernel<true> ranks by box area and
// inst_overlay_kernel<true> lays the frame of a box before its mask.  The <false> forms are the kernels described above.
//
// The semantic record: a per-block LDS histogram of the labels (lds_hist.h; the arg-max of semantic_confusion_kernel for a score
// tensor), the rank of every present class by counting, and one pass that turns labels into ids.
#include <algorithm>

#include "inst_words.h"
#include "lds_hist.h"
#include "record.h"
#include "rgb.h"
#include "vis_scan.h"

namespace odise {

constexpr int kDrawThreads = 256;
constexpr int kDrawChunk = 50;             // masks staged at a time
constexpr int kDrawStride = 256 + 16;      // dwords per staged mask: 16 row groups x 16 column groups, + 16 so that the 32 lanes of a
                                           // staging write (two masks) fall on 32 different banks
constexpr int kSemMaxClasses = kLdsHistCells;

struct InstDrawState {
    int area[kInstMaxTopk];                // pixels of a kept instance, 0 when it is not kept
    int list[kInstMaxTopk];                // list[k] = the instance drawn k-th
    int n_kept;
    int pad[3];
};
struct InstBoxState {                      // odise_hip_instance_draw_boxes, by table index
    float barea[kInstMaxTopk];             // (x1 - x0) * (y1 - y0) of a kept instance's box as the float product: the order key
    int box[kInstMaxTopk][4];              // bx0, by0, bx1, by1: the box clipped to the picture, members truncated
};

__global__ void __launch_bounds__(kDrawThreads) inst_col_kernel(const unsigned long long* __restrict__ words, RleGrid G, const int* __restrict__ table,
                                                               int topk, int* __restrict__ colhist) {
    const int i = blockIdx.y;
    if (i >= inst_count(table, topk)) return;
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= G.w) return;
    const unsigned long long* c = words + (int64_t)i * G.nw + x * G.R;
    int s = 0;
    for (int r = 0; r < G.R; ++r) s += __popcll(c[r]);
    colhist[(int64_t)i * G.w + x] = s;
}

__global__ void __launch_bounds__(64) inst_row_kernel(const unsigned long long* __restrict__ words, RleGrid G, const int* __restrict__ table, int topk,
                                                     int* __restrict__ rowhist) {
    const int i = blockIdx.y, r = blockIdx.x, lane = threadIdx.x;
    if (i >= inst_count(table, topk)) return;
    const unsigned long long* wd = words + (int64_t)i * G.nw + r;
    int cnt = 0;
    for (int x0 = 0; x0 < G.w; x0 += 64) {
        const int x = x0 + lane;
        const unsigned long long v = x < G.w ? wd[(int64_t)x * G.R] : 0ull;
        const int lo = (int)(unsigned)v, hi = (int)(unsigned)(v >> 32);
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const unsigned lj = (unsigned)__builtin_amdgcn_readlane(lo, j), hj = (unsigned)__builtin_amdgcn_readlane(hi, j);
            cnt += (int)(((lane < 32 ? lj : hj) >> (lane & 31)) & 1u);
        }
    }
    const int y = 64 * r + lane;
    if (y < G.h) rowhist[(int64_t)i * G.h + y] = cnt;
}

// axes = 1: areas only (nothing is scanned, `anchors` is null); axes = 2: a wave per axis.  The x wave owns segment_row, area and the
// x fields of a row (and all of a row that is not kept), the y wave the y fields.
__global__ void __launch_bounds__(64) inst_anchor_kernel(const int* __restrict__ colhist, const int* __restrict__ rowhist, int H, int W,
                                                        const int* __restrict__ table, const float* __restrict__ scores, int topk, float min_score,
                                                        int axes, InstDrawState* __restrict__ st, odise_anchor_row* __restrict__ anchors) {
    const int i = blockIdx.x / axes, axis = blockIdx.x - i * axes, lane = threadIdx.x;
    const int nb = axis ? H : W;
    const int* h = axis ? rowhist + (int64_t)i * H : colhist + (int64_t)i * W;
    int N = 0;
    if (inst_candidate(table, scores, topk, min_score, i)) {
        for (int b0 = 0; b0 < nb; b0 += 64) N += b0 + lane < nb ? h[b0 + lane] : 0;
        for (int d = 32; d; d >>= 1) N += __shfl_xor(N, d);
    }
    const bool kept = N > 0;
    if (!kept) {
        if (lane == 0 && axis == 0) {
            st->area[i] = 0;
            if (anchors) anchors[i] = vis_anchor_row(-1, 0);
        }
        return;
    }
    if (lane == 0 && axis == 0) st->area[i] = N;
    if (!anchors) return;
    int m1, m2, lo, hi;
    vis_scan_middle(h, nb, N, lane, m1, m2, lo, hi);
    if (lane == 0) {
        if (axis) { anchors[i].y2 = m1 + m2; anchors[i].y0 = lo; anchors[i].y1 = hi; }
        else { anchors[i].segment_row = i; anchors[i].area = N; anchors[i].x2 = m1 + m2; anchors[i].x0 = lo; anchors[i].x1 = hi; }
    }
}

// The box variant (odise_hip_instance_draw_boxes): a wave per table index.  kept = a candidate with a pixel AND a finite box of positive
// width and height; its order key, its box clipped to the picture and - the box, not the mask median, decides where the label goes - its
// anchor row (Visualizer.overlay_instances with boxes: the text at the box corner, moved for a small box).
__device__ __forceinline__ int box_trunc(float v) { return (int)fminf(fmaxf(v, -536870912.f), 536870912.f); }   // toward zero, within +-2^29

__global__ void __launch_bounds__(64) inst_box_anchor_kernel(const int* __restrict__ colhist, int H, int W, const int* __restrict__ table,
                                                            const float* __restrict__ scores, int topk, float min_score,
                                                            const float* __restrict__ boxes, int small_area, InstDrawState* __restrict__ st,
                                                            InstBoxState* __restrict__ bs, odise_anchor_row* __restrict__ anchors) {
    const int i = blockIdx.x, lane = threadIdx.x;
    int N = 0;
    if (inst_candidate(table, scores, topk, min_score, i)) {
        const int* h = colhist + (int64_t)i * W;
        for (int b0 = 0; b0 < W; b0 += 64) N += b0 + lane < W ? h[b0 + lane] : 0;
        for (int d = 32; d; d >>= 1) N += __shfl_xor(N, d);
    }
    if (lane != 0) return;
    const float x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
    const bool kept = N > 0 && isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && x1 > x0 && y1 > y0;
    st->area[i] = kept ? N : 0;
    if (!kept) {
        bs->barea[i] = 0.f;
        bs->box[i][0] = 0; bs->box[i][1] = 0; bs->box[i][2] = 0; bs->box[i][3] = 0;
        if (anchors) anchors[i] = vis_anchor_row(-1, 0);
        return;
    }
    const float ba = (x1 - x0) * (y1 - y0);
    const int ix0 = box_trunc(x0), iy0 = box_trunc(y0), ix1 = box_trunc(x1), iy1 = box_trunc(y1);
    bs->barea[i] = ba;
    bs->box[i][0] = max(ix0, 0); bs->box[i][1] = max(iy0, 0); bs->box[i][2] = min(ix1, W); bs->box[i][3] = min(iy1, H);
    if (!anchors) return;
    int tx = ix0, ty = iy0;
    if (ba < (float)small_area || y1 - y0 < 40.f) {
        if (y1 >= (float)(H - 5)) tx = ix1;
        else ty = iy1;
    }
    odise_anchor_row a;
    a.segment_row = i; a.area = N; a.x2 = 2 * tx; a.y2 = 2 * ty; a.x0 = ix0; a.y0 = iy0; a.x1 = ix1; a.y1 = iy1;
    anchors[i] = a;
}

// kBox: the order key is the box area (kept: area > 0), else the pixels
template <bool kBox>
__global__ void __launch_bounds__(128) inst_order_kernel(InstDrawState* __restrict__ st, const InstBoxState* __restrict__ bs, int topk,
                                                        int* __restrict__ order) {
    __shared__ int a[kInstMaxTopk];
    __shared__ float ba[kBox ? kInstMaxTopk : 1];
    const int t = threadIdx.x;
    if (t < topk) {
        a[t] = st->area[t];
        if (kBox) ba[t] = bs->barea[t];
    }
    __syncthreads();
    if (t < topk) {
        int rank = -1;
        if (a[t] > 0) {
            rank = 0;
            for (int j = 0; j < topk; ++j) {
                if (kBox) rank += (a[j] > 0 && (ba[j] > ba[t] || (ba[j] == ba[t] && j < t))) ? 1 : 0;
                else rank += (a[j] > a[t] || (a[j] == a[t] && j < t)) ? 1 : 0;
            }
            st->list[rank] = t;
        }
        if (order) order[t] = rank;
    }
    if (t == 0) {
        int n = 0;
        for (int j = 0; j < topk; ++j) n += a[j] > 0 ? 1 : 0;
        st->n_kept = n;
    }
}

// image == out is safe: a thread reads its own 16 pixels before it writes them and no other thread reads them.
// kBox (odise_hip_instance_draw_boxes): before the mask step of instance i its rectangle frame - the pixels of the clipped box bs->box[i]
// within box_width of one of its four sides - is blended with colors[i] at box_alpha.  The bounds of a chunk's boxes lie in LDS (every
// thread reads the same dword: a broadcast); a thread whose 4 x 4 pixels miss the box, or lie in its interior, makes four compares.
template <bool kBox>
__global__ void __launch_bounds__(kDrawThreads) inst_overlay_kernel(const unsigned long long* __restrict__ words, RleGrid G, int ntx,
                                                                   const InstDrawState* __restrict__ st, const uint8_t* image,
                                                                   const uint8_t* __restrict__ colors, const uint8_t* __restrict__ edge_colors,
                                                                   int alpha, uint8_t* out, const InstBoxState* __restrict__ bs, int box_width,
                                                                   int box_alpha) {
    __shared__ unsigned sl[kDrawChunk * kDrawStride];
    __shared__ unsigned s_crb[kDrawChunk], s_cg[kDrawChunk], s_edge[kDrawChunk];
    __shared__ int s_box[kBox ? kDrawChunk : 1][4];
    __shared__ unsigned s_brb[kBox ? kDrawChunk : 1], s_bg[kBox ? kDrawChunk : 1];
    const int t = threadIdx.x, H = G.h, W = G.w;
    const int r = blockIdx.x / ntx, x0 = (blockIdx.x - r * ntx) * 64;
    const int xq = t & 15, rg = t >> 4;
    const int px_x = x0 + 4 * xq, px_y = 64 * r + 4 * rg;
    const unsigned ia = (unsigned)(256 - alpha);

    unsigned px[4][4];
    bool vec[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = px_y + j;
        const int64_t off = 3 * ((int64_t)y * W + px_x);
        vec[j] = y < H && px_x + 3 < W && ((((uintptr_t)image + off) | ((uintptr_t)out + off)) & 3) == 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) px[j][c] = 0u;
        if (vec[j]) {
            const unsigned* src = (const unsigned*)(image + off);   // the 12 bytes of four pixels inside the row
            rgb4_unpack(src[0], src[1], src[2], px[j]);
        } else if (y < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (px_x + c < W) px[j][c] = rgb_load(image + off + 3 * c);
        }
    }

    const int n_kept = min(max(st->n_kept, 0), kInstMaxTopk);
    const int rows = min(64, H - 64 * r);
    const unsigned long long padbits = rows == 64 ? 0ull : ~0ull << rows;   // rows past the picture count as inside the mask: no edge there
    for (int k0 = 0; k0 < n_kept; k0 += kDrawChunk) {
        const int nk = min(kDrawChunk, n_kept - k0);
        __syncthreads();                                                     // the previous chunk has been read
        if (t < nk) {
            const int i = st->list[k0 + t];
            blend_color(rgb_load(colors + 3 * i), (unsigned)alpha, s_crb[t], s_cg[t]);
            s_edge[t] = rgb_load(edge_colors + 3 * i);
            if (kBox) {
#pragma unroll
                for (int c = 0; c < 4; ++c) s_box[t][c] = bs->box[i][c];
                blend_color(rgb_load(colors + 3 * i), (unsigned)box_alpha, s_brb[t], s_bg[t]);
            }
        }
        for (int it = t; it < nk * 16; it += kDrawThreads) {                // item = (mask k, four columns q)
            const int k = it >> 4, q = it & 15, xa = x0 + 4 * q;
            const int i = st->list[k0 + k];
            const unsigned long long* wm = words + (int64_t)i * G.nw + r;   // word (x, r) = wm[x * R]
            unsigned long long m[6];                                        // columns xa - 1 .. xa + 4; outside the picture: inside the mask
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const int x = xa - 1 + c;
                m[c] = (x >= 0 && x < W) ? wm[(int64_t)x * G.R] : ~0ull;
            }
            unsigned long long mm[4], ee[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int x = xa + c;
                mm[c] = 0ull; ee[c] = 0ull;
                if (x < W) {
                    const unsigned long long v = m[c + 1];
                    const unsigned long long above = r > 0 ? wm[(int64_t)x * G.R - 1] >> 63 : 1ull;
                    const unsigned long long below = r < G.R - 1 ? wm[(int64_t)x * G.R + 1] & 1ull : 1ull;
                    const unsigned long long up = (v << 1) | above, down = ((v | padbits) >> 1) | (below << 63);
                    mm[c] = v;
                    ee[c] = v & ~(up & down & m[c] & m[c + 2]);
                }
            }
            unsigned* dst = sl + k * kDrawStride + q;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                unsigned d = 0u;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    d |= ((unsigned)(mm[c] >> (4 * g)) & 0xfu) << (4 * c) | ((unsigned)(ee[c] >> (4 * g)) & 0xfu) << (16 + 4 * c);
                dst[g * 16] = d;
            }
        }
        __syncthreads();
        for (int k = 0; k < nk; ++k) {
            if (kBox) {                                                     // the frame first; a tile no mask touches may still hold one
                const int bx0 = s_box[k][0], by0 = s_box[k][1], bx1 = s_box[k][2], by1 = s_box[k][3];
                const bool touches = px_x < bx1 && px_x + 4 > bx0 && px_y < by1 && px_y + 4 > by0;
                const bool interior = px_x >= bx0 + box_width && px_x + 4 <= bx1 - box_width && px_y >= by0 + box_width && px_y + 4 <= by1 - box_width;
                if (touches && !interior) {
                    const unsigned brb = s_brb[k], bg = s_bg[k], iab = (unsigned)(256 - box_alpha);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int x = px_x + c, y = px_y + j;
                            const bool in = x >= bx0 && x < bx1 && y >= by0 && y < by1;
                            const bool side = x < bx0 + box_width || x >= bx1 - box_width || y < by0 + box_width || y >= by1 - box_width;
                            if (in && side) px[j][c] = blend_rgb(px[j][c], iab, brb, bg);
                        }
                }
            }
            const unsigned s = sl[k * kDrawStride + t];                     // t = rg * 16 + xq
            if ((s & 0xffffu) == 0u) continue;
            const unsigned crb = s_crb[k], cg = s_cg[k], edge = s_edge[k];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int bit = 4 * c + j;
                    if ((s >> bit) & 1u) px[j][c] = ((s >> (16 + bit)) & 1u) ? edge : blend_rgb(px[j][c], ia, crb, cg);
                }
        }
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = px_y + j;
        const int64_t off = 3 * ((int64_t)y * W + px_x);
        if (vec[j]) {
            rgb4_pack(px[j], (unsigned*)(out + off));
        } else if (y < H) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (px_x + c < W) rgb_store(out + off + 3 * c, px[j][c]);
        }
    }
}

// ---- the semantic record ----------------------------------------------------------------------------------------------------------

// counts[l] += 1 for every label in [0, K).  kSem: the label is the first-maximum arg-max over the K planes and is left in ids[p].
template <bool kSem>
__global__ void __launch_bounds__(256) sem_count_kernel(const int* __restrict__ labels, const float* __restrict__ sem, int K, int npix,
                                                       unsigned* __restrict__ counts, int* __restrict__ ids) {
    const LdsHist<unsigned> Hh(counts, K, K <= kLdsHistCells);
    Hh.clear();
    Hh.sync();
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        int l;
        if (kSem) { l = argmax_first(sem, K, npix, p); ids[p] = l; }
        else l = labels[p];
        if ((unsigned)l < (unsigned)K) Hh.add(l, 1u);
    }
    Hh.sync();
    Hh.flush();
}

// One block.  The row of a present class = the classes with a larger count, or an equal count and a smaller index.  map[c] = its id.
__global__ void __launch_bounds__(1024) sem_rank_kernel(const unsigned* __restrict__ counts, int K, int* __restrict__ map, int* __restrict__ table) {
    __shared__ int present;
    if (threadIdx.x == 0) present = 0;
    __syncthreads();
    for (int c = threadIdx.x; c < K; c += blockDim.x) {
        const unsigned cnt = counts[c];
        int id = 0;
        if (cnt > 0u) {
            int rank = 0;
            for (int j = 0; j < K; ++j) {
                const unsigned v = counts[j];
                rank += (v > cnt || (v == cnt && j < c)) ? 1 : 0;
            }
            if (rank < ODISE_MAX_SEGMENTS) {
                id = c + 1;
                record_set_row(table, rank, id, 0, c);
            }
            atomicAdd(&present, 1);
        }
        map[c] = id;
    }
    __syncthreads();
    const int n = min(present, ODISE_MAX_SEGMENTS);
    if (threadIdx.x == 0) table[0] = n;
    record_zero_rows(table, n, ODISE_MAX_SEGMENTS, threadIdx.x, blockDim.x);
}

template <bool kSem>
__global__ void __launch_bounds__(256) sem_ids_kernel(const int* __restrict__ labels, const int* __restrict__ map, int K, int npix, int* __restrict__ ids) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int l = kSem ? ids[p] : labels[p];
        ids[p] = (unsigned)l < (unsigned)K ? map[l] : 0;
    }
}

}  // namespace odise

using namespace odise;

// odise_hip_instance_draw (bx == nullptr) and odise_hip_instance_draw_boxes: one pack, the column (and row) histograms, kept / anchors /
// order by the masks alone or with the boxes, the picture
static int inst_draw(odise_hip_ctx* ctx, const char* what, const odise_inst_draw_desc* d, const odise_inst_box_draw* bx) {
    const InstSource src = inst_source(*d);
    ODISE_TRY(inst_source_check(what, src, false, kVisMaxPixels));
    ODISE_REQUIRE(!d->out || (d->image && d->colors && d->edge_colors), "%s: an output picture needs image, colors and edge_colors", what);
    ODISE_REQUIRE(d->out || d->anchors || d->order, "%s: no output", what);
    ODISE_REQUIRE(d->alpha256 >= 0 && d->alpha256 <= 256, "%s: alpha256 %d outside 0..256", what, d->alpha256);
    ODISE_REQUIRE((((uintptr_t)d->anchors | (uintptr_t)d->order) & 3) == 0, "%s: anchors / order must be 4-byte aligned", what);
    if (bx) {
        ODISE_REQUIRE(bx->boxes && ((uintptr_t)bx->boxes & 3) == 0, "%s: boxes must be a 4-byte aligned device pointer", what);
        ODISE_REQUIRE(bx->box_width >= 1, "%s: box_width %d below 1", what, bx->box_width);
        ODISE_REQUIRE(bx->box_alpha256 >= 0 && bx->box_alpha256 <= 256, "%s: box_alpha256 %d outside 0..256", what, bx->box_alpha256);
    }
    const int H = d->h, W = d->w, topk = d->topk;
    if (d->out && d->out != d->image) {
        const uintptr_t a = (uintptr_t)d->image, b = (uintptr_t)d->out, nb = (uintptr_t)3 * H * W;
        ODISE_REQUIRE(a + nb <= b || b + nb <= a, "%s: out overlaps image without being equal to it", what);
    }
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    InstGeom ig;
    ODISE_TRY(inst_geom(ctx, what, src, &ig));
    const RleGrid G = rle_grid(H, W);
    const bool rows_wanted = d->anchors && !bx;   // with boxes the anchors come from the boxes
    const size_t col_b = (size_t)round_up((int64_t)topk * W * 4, 16), row_b = rows_wanted ? (size_t)round_up((int64_t)topk * H * 4, 16) : 0;
    const size_t box_b = bx ? sizeof(InstBoxState) : 0;
    RleScratch s;
    ODISE_TRY(rle_scratch(ctx, topk, G, &s, sizeof(InstDrawState) + box_b + col_b + row_b));
    InstDrawState* st = (InstDrawState*)s.extra;
    InstBoxState* bs = (InstBoxState*)((char*)s.extra + sizeof(InstDrawState));
    int* colhist = (int*)((char*)bs + box_b);
    int* rowhist = (int*)((char*)colhist + col_b);
    const int* table = src.inst_table;
    ODISE_TRY(inst_pack(ctx, src, ig, G, s.words));
    hipLaunchKernelGGL(inst_col_kernel, dim3((unsigned)ceil_div(W, kDrawThreads), (unsigned)topk), dim3(kDrawThreads), 0, ctx->stream,
                       (const unsigned long long*)s.words, G, table, topk, colhist);
    ODISE_CHECK_HIP(hipGetLastError());
    if (rows_wanted) {
        hipLaunchKernelGGL(inst_row_kernel, dim3((unsigned)G.R, (unsigned)topk), dim3(64), 0, ctx->stream, (const unsigned long long*)s.words, G, table,
                           topk, rowhist);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    if (bx) {
        hipLaunchKernelGGL(inst_box_anchor_kernel, dim3((unsigned)topk), dim3(64), 0, ctx->stream, (const int*)colhist, H, W, table, d->inst_scores, topk,
                           d->min_score, bx->boxes, bx->small_area, st, bs, d->anchors);
    } else {
        const int axes = d->anchors ? 2 : 1;
        hipLaunchKernelGGL(inst_anchor_kernel, dim3((unsigned)(axes * topk)), dim3(64), 0, ctx->stream, (const int*)colhist, (const int*)rowhist, H, W, table,
                           d->inst_scores, topk, d->min_score, axes, st, d->anchors);
    }
    ODISE_CHECK_HIP(hipGetLastError());
    if (d->order || d->out) {
        if (bx) hipLaunchKernelGGL(inst_order_kernel<true>, dim3(1), dim3(128), 0, ctx->stream, st, (const InstBoxState*)bs, topk, (int*)d->order);
        else hipLaunchKernelGGL(inst_order_kernel<false>, dim3(1), dim3(128), 0, ctx->stream, st, (const InstBoxState*)nullptr, topk, (int*)d->order);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    if (d->out) {
        const int ntx = (int)ceil_div(W, 64);
        const dim3 grid((unsigned)((int64_t)ntx * G.R));
        if (bx)   // a width beyond the picture draws what the picture's longer side draws
            hipLaunchKernelGGL(inst_overlay_kernel<true>, grid, dim3(kDrawThreads), 0, ctx->stream, (const unsigned long long*)s.words, G, ntx,
                               (const InstDrawState*)st, d->image, d->colors, d->edge_colors, d->alpha256, d->out, (const InstBoxState*)bs,
                               std::min(bx->box_width, std::max(H, W)), bx->box_alpha256);
        else
            hipLaunchKernelGGL(inst_overlay_kernel<false>, grid, dim3(kDrawThreads), 0, ctx->stream, (const unsigned long long*)s.words, G, ntx,
                               (const InstDrawState*)st, d->image, d->colors, d->edge_colors, d->alpha256, d->out, (const InstBoxState*)nullptr, 0, 0);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

extern "C" int odise_hip_instance_draw(odise_hip_ctx* ctx, const odise_inst_draw_desc* d) {
    ODISE_REQUIRE(ctx && d, "instance_draw: null argument");
    return inst_draw(ctx, "instance_draw", d, nullptr);
}

extern "C" int odise_hip_sizeof_inst_box_draw(void) { return (int)sizeof(odise_inst_box_draw); }

extern "C" int odise_hip_instance_draw_boxes(odise_hip_ctx* ctx, const odise_inst_draw_desc* d, const odise_inst_box_draw* bx) {
    ODISE_REQUIRE(ctx && d && bx, "instance_draw_boxes: null argument");
    return inst_draw(ctx, "instance_draw_boxes", d, bx);
}

extern "C" int odise_hip_semantic_record(odise_hip_ctx* ctx, const int32_t* labels, const float* sem_seg, int K, int H, int W, int32_t* record) {
    ODISE_REQUIRE(ctx, "semantic_record: null context");
    ODISE_REQUIRE((labels != nullptr) != (sem_seg != nullptr) && record, "semantic_record: one of labels / sem_seg, and a record");
    ODISE_TRY(vis_check_size("semantic_record", H, W));
    ODISE_REQUIRE(K >= 1 && K <= kSemMaxClasses, "semantic_record: %d classes (1..%d)", K, kSemMaxClasses);
    ODISE_REQUIRE((((uintptr_t)labels | (uintptr_t)sem_seg | (uintptr_t)record) & 3) == 0, "semantic_record: buffers must be 4-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const int npix = H * W;
    const size_t kb = (size_t)round_up((int64_t)K * 4, 16);
    ODISE_TRY(scratch_reserve(ctx->vis, 2 * kb, 8, drain_streams(ctx->stream), "semantic_record"));
    unsigned* counts = (unsigned*)ctx->vis.ptr;
    int* map = (int*)((char*)ctx->vis.ptr + kb);
    int* ids = (int*)record;
    ODISE_CHECK_HIP(hipMemsetAsync(counts, 0, kb, ctx->stream));
    const int blocks = grid_blocks(ctx, npix, 256);
    if (sem_seg) hipLaunchKernelGGL(sem_count_kernel<true>, dim3(blocks), dim3(256), lds_hist_bytes(K), ctx->stream, (const int*)nullptr, sem_seg, K, npix, counts, ids);
    else hipLaunchKernelGGL(sem_count_kernel<false>, dim3(blocks), dim3(256), lds_hist_bytes(K), ctx->stream, (const int*)labels, (const float*)nullptr, K, npix, counts, ids);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sem_rank_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned*)counts, K, map, ids + npix);
    ODISE_CHECK_HIP(hipGetLastError());
    if (sem_seg) hipLaunchKernelGGL(sem_ids_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, (const int*)nullptr, (const int*)map, K, npix, ids);
    else hipLaunchKernelGGL(sem_ids_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, (const int*)labels, (const int*)map, K, npix, ids);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
