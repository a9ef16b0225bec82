// eval_ops.hip — input resize and evaluator reductions of the evaluation loop on the device.
//
//   odise_hip_resize_bilinear_u8   detectron2 T.ResizeShortestEdge -> ResizeTransform -> PIL.Image.resize(BILINEAR) on uint8 images
//                                  (configs/common/data/pano_open_d2_eval.py:74-107).  Pillow's 8-bit resampler is reproduced bit for
//                                  bit: double-precision triangle-filter coefficients normalised per output pixel, rounded to 22-bit
//                                  fixed point on the host, horizontal pass then vertical pass with a uint8 intermediate, accumulate
//                                  from 1 << 21, shift, clip.
//   odise_hip_u8_hwc_to_f32_chw    the DatasetMapper's HWC uint8 -> CHW float step (times `scale`, e.g. 1/255 for pixel_std 255).
//   odise_hip_semantic_confusion   detectron2 SemSegEvaluator.process (odise/evaluation/d2_evaluator.py:63): argmax over classes,
//                                  (K+1)^2 confusion counts (rows = prediction, ignore label mapped to K by the caller).
//   odise_hip_pair_histogram       the per-pixel part of panopticapi pq_compute_single_core (COCOPanopticEvaluator,
//                                  d2_evaluator.py:49): co-occurrence counts of (ground-truth segment, predicted segment) indices of
//                                  pre-indexed maps.  The evaluator's whole per-picture step - ids to slots, counts, matching, the add
//                                  into (iou, tp, fp, fn) - is odise_hip_panoptic_quality in pq.hip.
//   odise_hip_semantic_eval        the whole SemSegEvaluator.process step from the prediction as it lies in HBM - the int32 label map of the
//                                  fused arg-max, or the score tensor with the arg-max taken once into scratch: both matrices below and the
//                                  per-class COCO RLE strings of sem_seg_predictions.json (sem_rle.hip).
//   odise_hip_semantic_eval_pq     the same launches, then the PQ-for-semantic-segmentation statistics of the same label map (sem_pq.hip).
//   odise_hip_label_boundary / odise_hip_semantic_boundary_confusion
//                                  the second per-pixel job of SemSegEvaluator.process (K < 255, OpenCV importable): prediction and ground
//                                  truth both go through _mask_to_boundary - a 3x3 grey-scale erosion behind a zero ring, repeated
//                                  r = max(1, round(0.02 * diagonal)) times, subtracted from the map - and the pairs of the two LABEL
//                                  DIFFERENCES are counted in a second (K+1)^2 matrix (_b_conf_matrix, Boundary IoU).  r erosions are one
//                                  (2r+1)^2 minimum with zeros outside the picture, so:
//                                    labels  arg-max (+ the confusion counts) -> two byte maps [H][pitch], four labels per dword
//                                    min     row direction, then column direction, each by window growing: a pass takes the minimum of up
//                                            to four shifted copies of the previous pass's windows (1 -> 4 -> 16 -> ... pixels, the last pass
//                                            places ceil((2r+1) / s) windows of s over the 2r+1), reads outside the picture give 0.  The cost
//                                            per pixel grows with log4(r), the passes run in global memory (the maps are 1-7 MB and stay in
//                                            the L2 / MALL), so r may exceed any tile; 2r+1 > min(H, W) erodes everything and skips them.
//                                    count   b = m - e per byte (m >= e: a plain dword subtraction), cell (0, 0) - every pixel away from a
//                                            boundary - in a register, the rest through the per-block histogram.
// All of it is HBM-bound integer / byte work: coalesced row-major sweeps, per-block histograms (lds_hist.h).
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "label_maps.h"
#include "lds_hist.h"
#include "rle_pack.h"   // sem_rle.hip: the per-class strings of odise_hip_semantic_eval

namespace odise {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int64_t kSemEvalMaxPixels = (1ll << 29) - 1;   // odise_hip_semantic_eval: per picture, as odise_hip_panoptic_quality

struct ResampleCoeffs {
    std::vector<int> bounds;  // [out][2] (xmin, count)
    std::vector<int> kk;      // [out][ksize]
    int ksize = 0;
};

// Pillow precompute_coeffs + normalize_coeffs_8bpc, bilinear filter (support 1), whole input range
static void precompute_coeffs(int in_size, int out_size, ResampleCoeffs& c) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    c.ksize = (int)ceil(support) * 2 + 1;
    c.bounds.assign((size_t)out_size * 2, 0);
    c.kk.assign((size_t)out_size * c.ksize, 0);
    std::vector<double> k(c.ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < c.ksize; ++x) k[x] = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        c.bounds[2 * xx] = xmin;
        c.bounds[2 * xx + 1] = xmax;
        for (int x = 0; x < c.ksize; ++x)
            c.kk[(size_t)xx * c.ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kPrecisionBits)) : (int)(0.5 + k[x] * (1 << kPrecisionBits));
    }
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// one thread per output byte (row, ox, c); src row pitch W*C
__global__ void __launch_bounds__(256) resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ bounds,
                                                        const int* __restrict__ kk, int H, int W, int OW, int C, int ksize) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)H * OW * C;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int ox = (int)((idx / C) % OW);
    const int y = (int)(idx / ((int64_t)C * OW));
    const int xmin = bounds[2 * ox], n = bounds[2 * ox + 1];
    const int* k = kk + (size_t)ox * ksize;
    const uint8_t* s = src + ((int64_t)y * W + xmin) * C + c;
    int acc = 1 << (kPrecisionBits - 1);
    for (int x = 0; x < n; ++x) acc += (int)s[(int64_t)x * C] * k[x];
    dst[idx] = clip8(acc);
}

// one thread per output byte (oy, x*C + c); rows of W*C bytes
__global__ void __launch_bounds__(256) resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int* __restrict__ bounds,
                                                        const int* __restrict__ kk, int OH, int row_bytes, int ksize) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)OH * row_bytes;
    if (idx >= total) return;
    const int xb = (int)(idx % row_bytes);
    const int oy = (int)(idx / row_bytes);
    const int ymin = bounds[2 * oy], n = bounds[2 * oy + 1];
    const int* k = kk + (size_t)oy * ksize;
    const uint8_t* s = src + (int64_t)ymin * row_bytes + xb;
    int acc = 1 << (kPrecisionBits - 1);
    for (int y = 0; y < n; ++y) acc += (int)s[(int64_t)y * row_bytes] * k[y];
    dst[idx] = clip8(acc);
}

__global__ void __launch_bounds__(256) u8_hwc_to_f32_chw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int HW, int C, float scale) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)HW * C) return;
    const int c = (int)(idx / HW);
    const int p = (int)(idx - (int64_t)c * HW);
    dst[idx] = (float)src[(int64_t)p * C + c] * scale;
}

// dst [C,Hp,Wp]: the image in the top-left corner, zeros elsewhere (ImageList.from_tensors)
__global__ void __launch_bounds__(256) u8_hwc_to_f32_chw_pad_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int H, int W, int C,
                                                                   int Hp, int Wp, float scale) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t plane = (int64_t)Hp * Wp;
    if (idx >= plane * C) return;
    const int c = (int)(idx / plane);
    const int64_t p = idx - c * plane;
    const int y = (int)(p / Wp), x = (int)(p - (int64_t)y * Wp);
    dst[idx] = (y < H && x < W) ? (float)src[((int64_t)y * W + x) * C + c] * scale : 0.f;
}

// ---- Boundary IoU counters ------------------------------------------------------------------------------------------------------------------
// The byte label maps (LabelGrid, store_label, BoundaryMaps): label_maps.h.
constexpr int kMinTaps = 4;
struct MinTaps {
    int n, off[kMinTaps];
};

__device__ __forceinline__ unsigned min_u8x4(unsigned a, unsigned b) {   // per byte, as two pairs of 16-bit lanes (v_pk_min_u16)
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const unsigned m = 0x00ff00ffu;
    const u16x2 lo = __builtin_elementwise_min(__builtin_bit_cast(u16x2, a & m), __builtin_bit_cast(u16x2, b & m));
    const u16x2 hi = __builtin_elementwise_min(__builtin_bit_cast(u16x2, (a >> 8) & m), __builtin_bit_cast(u16x2, (b >> 8) & m));
    return __builtin_bit_cast(unsigned, lo) | (__builtin_bit_cast(unsigned, hi) << 8);
}
// dword xd of a row, 0 outside it
__device__ __forceinline__ unsigned label_dword(const unsigned* __restrict__ row, int xd, const LabelGrid& G) {
    if ((unsigned)xd >= (unsigned)G.Pd) return 0u;
    const unsigned v = row[xd];
    return xd == G.Pd - 1 ? v & G.tail : v;
}
// pixels 4 xd + dx .. 4 xd + dx + 3 of row y, 0 outside the picture
__device__ __forceinline__ unsigned label_window(const unsigned* __restrict__ map, int y, int xd, int dx, const LabelGrid& G) {
    if ((unsigned)y >= (unsigned)G.H) return 0u;
    const unsigned* row = map + (int64_t)y * G.Pd;
    const int q = xd + (dx >> 2), t = dx & 3;
    const unsigned lo = label_dword(row, q, G), hi = t ? label_dword(row, q + 1, G) : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)t);
}

// int32 labels -> one byte map, values outside [0, K] -> K
__global__ void __launch_bounds__(256) pack_labels_kernel(const int* __restrict__ labels, int K, LabelGrid G, unsigned* __restrict__ map) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)G.H * G.W) return;
    const int g = labels[p];
    store_label(map, p, G, (g < 0 || g > K) ? K : g);
}

// per pixel: argmax, count (pred, gt) in conf.  kKeepMaps: also keep what was counted, maps[0] = argmax, maps[1] = ground truth
// (ignore -> K), and conf may be null
template <bool kKeepMaps>
__global__ void __launch_bounds__(256) semantic_confusion_kernel(const float* __restrict__ sem, const int* __restrict__ gt, int K, int npix_, LabelGrid G,
                                                                unsigned long long* __restrict__ conf, unsigned* __restrict__ maps) {
    const int64_t npix = kKeepMaps ? (int64_t)G.H * G.W : npix_;   // without maps there is no grid
    const int n = (K + 1) * (K + 1);
    const bool count = !kKeepMaps || conf;
    const LdsHist<unsigned long long> H(conf, n, count && n <= kLdsHistCells);
    H.clear();
    H.sync();
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int bi = argmax_first(sem, K, npix, p);
        int g = gt[p];
        g = (g < 0 || g > K) ? K : g;
        if (kKeepMaps) {
            store_label(maps, p, G, bi);
            store_label(maps + (int64_t)G.H * G.Pd, p, G, g);
        }
        if (count) H.add(bi * (K + 1) + g, 1u);
    }
    H.sync();
    H.flush();
}

// odise_hip_semantic_eval: per pixel the label - the arg-max, taken here once and kept in lab_out (kSem), or the caller's map - and, with a
// ground truth, what semantic_confusion_kernel counts of it: (label, gt) in conf (optional) and the two byte maps (kMaps).  A label
// outside [0, K) (possible only in a caller's map) raises flag 1, is counted in no cell and stands as K in the byte map.
template <bool kSem, bool kMaps>
__global__ void __launch_bounds__(256) semantic_eval_kernel(const float* __restrict__ sem, const int* __restrict__ labels, const int* __restrict__ gt, int K,
                                                           LabelGrid G, unsigned long long* __restrict__ conf, unsigned* __restrict__ maps,
                                                           int* __restrict__ lab_out, int* __restrict__ flags) {
    const int64_t npix = (int64_t)G.H * G.W;
    const int n = (K + 1) * (K + 1);
    const bool count = conf != nullptr;
    const LdsHist<unsigned long long> H(conf, n, count && n <= kLdsHistCells);
    H.clear();
    H.sync();
    bool bad = false;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        int l;
        bool in = true;
        if (kSem) {
            l = argmax_first(sem, K, npix, p);
            if (lab_out) lab_out[p] = l;   // only the strings read it
        } else {
            l = labels[p];
            in = (unsigned)l < (unsigned)K;
            bad |= !in;
        }
        if (gt) {
            int g = gt[p];
            g = (g < 0 || g > K) ? K : g;
            if (kMaps) {
                store_label(maps, p, G, in ? l : K);
                store_label(maps + (int64_t)G.H * G.Pd, p, G, g);
            }
            if (count && in) H.add(l * (K + 1) + g, 1u);
        }
    }
    H.sync();
    H.flush();
    if (!kSem && bad) atomicOr(flags, 1);
}

// dst = per-byte minimum of taps.n copies of src shifted by taps.off pixels along the rows (vertical == 0) or the columns; 0 outside
__global__ void __launch_bounds__(256) min_taps_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst, LabelGrid G, MinTaps taps,
                                                      int vertical) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, per_map = (int64_t)G.H * G.Pd;
    if (i >= per_map) return;
    const int y = (int)(i / G.Pd), xd = (int)(i - (int64_t)y * G.Pd);
    const unsigned* map = src + blockIdx.y * per_map;
    unsigned v = ~0u;
#pragma unroll
    for (int k = 0; k < kMinTaps; ++k)
        if (k < taps.n) v = min_u8x4(v, vertical ? label_window(map, y + taps.off[k], xd, 0, G) : label_window(map, y, xd, taps.off[k], G));
    dst[blockIdx.y * per_map + i] = v;
}

// boundary int32 [H, W] = m - e of one map
__global__ void __launch_bounds__(256) unpack_boundary_kernel(const unsigned* __restrict__ m, const unsigned* __restrict__ e, LabelGrid G,
                                                             int* __restrict__ boundary) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)G.H * G.W) return;
    const int y = (int)(p / G.W), x = (int)(p - (int64_t)y * G.W);
    const int64_t b = (int64_t)y * G.Pd * 4 + x;
    boundary[p] = (int)((const uint8_t*)m)[b] - (int)((const uint8_t*)e)[b];
}

// b_conf[(m0 - e0) * (K + 1) + (m1 - e1)] += 1 per pixel; m, e = [2][H][Pd]
__global__ void __launch_bounds__(256) boundary_confusion_kernel(const unsigned* __restrict__ m, const unsigned* __restrict__ e, int K, LabelGrid G,
                                                                unsigned long long* __restrict__ b_conf) {
    __shared__ unsigned int zeros;          // cell (0, 0): all pixels that lie on no boundary in either map
    const int n = (K + 1) * (K + 1);
    const LdsHist<unsigned long long> H(b_conf, n, n <= kLdsHistCells);
    H.clear();
    if (threadIdx.x == 0) zeros = 0;
    __syncthreads();
    const int64_t per_map = (int64_t)G.H * G.Pd;
    unsigned own_zeros = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_map; i += (int64_t)gridDim.x * blockDim.x) {
        const int xd = (int)(i % G.Pd);
        const int nb = min(4, G.W - 4 * xd);
        // m >= e in every byte, so the dword difference borrows nowhere below the (ignored) bytes past W
        const unsigned bp = m[i] - e[i], bg = m[per_map + i] - e[per_map + i];
        for (int j = 0; j < nb; ++j) {
            const int cell = (int)((bp >> (8 * j)) & 255u) * (K + 1) + (int)((bg >> (8 * j)) & 255u);
            if (cell == 0) ++own_zeros;
            else if (cell >= n) continue;   // cannot happen for labels <= K; never write past the matrix
            else H.add(cell, 1u);
        }
    }
    if (own_zeros) atomicAdd(&zeros, own_zeros);
    __syncthreads();
    if (threadIdx.x == 0 && zeros) atomicAdd(&b_conf[0], (unsigned long long)zeros);
    H.flush();
}

__global__ void __launch_bounds__(256) pair_histogram_kernel(const int* __restrict__ a, const int* __restrict__ b, int npix, int na, int nb,
                                                            unsigned int* __restrict__ out) {
    const int n = na * nb;
    const LdsHist<unsigned> H(out, n, n <= kLdsHistCells);
    H.clear();
    H.sync();
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int ia = a[p], ib = b[p];
        if ((unsigned)ia < (unsigned)na && (unsigned)ib < (unsigned)nb) H.add(ia * nb + ib, 1u);
    }
    H.sync();
    H.flush();
}

static int upload_coeffs(odise_hip_ctx* ctx, const ResampleCoeffs& c, int** d_bounds, int** d_kk) {
    ODISE_CHECK_HIP(hipMalloc((void**)d_bounds, c.bounds.size() * sizeof(int)));
    ODISE_CHECK_HIP(hipMalloc((void**)d_kk, c.kk.size() * sizeof(int)));
    ODISE_CHECK_HIP(hipMemcpyAsync(*d_bounds, c.bounds.data(), c.bounds.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    ODISE_CHECK_HIP(hipMemcpyAsync(*d_kk, c.kk.data(), c.kk.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    return ODISE_OK;
}

int boundary_radius(int H, int W) {   // _mask_to_boundary: max(1, int(round(0.02 * sqrt(h^2 + w^2)))), Python's round (half to even)
    const double r = nearbyint(0.02 * sqrt((double)H * H + (double)W * W));
    return r < 1.0 ? 1 : (int)r;
}

// the context's scratch for the byte maps of one picture (grown on demand; earlier calls on the stream may still read the old buffer)
int boundary_maps(odise_hip_ctx* ctx, int H, int W, int nmaps, BoundaryMaps* b) {
    b->G.H = H; b->G.W = W; b->G.Pd = (int)ceil_div(W, 4);
    b->G.tail = (W & 3) ? (1u << (8 * (W & 3))) - 1u : ~0u;
    b->per_map = (int64_t)H * b->G.Pd;
    const size_t each = (size_t)round_up(nmaps * b->per_map * 4, 256), need = 3 * each;
    ODISE_TRY(scratch_reserve(ctx->boundary, need, 0, drain_streams(ctx->stream), "boundary"));
    char* p = (char*)ctx->boundary.ptr;
    b->m = (unsigned*)p;
    b->e = (unsigned*)(p + each);
    b->tmp = (unsigned*)(p + 2 * each);
    return ODISE_OK;
}

// b->e = the (2r+1)^2 minimum of b->m with zeros outside the picture
int erode_maps(odise_hip_ctx* ctx, BoundaryMaps* b, int nmaps, int r) {
    const LabelGrid& G = b->G;
    if (2 * (int64_t)r + 1 > std::min(G.H, G.W)) {   // every window leaves the picture
        ODISE_CHECK_HIP(hipMemsetAsync(b->e, 0, (size_t)nmaps * b->per_map * 4, ctx->stream));
        return ODISE_OK;
    }
    const int w = 2 * r + 1;
    const dim3 grid((unsigned)ceil_div(b->per_map, 256), (unsigned)nmaps);
    const unsigned* cur = b->m;
    for (int vertical = 0; vertical < 2; ++vertical) {
        int s = 1;   // cur holds the minima of the windows [x, x + s)
        for (bool last = false; !last; s *= kMinTaps) {
            MinTaps taps;
            last = ceil_div(w, s) <= kMinTaps;
            taps.n = last ? (int)ceil_div(w, s) : kMinTaps;
            for (int k = 0; k < kMinTaps; ++k) taps.off[k] = last ? (k < taps.n - 1 ? k * s - r : r + 1 - s) : k * s;
            unsigned* dst = cur == b->e ? b->tmp : b->e;
            hipLaunchKernelGGL(min_taps_kernel, grid, dim3(256), 0, ctx->stream, cur, dst, G, taps, vertical);
            ODISE_CHECK_HIP(hipGetLastError());
            cur = dst;
        }
    }
    if (cur != b->e) std::swap(b->e, b->tmp);
    return ODISE_OK;
}

static int boundary_args(const char* what, int K, int H, int W) {
    ODISE_REQUIRE(K >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= INT32_MAX, "%s: bad dims (K %d, %dx%d)", what, K, H, W);
    ODISE_REQUIRE(K <= 254, "%s: K = %d; SemSegEvaluator switches Boundary IoU off for 255 classes and more (labels and the ignore label share a byte)",
                  what, K);
    return ODISE_OK;
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_resize_bilinear_u8(odise_hip_ctx* ctx, const void* src, int H, int W, int C, void* dst, int OH, int OW) {
    ODISE_REQUIRE(ctx && src && dst, "resize_bilinear_u8: null argument");
    ODISE_REQUIRE(H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, "resize_bilinear_u8: bad dims");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const uint8_t* cur = (const uint8_t*)src;
    uint8_t* tmp = nullptr;
    int *bh = nullptr, *kh = nullptr, *bv = nullptr, *kv = nullptr;
    int rc = ODISE_OK;
    if (OW != W) {  // horizontal pass first (ImagingResampleInner); its output is the final image when the height is unchanged
        ResampleCoeffs c;
        precompute_coeffs(W, OW, c);
        rc = upload_coeffs(ctx, c, &bh, &kh);
        uint8_t* out = (uint8_t*)dst;
        if (rc == ODISE_OK && OH != H) {
            if (hipMalloc((void**)&tmp, (size_t)H * OW * C) != hipSuccess) { set_error("resize_bilinear_u8: out of memory"); rc = ODISE_ERR_NOMEM; }
            out = tmp;
        }
        if (rc == ODISE_OK) {
            const int64_t total = (int64_t)H * OW * C;
            hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, cur, out, bh, kh, H, W, OW, C, c.ksize);
            cur = out;
        }
    }
    if (rc == ODISE_OK && OH != H) {
        ResampleCoeffs c;
        precompute_coeffs(H, OH, c);
        rc = upload_coeffs(ctx, c, &bv, &kv);
        if (rc == ODISE_OK) {
            const int row_bytes = OW * C;
            const int64_t total = (int64_t)OH * row_bytes;
            hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, cur, (uint8_t*)dst, bv, kv, OH, row_bytes, c.ksize);
        }
    } else if (rc == ODISE_OK && OW == W) {
        if (hipMemcpyAsync(dst, src, (size_t)H * W * C, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) rc = ODISE_ERR_HIP;
    }
    // the coefficient tables and the intermediate image are per-call temporaries: wait for the stream, then free them
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == ODISE_OK) { set_error("resize_bilinear_u8: stream error"); rc = ODISE_ERR_HIP; }
    for (void* p : {(void*)tmp, (void*)bh, (void*)kh, (void*)bv, (void*)kv})
        if (p) (void)hipFree(p);
    return rc;
}

extern "C" int odise_hip_u8_hwc_to_f32_chw(odise_hip_ctx* ctx, const void* src, float* dst, int H, int W, int C, float scale) {
    ODISE_REQUIRE(ctx && src && dst && H > 0 && W > 0 && C > 0, "u8_hwc_to_f32_chw: bad argument");
    const int64_t total = (int64_t)H * W * C;
    hipLaunchKernelGGL(u8_hwc_to_f32_chw_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)src, dst, H * W, C, scale);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_u8_hwc_to_f32_chw_padded(odise_hip_ctx* ctx, const void* src, float* dst, int H, int W, int C, int Hp, int Wp, float scale) {
    ODISE_REQUIRE(ctx && src && dst && H > 0 && W > 0 && C > 0 && Hp >= H && Wp >= W, "u8_hwc_to_f32_chw_padded: bad argument");
    const int64_t total = (int64_t)Hp * Wp * C;
    hipLaunchKernelGGL(u8_hwc_to_f32_chw_pad_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)src, dst, H, W, C,
                       Hp, Wp, scale);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_semantic_confusion(odise_hip_ctx* ctx, const float* sem_seg, const int* gt, int K, int npix, int64_t* conf) {
    ODISE_REQUIRE(ctx && sem_seg && gt && conf && K >= 1 && npix > 0, "semantic_confusion: bad argument");
    const int blocks = (int)std::min<int64_t>(ceil_div(npix, 256), 4 * ctx->cu_count);
    hipLaunchKernelGGL(semantic_confusion_kernel<false>, dim3(blocks), dim3(256), lds_hist_bytes((K + 1) * (K + 1)), ctx->stream, sem_seg, gt, K, npix,
                       LabelGrid{}, (unsigned long long*)conf, (unsigned*)nullptr);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_boundary_radius(int H, int W) {
    ODISE_REQUIRE(H >= 1 && W >= 1, "boundary_radius: bad size %dx%d", H, W);
    return boundary_radius(H, W);
}

extern "C" int odise_hip_label_boundary(odise_hip_ctx* ctx, const int* labels, int K, int H, int W, int radius, int* boundary) {
    ODISE_TRY(boundary_args("label_boundary", K, H, W));
    ODISE_REQUIRE(ctx && labels && boundary, "label_boundary: null argument");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    BoundaryMaps b;
    ODISE_TRY(boundary_maps(ctx, H, W, 1, &b));
    const dim3 per_pixel((unsigned)ceil_div((int64_t)H * W, 256));
    hipLaunchKernelGGL(pack_labels_kernel, per_pixel, dim3(256), 0, ctx->stream, labels, K, b.G, b.m);
    ODISE_CHECK_HIP(hipGetLastError());
    ODISE_TRY(erode_maps(ctx, &b, 1, radius > 0 ? radius : boundary_radius(H, W)));
    hipLaunchKernelGGL(unpack_boundary_kernel, per_pixel, dim3(256), 0, ctx->stream, b.m, b.e, b.G, boundary);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_semantic_boundary_confusion(odise_hip_ctx* ctx, const float* sem_seg, const int* gt, int K, int H, int W, int radius,
                                                     int64_t* conf, int64_t* b_conf) {
    ODISE_TRY(boundary_args("semantic_boundary_confusion", K, H, W));
    ODISE_REQUIRE(ctx && sem_seg && gt && b_conf, "semantic_boundary_confusion: null argument");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    BoundaryMaps b;
    ODISE_TRY(boundary_maps(ctx, H, W, 2, &b));
    const size_t lds = lds_hist_bytes((K + 1) * (K + 1));
    int blocks = (int)std::min<int64_t>(ceil_div((int64_t)H * W, 256), 4 * ctx->cu_count);
    hipLaunchKernelGGL(semantic_confusion_kernel<true>, dim3(blocks), dim3(256), conf ? lds : 0, ctx->stream, sem_seg, gt, K, H * W, b.G,
                       (unsigned long long*)conf, b.m);
    ODISE_CHECK_HIP(hipGetLastError());
    ODISE_TRY(erode_maps(ctx, &b, 2, radius > 0 ? radius : boundary_radius(H, W)));
    blocks = (int)std::min<int64_t>(ceil_div(b.per_map, 256), 4 * ctx->cu_count);
    hipLaunchKernelGGL(boundary_confusion_kernel, dim3(blocks), dim3(256), lds, ctx->stream, b.m, b.e, K, b.G, (unsigned long long*)b_conf);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

// odise_hip_semantic_eval, and with `t` odise_hip_semantic_eval_pq: the same launches in the same order, then the PQ statistics of the same label map
static int semantic_eval_run(odise_hip_ctx* ctx, const odise_semseg_eval_desc* d, const odise_semseg_pq_task* t) {
    ODISE_REQUIRE(ctx && d, "semantic_eval: null argument");
    ODISE_REQUIRE((d->labels != nullptr) != (d->sem_seg != nullptr), "semantic_eval: exactly one of labels / sem_seg");
    ODISE_REQUIRE(d->flags, "semantic_eval: null flags");
    const int K = d->K, H = d->H, W = d->W;
    const bool counting = d->conf || d->b_conf, strings = d->offsets != nullptr;
    ODISE_REQUIRE(counting || strings || t, "semantic_eval: nothing to do (no conf, no b_conf, no offsets)");
    ODISE_REQUIRE(!(counting || t) || d->gt, "semantic_eval: counting needs a ground truth");
    ODISE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= kSemEvalMaxPixels, "semantic_eval: picture size %dx%d out of range", H, W);
    ODISE_REQUIRE(K >= 1 && K <= kLdsHistCells, "semantic_eval: %d classes (1..%d)", K, kLdsHistCells);
    if (d->b_conf) ODISE_TRY(boundary_args("semantic_eval", K, H, W));
    if (strings) {
        ODISE_REQUIRE(d->classes && d->n_classes, "semantic_eval: the strings need classes and n_classes");
        ODISE_REQUIRE(d->max_classes >= 1 && d->max_classes <= 65535, "semantic_eval: max_classes %d (1..65535)", d->max_classes);
        ODISE_REQUIRE(d->capacity >= 0 && (d->rle || d->capacity == 0), "semantic_eval: capacity %lld without an output buffer", (long long)d->capacity);
    }
    ODISE_REQUIRE((((uintptr_t)d->labels | (uintptr_t)d->sem_seg | (uintptr_t)d->gt | (uintptr_t)d->classes | (uintptr_t)d->n_classes | (uintptr_t)d->flags) & 3) == 0 &&
                      (((uintptr_t)d->conf | (uintptr_t)d->b_conf | (uintptr_t)d->offsets | (uintptr_t)d->area) & 7) == 0,
                  "semantic_eval: int32 / float buffers must be 4-byte aligned, int64 buffers 8-byte aligned");
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const RleGrid RG = rle_grid(H, W);
    const int nmask = strings ? std::min(d->max_classes, K) : 0;
    SemRleScratch s{};
    if (strings || (t && d->sem_seg)) ODISE_TRY(sem_rle_scratch(ctx, nmask, RG, K, d->sem_seg != nullptr, &s));   // count only: no label map is kept
    BoundaryMaps b{};
    if (d->b_conf) ODISE_TRY(boundary_maps(ctx, H, W, 2, &b));
    else { b.G.H = H; b.G.W = W; }
    const int* labels = d->sem_seg ? s.labels : d->labels;
    if (d->sem_seg || counting) {   // with a caller's map and no ground truth the labels are first read by the RLE passes
        const size_t lds = d->conf ? lds_hist_bytes((K + 1) * (K + 1)) : 0;
        const dim3 grid((unsigned)std::min<int64_t>(ceil_div((int64_t)H * W, 256), 4 * ctx->cu_count));
        unsigned long long* conf = (unsigned long long*)d->conf;
        const int* gt = counting ? d->gt : nullptr;
        if (d->sem_seg && d->b_conf)
            hipLaunchKernelGGL((semantic_eval_kernel<true, true>), grid, dim3(256), lds, ctx->stream, d->sem_seg, (const int*)nullptr, gt, K, b.G, conf, b.m, s.labels, d->flags);
        else if (d->sem_seg)
            hipLaunchKernelGGL((semantic_eval_kernel<true, false>), grid, dim3(256), lds, ctx->stream, d->sem_seg, (const int*)nullptr, gt, K, b.G, conf, b.m, s.labels, d->flags);
        else if (d->b_conf)
            hipLaunchKernelGGL((semantic_eval_kernel<false, true>), grid, dim3(256), lds, ctx->stream, (const float*)nullptr, d->labels, gt, K, b.G, conf, b.m, (int*)nullptr, d->flags);
        else
            hipLaunchKernelGGL((semantic_eval_kernel<false, false>), grid, dim3(256), lds, ctx->stream, (const float*)nullptr, d->labels, gt, K, b.G, conf, b.m, (int*)nullptr, d->flags);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    if (d->b_conf) {
        ODISE_TRY(erode_maps(ctx, &b, 2, d->radius > 0 ? d->radius : boundary_radius(H, W)));
        const int blocks = (int)std::min<int64_t>(ceil_div(b.per_map, 256), 4 * ctx->cu_count);
        hipLaunchKernelGGL(boundary_confusion_kernel, dim3(blocks), dim3(256), lds_hist_bytes((K + 1) * (K + 1)), ctx->stream, b.m, b.e, K, b.G,
                           (unsigned long long*)d->b_conf);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    if (strings)
        ODISE_TRY(sem_rle_encode(ctx, s, RG, labels, K, nmask, d->max_classes, d->classes, d->n_classes, d->rle, d->capacity, d->offsets, d->area, d->flags));
    if (t) ODISE_TRY(sem_pq_enqueue(ctx, labels, nullptr, d->gt, K, H, W, t->stats, d->flags));   // the labels: the caller's, or the arg-max kept above
    return ODISE_OK;
}

extern "C" int odise_hip_semantic_eval(odise_hip_ctx* ctx, const odise_semseg_eval_desc* d) { return semantic_eval_run(ctx, d, nullptr); }

extern "C" int odise_hip_semantic_eval_pq(odise_hip_ctx* ctx, const odise_semseg_eval_desc* d, const odise_semseg_pq_task* t) {
    ODISE_REQUIRE(ctx && d && t && t->stats, "semantic_eval_pq: null argument, task or statistics");
    ODISE_REQUIRE(d->gt, "semantic_eval_pq: the statistics need a ground truth");
    ODISE_REQUIRE(((uintptr_t)t->stats & 7) == 0, "semantic_eval_pq: the statistics must be 8-byte aligned");
    return semantic_eval_run(ctx, d, t);
}

extern "C" int odise_hip_pair_histogram(odise_hip_ctx* ctx, const int* a, const int* b, int npix, int na, int nb, int* hist) {
    ODISE_REQUIRE(ctx && a && b && hist && npix > 0 && na > 0 && nb > 0, "pair_histogram: bad argument");
    const int blocks = (int)std::min<int64_t>(ceil_div(npix, 256), 4 * ctx->cu_count);
    hipLaunchKernelGGL(pair_histogram_kernel, dim3(blocks), dim3(256), lds_hist_bytes(na * nb), ctx->stream, a, b, npix, na, nb, (unsigned int*)hist);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}
