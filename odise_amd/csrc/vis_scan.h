// vis_scan.h — what the drawing kernels share (vis.hip: panoptic anchors; vis_inst.hip: instance anchors): the scan of a coordinate
// histogram for the two middle elements, and the size check of a picture.
#pragma once
#include "common.h"

namespace odise {

// The two middle elements of the sorted coordinates of N counted pixels (twice the median is their sum) and the first / last occupied
// bin of h[0 .. nb), by an inclusive scan 64 bins at a time.  Called by a whole wave; every lane returns the same four values
// (m1 = m2 = hi = -1, lo = INT32_MAX when nothing is counted).
__device__ __forceinline__ void vis_scan_middle(const int* __restrict__ h, int nb, int N, int lane, int& m1, int& m2, int& lo, int& hi) {
    const int k1 = (N - 1) >> 1, k2 = N >> 1;
    m1 = -1; m2 = -1; lo = INT32_MAX; hi = -1;
    int run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int i = b0 + lane, c = i < nb ? h[i] : 0;
        int inc = c;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        const int cum = run + inc, exc = cum - c;
        if (c > 0) {
            if (exc <= k1 && k1 < cum) m1 = i;
            if (exc <= k2 && k2 < cum) m2 = i;
            lo = min(lo, i);
            hi = max(hi, i);
        }
        run = __shfl(cum, 63);
    }
    for (int d = 32; d; d >>= 1) {
        m1 = max(m1, __shfl_xor(m1, d));
        m2 = max(m2, __shfl_xor(m2, d));
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
}

// an anchor row before its coordinates are scanned
__device__ __forceinline__ odise_anchor_row vis_anchor_row(int segment_row, int area) {
    odise_anchor_row r;
    r.segment_row = segment_row; r.area = area; r.x2 = 0; r.y2 = 0; r.x0 = 0; r.y0 = 0; r.x1 = 0; r.y1 = 0;
    return r;
}

constexpr int64_t kVisMaxPixels = INT32_MAX / 4;   // of a picture that is drawn
static inline int vis_check_size(const char* who, int H, int W) {
    ODISE_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W <= kVisMaxPixels, "%s: bad size %dx%d", who, H, W);
    return ODISE_OK;
}

}  // namespace odise
