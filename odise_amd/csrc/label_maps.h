// label_maps.h — the byte label maps of the boundary measures and their erosion, shared by eval_ops.hip (Boundary IoU of SemSegEvaluator,
// where the kernels and the host functions live) and pq.hip (Boundary PQ: the maps hold table slots).
#pragma once
#include "common.h"

namespace odise {

// A byte label map is [H][Pd] dwords, Pd = ceil(W / 4), byte x & 3 of dword x >> 2; the bytes past W in a row's last dword are never
// initialised: every dword read masks them (`tail`).  Two maps (prediction, ground truth) lie back to back and share a launch (blockIdx.y).
struct LabelGrid {
    int H, W, Pd;
    unsigned tail;   // the valid bytes of a row's last dword
};

__device__ __forceinline__ void store_label(unsigned* __restrict__ map, int64_t p, const LabelGrid& G, int v) {
    const int y = (int)(p / G.W), x = (int)(p - (int64_t)y * G.W);
    ((uint8_t*)map)[(int64_t)y * G.Pd * 4 + x] = (uint8_t)v;
}

struct BoundaryMaps {
    LabelGrid G;
    int64_t per_map;   // dwords
    unsigned *m, *e;   // [nmaps] label maps and, after erode_maps, their erosions
    unsigned* tmp;
};

int boundary_radius(int H, int W);   // _mask_to_boundary: max(1, int(round(0.02 * sqrt(h^2 + w^2)))), Python's round (half to even)
// the context's scratch for the byte maps of one picture (grown on demand; earlier calls on the stream may still read the old buffer)
int boundary_maps(odise_hip_ctx* ctx, int H, int W, int nmaps, BoundaryMaps* b);
// b->e = the (2r+1)^2 minimum of b->m with zeros outside the picture
int erode_maps(odise_hip_ctx* ctx, BoundaryMaps* b, int nmaps, int r);

}  // namespace odise
