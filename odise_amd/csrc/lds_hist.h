// lds_hist.h — the per-block counting histogram (eval_ops.hip, pq.hip, sem_pq.hip, track.hip, vis_inst.hip), the run of equal cells that a
// lane counts in a register before it touches the histogram (pq.hip, sem_pq.hip, track.hip), and the arg-max over class planes that feeds
// it (eval_ops.hip, sem_pq.hip, vis_inst.hip).
//
// A block counts `n` cells in the dynamic LDS of its launch and adds the non-zero ones to the global matrix with integer atomics when it is
// done (deterministic: integer addition commutes); a matrix of more than kLdsHistCells cells is counted in global memory directly.  Which of
// the two is decided once per block and is uniform across it.  The kernel places the barriers, one between clear() and the first add() and
// one between the last add() and flush(): sync(), or its own __syncthreads() where it has shared state of its own to publish there.
#pragma once
#include "common.h"

namespace odise {

constexpr int kLdsHistCells = 12288;   // 48 KiB of unsigned counters

// dynamic LDS bytes to launch with for n cells; 0 = they do not fit, the kernel counts in global memory
static inline size_t lds_hist_bytes(int64_t n) { return n <= kLdsHistCells ? (size_t)n * sizeof(unsigned) : 0; }

template <class Cell>   // the global matrix: unsigned long long (confusion matrices), unsigned / int (pair histogram, panoptic quality)
struct LdsHist {
    Cell* global;
    int n;
    bool lds;   // uniform across the block; true needs a launch with (at least) lds_hist_bytes(n) of dynamic LDS
    __device__ __forceinline__ LdsHist(Cell* global_, int n_, bool lds_) : global(global_), n(n_), lds(lds_) {}
    __device__ __forceinline__ static unsigned* cells() {
        extern __shared__ unsigned lds_hist_cells[];
        return lds_hist_cells;
    }
    __device__ __forceinline__ void clear() const {
        if (lds)
            for (int i = threadIdx.x; i < n; i += blockDim.x) cells()[i] = 0;
    }
    __device__ __forceinline__ void sync() const {   // nothing to wait for when the counts go to global memory
        if (lds) __syncthreads();
    }
    // the two halves of add(), for a kernel that hoists the decision out of its pixel loop
    __device__ __forceinline__ void add_lds(int cell, unsigned count) const { atomicAdd(&cells()[cell], count); }
    __device__ __forceinline__ void add_global(int cell, unsigned count) const { atomicAdd(&global[cell], (Cell)count); }
    __device__ __forceinline__ void add(int cell, unsigned count) const {
        if (lds) add_lds(cell, count);
        else add_global(cell, count);
    }
    __device__ __forceinline__ void flush() const {
        if (lds)
            for (int i = threadIdx.x; i < n; i += blockDim.x)
                if (const unsigned c = cells()[i]) add_global(i, c);
    }
};

// A run of equal cells counted in a register and added to the histogram when the cell changes.  LDS = H.lds, decided once per kernel: the
// pixel loop is a template over it.  The bounds guard is for track.hip, whose cells come from bytes of retained maps (a byte is at most that
// frame's row count: always inside); in pq.hip a cell is below H.n by construction and the guard costs one compare per change of pair;
// sem_pq.hip counts "no cell" as cell -1, which the guard drops.
struct HistRun {
    int cell = 0, run = 0;
    template <bool LDS, class Cell>
    __device__ __forceinline__ void flush(const LdsHist<Cell>& H) const {
        if (run && (unsigned)cell < (unsigned)H.n) {
            if (LDS) H.add_lds(cell, (unsigned)run);
            else H.add_global(cell, (unsigned)run);
        }
    }
    template <bool LDS, class Cell>
    __device__ __forceinline__ void count(int c, const LdsHist<Cell>& H) {
        if (c == cell) { ++run; return; }
        flush<LDS>(H);
        cell = c;
        run = 1;
    }
};

// first-maximum argmax over the K planes of pixel p (torch.argmax semantics for distinct values; ties -> lowest class)
__device__ __forceinline__ int argmax_first(const float* __restrict__ sem, int K, int64_t npix, int64_t p) {
    float best = sem[p];
    int bi = 0;
    for (int k = 1; k < K; ++k) {
        const float v = sem[(int64_t)k * npix + p];
        if (v > best) { best = v; bi = k; }
    }
    return bi;
}

}  // namespace odise
