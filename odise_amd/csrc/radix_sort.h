// radix_sort.h — a stable LSD radix sort of (64-bit key, 32-bit value) pairs on the device, 8 bits per pass, for inst_accum.hip and whoever
// needs a sort next (the instance top-k and the draw order rank by counting, which is quadratic).
//
//   per pass   1. hist     a block per tile of kSortTile pairs counts the digits of its tile: hist[digit][tile]
//              2. rows     a block per digit turns its row of `hist` into an exclusive scan over the tiles and keeps the row total
//              3. scatter  a block per tile scans the 256 totals (the first position of every digit), adds its own entry of `hist` and places
//                          its pairs.  A wave owns kSortItems * 64 consecutive pairs of the tile and takes them 64 at a time, in memory
//                          order: the lanes that hold the same digit find one another with eight ballots, the lowest of them takes the
//                          wave's counter of that digit, and a pair's place among its wave's pairs of that digit is the counter plus the
//                          peers in lower lanes.  The waves of a block follow one another in memory, so a prefix over the wave counters
//                          finishes the position.
//
// Pairs with equal keys keep their order and every position is a function of the input alone: the same bytes from run to run.  n up to 2^31 - 1
// pairs as far as the indices go; the callers stay far below.  Everything is enqueued on the given stream; nothing waits.
#pragma once
#include "common.h"

namespace odise {

constexpr int kSortThreads = 256, kSortItems = 8, kSortTile = kSortThreads * kSortItems;   // 2048 pairs per block
typedef unsigned long long sort_key;

struct SortBufs {                // n pairs each way; the sort ping-pongs between (keys[0], vals[0]) and (keys[1], vals[1])
    sort_key* keys[2];
    uint32_t* vals[2];
    uint32_t* hist;              // [256][tiles] + [256] totals
};
static inline int64_t sort_tiles(int64_t n) { return ceil_div(n, kSortTile); }
static inline size_t sort_hist_bytes(int64_t n) { return (size_t)(256 * sort_tiles(n) + 256) * sizeof(uint32_t); }

// exclusive scan of one value per thread over the block's 256 threads; lds [4]; ends in a barrier
__device__ __forceinline__ uint32_t sort_block_scan(uint32_t v, uint32_t* lds, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < kSortThreads / 64; ++k) {
        if (k < wave) pre += lds[k];
        total += lds[k];
    }
    __syncthreads();
    return pre + inc - v;
}

__global__ void __launch_bounds__(kSortThreads) sort_hist_kernel(const sort_key* __restrict__ keys, int n, int shift, int tiles,
                                                                uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t0 = (int64_t)blockIdx.x * kSortTile;
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = t0 + j * kSortThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ void __launch_bounds__(kSortThreads) sort_rows_kernel(uint32_t* __restrict__ hist, int tiles) {
    __shared__ uint32_t lds[kSortThreads / 64];
    uint32_t* row = hist + (int64_t)blockIdx.x * tiles;
    uint32_t carry = 0;
    for (int t0 = 0; t0 < tiles; t0 += kSortThreads) {   // uniform trip count: the scan holds barriers
        const int t = t0 + threadIdx.x;
        const uint32_t v = t < tiles ? row[t] : 0u;
        uint32_t total;
        const uint32_t ex = sort_block_scan(v, lds, total);
        if (t < tiles) row[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) hist[(int64_t)256 * tiles + blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kSortThreads) sort_scatter_kernel(const sort_key* __restrict__ keys, const uint32_t* __restrict__ vals, int n,
                                                                   int shift, int tiles, const uint32_t* __restrict__ hist,
                                                                   sort_key* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t cnt[kSortThreads / 64][256];
    __shared__ uint32_t lds[kSortThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t total;
    const uint32_t first = sort_block_scan(hist[(int64_t)256 * tiles + tid], lds, total);   // where digit `tid` begins in the output
    const uint32_t base = first + hist[(int64_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kSortThreads / 64; ++w) cnt[w][tid] = 0;
    __syncthreads();
    const int64_t w0 = (int64_t)blockIdx.x * kSortTile + (int64_t)wave * (64 * kSortItems);
    const unsigned long long below = (1ull << lane) - 1ull;
    sort_key key[kSortItems];
    uint32_t val[kSortItems], rank[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = w0 + j * 64 + lane;
        const bool valid = i < n;
        key[j] = valid ? keys[i] : 0ull;
        val[j] = valid ? vals[i] : 0u;
        const uint32_t d = (uint32_t)(key[j] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long set = __ballot(valid && ((d >> b) & 1u));
            peers &= ((d >> b) & 1u) ? set : ~set;
        }
        uint32_t old = 0;
        const int leader = valid ? __ffsll(peers) - 1 : lane;
        if (valid && lane == leader) old = atomicAdd(&cnt[wave][d], (uint32_t)__popcll(peers));
        old = __shfl(old, leader);
        rank[j] = old + (uint32_t)__popcll(peers & below);
    }
    __syncthreads();
    {   // the counters of the waves become the first position of each wave's pairs of digit `tid`
        uint32_t run = base;
#pragma unroll
        for (int w = 0; w < kSortThreads / 64; ++w) {
            const uint32_t c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const int64_t i = w0 + j * 64 + lane;
        if (i < n) {
            const uint32_t pos = cnt[wave][(uint32_t)(key[j] >> shift) & 255u] + rank[j];
            if (pos < (uint32_t)n) {   // always, when `hist` was counted from these keys
                keys_out[pos] = key[j];
                vals_out[pos] = val[j];
            }
        }
    }
}

// Sorts the n pairs in (keys[0], vals[0]) by the key bits [0, bits), stable.  *where = 0 or 1: the side that holds the result.
static inline int radix_sort_pairs(hipStream_t stream, const SortBufs& s, int64_t n, int bits, int* where) {
    *where = 0;
    if (n <= 1) return ODISE_OK;
    const int tiles = (int)sort_tiles(n);
    int side = 0;
    for (int shift = 0; shift < bits; shift += 8, side ^= 1) {
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, stream, (const sort_key*)s.keys[side], (int)n, shift, tiles,
                           s.hist);
        ODISE_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(sort_rows_kernel, dim3(256), dim3(kSortThreads), 0, stream, s.hist, tiles);
        ODISE_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, stream, (const sort_key*)s.keys[side],
                           (const uint32_t*)s.vals[side], (int)n, shift, tiles, (const uint32_t*)s.hist, s.keys[side ^ 1], s.vals[side ^ 1]);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    *where = side;
    return ODISE_OK;
}

}  // namespace odise
