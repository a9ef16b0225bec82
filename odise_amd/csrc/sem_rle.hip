// sem_rle.hip — COCO RLE of every class of a semantic label map on the device: the second half of detectron2's SemSegEvaluator.process
// (encode_json_sem_seg: for label in np.unique(pred): mask_util.encode(np.array((pred == label)[:, :, None], order="F")), the strings of
// sem_seg_predictions.json).  A label map is the easy case of rle.hip: its classes partition the picture, so ONE pass over the map packs
// the bit words of all the masks and the string passes of rle.hip (count -> offsets -> write, rle_pack.h) run on them unchanged.
//
//   1. present  per-block LDS histogram (lds_hist.h) of the labels in [0, K): counts[K]; a label outside raises flag 1 and is a zero in
//               every mask.
//   2. slots    one block: an exclusive scan of (count > 0) over the classes gives class -> slot in ASCENDING class order (np.unique's
//               order), slot 0xffff for an absent class and for the classes past max_classes; classes / n_classes are written here.
//   3. clear    the words of the min(n, max_classes) masks that exist (the count is read on the device).
//   4. pack     thread (x, r) walks rows 64 r .. 64 r + 63 of column x (consecutive lanes = consecutive columns: coalesced row reads),
//               translates label -> slot through the table in LDS only when the label differs from the lane's previous one, keeps the
//               current (slot, bits) in registers and ORs the bits into word (x, r) of that slot's mask when the slot changes.  It is the
//               only writer of word (x, r) of EVERY mask: plain loads and stores, no atomics, and a vertical run costs one word access.
//   5. strings  rle_finish on those words; area = the ones of each mask.
// Integer work only: the output is deterministic.
#include <algorithm>

#include "lds_hist.h"
#include "rle_pack.h"

namespace odise {

constexpr unsigned kSemNoSlot = 0xffffu;
constexpr int kSemPackThreads = 64;    // columns per block of the pack pass (one wave)
constexpr int kSemPackBatch = 8;       // rows loaded ahead of their use

__global__ void __launch_bounds__(256) sem_present_kernel(const int* __restrict__ labels, int K, int npix, unsigned* __restrict__ counts,
                                                         int* __restrict__ flags) {
    const LdsHist<unsigned> Hh(counts, K, true);   // K <= kLdsHistCells: always in LDS
    Hh.clear();
    Hh.sync();
    bool bad = false;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        const int l = labels[p];
        if ((unsigned)l < (unsigned)K) Hh.add_lds(l, 1u);
        else bad = true;
    }
    Hh.sync();
    Hh.flush();
    if (bad) atomicOr(flags, 1);
}

// One block of kRleThreads.  slot[c] = the rank of class c among the present classes (kSemNoSlot: absent, or rank >= max_classes).
__global__ void __launch_bounds__(kRleThreads) sem_slots_kernel(const unsigned* __restrict__ counts, int K, int max_classes, unsigned short* __restrict__ slot,
                                                               int* __restrict__ n_enc, int* __restrict__ classes, int* __restrict__ n_classes) {
    __shared__ long long ls[kRleThreads / 64];
    const int t = threadIdx.x;
    const int per = (K + kRleThreads - 1) / kRleThreads;
    const int a = min(K, t * per), b = min(K, a + per);
    long long own = 0;
    for (int c = a; c < b; ++c) own += counts[c] > 0u ? 1 : 0;
    long long total;
    int rank = (int)block_scan_sum(own, ls, total);
    for (int c = a; c < b; ++c) {
        unsigned s = kSemNoSlot;
        if (counts[c] > 0u) {
            if (rank < max_classes) {
                s = (unsigned)rank;
                classes[rank] = c;
            }
            ++rank;
        }
        slot[c] = (unsigned short)s;
    }
    const int n = (int)min(total, (long long)max_classes);
    if (t == 0) {
        *n_classes = (int)total;
        *n_enc = n;
    }
    for (int i = n + t; i < max_classes; i += kRleThreads) classes[i] = -1;
}

__global__ void __launch_bounds__(256) sem_clear_kernel(unsigned long long* __restrict__ words, int64_t nw, const int* __restrict__ n_enc) {
    if ((int)blockIdx.y >= *n_enc) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nw) words[(int64_t)blockIdx.y * nw + i] = 0ull;
}

__global__ void __launch_bounds__(kSemPackThreads) sem_pack_kernel(const int* __restrict__ labels, int K, const unsigned short* __restrict__ slot, RleGrid G,
                                                                  unsigned long long* __restrict__ words) {
    extern __shared__ unsigned short tab[];   // [K]: the launch sizes it
    for (int c = threadIdx.x; c < K; c += kSemPackThreads) tab[c] = slot[c];
    __syncthreads();
    const int xb = (G.w + kSemPackThreads - 1) / kSemPackThreads;   // blockIdx.x = r * xb + (block of columns): gridDim.y would cap H at 64 * 65535
    const int r = blockIdx.x / xb, x = (blockIdx.x - r * xb) * kSemPackThreads + threadIdx.x;
    if (x >= G.w) return;
    const int rows = min(64, G.h - 64 * r);
    const int* src = labels + (int64_t)64 * r * G.w + x;
    unsigned long long* col = words + (int64_t)x * G.R + r;   // word (x, r) of mask 0
    int last = -1;                      // the lane's previous label and its translation
    unsigned last_slot = kSemNoSlot;
    unsigned cur = kSemNoSlot;          // the mask the bits in flight belong to
    unsigned long long bits = 0ull;
    for (int k0 = 0; k0 < rows; k0 += kSemPackBatch) {
        int l[kSemPackBatch];
#pragma unroll
        for (int j = 0; j < kSemPackBatch; ++j) l[j] = k0 + j < rows ? src[(int64_t)(k0 + j) * G.w] : last;
#pragma unroll
        for (int j = 0; j < kSemPackBatch; ++j) {
            if (k0 + j >= rows) break;
            if (l[j] != last) {
                last = l[j];
                last_slot = (unsigned)last < (unsigned)K ? (unsigned)tab[last] : kSemNoSlot;
                if (last_slot != cur) {
                    if (cur != kSemNoSlot) col[(int64_t)cur * G.nw] |= bits;
                    cur = last_slot;
                    bits = 0ull;
                }
            }
            bits |= 1ull << (k0 + j);
        }
    }
    if (cur != kSemNoSlot) col[(int64_t)cur * G.nw] |= bits;
}

// offsets (nmask, max_classes] = offsets[nmask], area [nmask, max_classes) = 0: the entries that no class can fill (max_classes > K)
__global__ void __launch_bounds__(256) sem_tail_kernel(long long* __restrict__ offsets, long long* __restrict__ area, int nmask, int max_classes) {
    const long long end = offsets[nmask];
    for (int i = nmask + blockIdx.x * blockDim.x + threadIdx.x; i < max_classes; i += gridDim.x * blockDim.x) {
        offsets[i + 1] = end;
        if (area) area[i] = 0;
    }
}

int sem_rle_scratch(odise_hip_ctx* ctx, int nmask, const RleGrid& G, int K, bool own_labels, SemRleScratch* s) {
    const size_t lb = own_labels ? (size_t)round_up((int64_t)G.h * G.w * 4, 256) : 0;
    const size_t cb = nmask ? (size_t)round_up((int64_t)K * 4, 256) : 0, sb = nmask ? (size_t)round_up((int64_t)K * 2, 256) : 0;
    ODISE_TRY(rle_scratch(ctx, nmask, G, &s->rle, lb + cb + sb + (nmask ? 256 : 0)));
    char* p = (char*)s->rle.extra;
    s->labels = own_labels ? (int*)p : nullptr;
    s->counts = (unsigned*)(p + lb);
    s->slot = (unsigned short*)(p + lb + cb);
    s->n_enc = (int*)(p + lb + cb + sb);
    return ODISE_OK;
}

int sem_rle_encode(odise_hip_ctx* ctx, const SemRleScratch& s, const RleGrid& G, const int* labels, int K, int nmask, int max_classes, int* classes,
                   int* n_classes, void* rle, int64_t capacity, int64_t* offsets, int64_t* area, int* flags) {
    const int npix = G.h * G.w;
    ODISE_CHECK_HIP(hipMemsetAsync(s.counts, 0, (size_t)K * 4, ctx->stream));
    hipLaunchKernelGGL(sem_present_kernel, dim3(grid_blocks(ctx, npix, 256)), dim3(256), lds_hist_bytes(K), ctx->stream, labels, K, npix, s.counts, flags);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sem_slots_kernel, dim3(1), dim3(kRleThreads), 0, ctx->stream, (const unsigned*)s.counts, K, max_classes, s.slot, s.n_enc, classes,
                       n_classes);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sem_clear_kernel, dim3((unsigned)ceil_div(G.nw, 256), (unsigned)nmask), dim3(256), 0, ctx->stream, s.rle.words, G.nw,
                       (const int*)s.n_enc);
    ODISE_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sem_pack_kernel, dim3((unsigned)(ceil_div(G.w, kSemPackThreads) * G.R)), dim3(kSemPackThreads), (size_t)round_up((int64_t)K * 2, 16), ctx->stream, labels, K,
                       (const unsigned short*)s.slot, G, s.rle.words);
    ODISE_CHECK_HIP(hipGetLastError());
    ODISE_TRY(rle_finish(ctx, s.rle, G, nmask, rle, capacity, offsets, area, s.n_enc));
    if (max_classes > nmask) {
        hipLaunchKernelGGL(sem_tail_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(max_classes - nmask, 256), 64)), dim3(256), 0, ctx->stream,
                           (long long*)offsets, (long long*)area, nmask, max_classes);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    return ODISE_OK;
}

}  // namespace odise
