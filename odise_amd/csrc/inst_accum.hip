// inst_accum.hip — odise_hip_instance_accumulate: COCOeval.accumulate of the segm evaluator on the rows that odise_hip_instance_eval left on the
// device (maxDets 1 / 10 / 100, the four area ranges, the ten IoU thresholds, the caller's recall thresholds).  Host restatement, which the
// result equals byte for byte: odise_amd/instance_eval.py accumulate.
//
//   1. slots    every slot of every block gets a record (its rows, its clamped count, its image number); the slots are sorted by image
//               number (radix_sort.h; stable, so slots of one image number keep their arrival order).
//   2. rows     a wave per slot, in that order: the rank of a row among the rows of its category in the slot (the host code's `rank`, which
//               maxDets cuts), the sort key category << 32 | score key, and two words per row: bits 0..39 = matched & ~ignored (a true
//               positive of cell 10 a + t), bits 40..42 = rank < 1 / 10 / 100, and ~matched & ~ignored (a false positive).  Rows that
//               do not exist, and rows that raise a flag, take the category K and sort behind everything.
//               score key: the bits of the score with -0 folded onto +0, mapped so that unsigned order is float order, inverted: ascending
//               keys are descending scores, +inf first, equal scores (and only those) equal keys.
//   3. sort     by (category, score key), stable: behind it a category's rows are in descending score, ties by image number, then by
//               arrival - the order of the host's stable sort on `image` followed by argsort(-score, kind="mergesort").
//   4. permute  the two words of every row into sorted order.
//   5. cells    a block per (category k, range a, maxDet m), a wave per threshold t.  The wave counts the true and false positives of its
//               cell over the category's rows, then walks the rows from the right, 64 at a time: the inclusive counts of a row are the totals
//               minus what lies to its right (two ballots), pr = tp / (fp + tp + 2^-52) in double, the running maximum comes from a shuffle
//               scan plus the carry of the chunks already walked.  The recall thresholds are turned once per block into counts: c[r] = the
//               smallest tp with tp / npig >= rec_thrs[r] (by the same double division), at least 1.  The row that holds the e-th true
//               positive writes precision[t, r, k, a, m] for every r with c[r] == e; cells with c[r] beyond the total are 0.  Rows past a
//               maxDet cut carry the counts of the row before them, so they never raise the maximum.
//
// odise_hip_lvis_accumulate (LVISEval.accumulate; host restatement odise_amd/lvis_eval.py accumulate) is the same five steps with up to 300
// rows per slot (five rows per lane in step 2) and ONE cut, which the rows of odise_hip_lvis_eval already respect: every row is selected
// (bit 40), there is no rank, and the outputs have no maxDets axis.
//
// Counts are integers and the maximum is exact: the same bytes from run to run.  No fast-math, no contraction: the divisions are IEEE.
#include <algorithm>

#include "radix_sort.h"

#pragma clang fp contract(off)

namespace odise {

constexpr int kAccumMaxTopk = 100, kLvisAccumMaxTopk = 300, kAccumMaxRec = 101, kAccumMaxK = 65535;
constexpr int64_t kAccumMaxRows = 1 << 24;
constexpr int kAccumT = 10, kAccumA = 4, kAccumM = 3;
constexpr int kAccumChunkBlocks = 32;      // blocks of rows described by value in one launch of the slot kernel
constexpr unsigned long long kCellMask = (1ull << 40) - 1ull;

typedef unsigned long long u64;

struct AccumBlocks {
    const odise_inst_eval_row* rows[kAccumChunkBlocks];
    const int32_t* counts[kAccumChunkBlocks];
    int first[kAccumChunkBlocks + 1];      // first slot of block i of this launch, counted from the launch's first slot
    int n, slot0;                          // blocks in this launch; the launch's first slot among all slots
};

// ---- 1. slots -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) accum_slots_kernel(AccumBlocks B, int topk, const odise_inst_eval_row** __restrict__ slot_rows,
                                                         int* __restrict__ slot_n, sort_key* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= B.first[B.n]) return;
    int b = 0;
    while (b + 1 < B.n && s >= B.first[b + 1]) ++b;
    const int local = s - B.first[b];
    const odise_inst_eval_row* rows = B.rows[b] + (int64_t)local * topk;
    const int n = min(max(B.counts[b][local], 0), topk);
    const int g = B.slot0 + s;
    slot_rows[g] = rows;
    slot_n[g] = n;
    keys[g] = n > 0 ? (sort_key)((uint32_t)rows[0].image ^ 0x80000000u) : 0ull;   // signed order
    vals[g] = (uint32_t)g;
}

// ---- 2. rows ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t score_key(float s) {
    uint32_t u = s == 0.f ? 0u : __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

// kPer: the rows of a slot that a lane takes (64 kPer >= topk); kOneCut: no maxDets cuts, every row is selected (bit 40)
template <int kPer, bool kOneCut>
__global__ void __launch_bounds__(256) accum_rows_kernel(const uint32_t* __restrict__ order, const odise_inst_eval_row* const* __restrict__ slot_rows,
                                                        const int* __restrict__ slot_n, int n_slots, int topk, int K,
                                                        sort_key* __restrict__ keys, uint32_t* __restrict__ vals, u64* __restrict__ tpw,
                                                        u64* __restrict__ fpw, int* __restrict__ status, int* __restrict__ flags) {
    __shared__ int cats[4][64 * kPer];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wave;                       // position of the slot in image order
    const bool live = r < n_slots;
    const int slot = live ? (int)order[r] : 0;
    const odise_inst_eval_row* rows = live ? slot_rows[slot] : nullptr;
    const int n = live ? slot_n[slot] : 0;
    odise_inst_eval_row row[kPer];
    int f = 0;
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
        const int i = lane + 64 * h;
        int cat = K;
        if (i < n) {
            row[h] = rows[i];
            cat = row[h].category;
            if ((unsigned)cat >= (unsigned)K) { f |= 1; cat = K; }
            if (row[h].score != row[h].score) { f |= 2; cat = K; }
        }
        cats[wave][i] = cat;
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int h = 0; h < kPer; ++h) {
        const int i = lane + 64 * h;
        if (i >= topk) continue;
        const int64_t o = (int64_t)r * topk + i;
        const int cat = cats[wave][i];
        u64 tw = 0ull, fw = 0ull;
        sort_key key = ((sort_key)(uint32_t)K << 32) | 0xFFFFFFFFull;
        if (cat < K) {                                         // an existing row without a flag
            u64 sel = 1ull;
            if constexpr (!kOneCut) {
                int rank = 0;
                for (int j = 0; j < n; ++j) rank += (j < i && cats[wave][j] == cat) ? 1 : 0;
                sel = (rank < 1 ? 1ull : 0ull) | (rank < 10 ? 2ull : 0ull) | (rank < 100 ? 4ull : 0ull);
            }
            tw = (row[h].matched & ~row[h].ignored & kCellMask) | (sel << 40);
            fw = ~row[h].matched & ~row[h].ignored & kCellMask;
            key = ((sort_key)(uint32_t)cat << 32) | score_key(row[h].score);
        }
        keys[o] = key;
        vals[o] = (uint32_t)o;
        tpw[o] = tw;
        fpw[o] = fw;
    }
    if (f) {
        atomicOr(status, f);
        atomicOr(flags, f);
    }
}

// ---- 4. permute ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) accum_permute_kernel(const uint32_t* __restrict__ vals, const u64* __restrict__ tpw, const u64* __restrict__ fpw,
                                                           int n, u64* __restrict__ tps, u64* __restrict__ fps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = vals[i];
    tps[i] = tpw[v];
    fps[i] = fpw[v];
}

// ---- 5. cells -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int first_of_category(const sort_key* keys, int n, uint32_t cat) {   // the first row whose category is >= cat
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(keys[mid] >> 32) >= cat) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// kM: the maxDets cuts, the last axis of both outputs (3: bits 40..42 of a row's first word; 1: bit 40, which every row carries)
template <int kM>
__global__ void __launch_bounds__(64 * kAccumT) accum_cells_kernel(const sort_key* __restrict__ keys, const u64* __restrict__ tps,
                                                                  const u64* __restrict__ fps, int n_rows, int K, int R,
                                                                  const long long* __restrict__ npig, const double* __restrict__ rec_thrs,
                                                                  const int* __restrict__ status, double* __restrict__ precision,
                                                                  double* __restrict__ recall) {
    __shared__ int c[kAccumMaxRec];      // the true positives that reach recall threshold r, at least 1
    __shared__ int seg[2];
    const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6;
    const int k = blockIdx.x, a = blockIdx.y / kM, m = blockIdx.y - a * kM;
    const long long np = npig[(int64_t)k * kAccumA + a];
    const int64_t pstride = (int64_t)K * (kAccumA * kM);                                        // between r and r + 1
    double* prec = precision + (int64_t)t * R * pstride + (int64_t)k * (kAccumA * kM) + a * kM + m;
    double* rec = recall + ((int64_t)t * K + k) * (kAccumA * kM) + a * kM + m;
    if (status[0] != 0 || np <= 0) {     // no non-ignored ground truth in (k, a), or the call raised a flag
        for (int r = lane; r < R; r += 64) prec[r * pstride] = -1.0;
        if (lane == 0) rec[0] = -1.0;
        return;
    }
    if (tid < 2) seg[tid] = first_of_category(keys, n_rows, (uint32_t)(k + tid));
    __syncthreads();
    const int lo = seg[0], n = seg[1] - seg[0];
    const double dnp = (double)np;
    if (tid < R) {
        const double thr = rec_thrs[tid], g0 = ceil(thr * dnp);
        long long g = !(g0 > 0.0) ? 0ll : (g0 > (double)(n + 1) ? (long long)(n + 1) : (long long)g0);
        while (g > 0 && (double)(g - 1) / dnp >= thr) --g;
        while (g <= n && (double)g / dnp < thr) ++g;
        c[tid] = (int)max(g, 1ll);
    }
    __syncthreads();

    const int q = 10 * a + t, sel_bit = 40 + m;
    const int chunks = (n + 63) >> 6;
    int tp_tot = 0, fp_tot = 0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int i = ch * 64 + lane;
        if (i < n) {
            const u64 tw = tps[lo + i], fw = fps[lo + i];
            const int sel = (int)(tw >> sel_bit) & 1;
            tp_tot += sel & (int)(tw >> q);
            fp_tot += sel & (int)(fw >> q);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        tp_tot += __shfl_xor(tp_tot, o);
        fp_tot += __shfl_xor(fp_tot, o);
    }
    if (lane == 0) rec[0] = (double)tp_tot / dnp;
    for (int r = lane; r < R; r += 64)
        if (c[r] > tp_tot) prec[r * pstride] = 0.0;

    const u64 above = lane == 63 ? 0ull : (~0ull << (lane + 1));
    const double eps = 2.220446049250313e-16;   // 2^-52: np.spacing(1)
    int tp_right = 0, fp_right = 0;
    double run = 0.0;                           // the maximum of pr over the chunks already walked; pr is never negative
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int i = ch * 64 + lane;
        const bool valid = i < n;
        const u64 tw = valid ? tps[lo + i] : 0ull, fw = valid ? fps[lo + i] : 0ull;
        const int sel = (int)(tw >> sel_bit) & 1;
        const bool tb = sel & (int)(tw >> q), fb = sel & (int)(fw >> q);
        const u64 mt = __ballot(tb), mf = __ballot(fb);
        const int tp = tp_tot - tp_right - __popcll(mt & above), fp = fp_tot - fp_right - __popcll(mf & above);
        double s = valid ? (double)tp / ((double)fp + (double)tp + eps) : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_down(s, o);
            if (lane + o < 64) s = fmax(s, v);
        }
        s = fmax(s, run);
        if (tb) {                               // the tp-th true positive: every recall threshold it is the first to reach
            int r0 = 0, r1 = R;
            while (r0 < r1) {
                const int mid = (r0 + r1) >> 1;
                if (c[mid] >= tp) r1 = mid;
                else r0 = mid + 1;
            }
            for (int r = r0; r < R && c[r] == tp; ++r) prec[r * pstride] = s;
        }
        run = __shfl(s, 0);
        tp_right += __popcll(mt);
        fp_right += __popcll(mf);
    }
}

}  // namespace odise

using namespace odise;

extern "C" int odise_hip_sizeof_inst_accum_desc(void) { return (int)sizeof(odise_inst_accum_desc); }

// COCOeval.accumulate (odise_inst_accum_desc: maxDets 1 / 10 / 100, topk <= 100) or LVISEval.accumulate (odise_lvis_accum_desc: one cut,
// topk <= 300) of a descriptor; the two have the same members
template <class Desc, int kMaxTopk, int kM>
static int accum_run(odise_hip_ctx* ctx, const Desc* d, const char* what) {
    ODISE_REQUIRE(ctx && d, "%s: null argument", what);
    ODISE_REQUIRE(d->npig && d->rec_thrs && d->precision && d->recall && d->flags, "%s: null pointer", what);
    ODISE_REQUIRE(d->topk >= 1 && d->topk <= kMaxTopk, "%s: topk %d (1..%d)", what, d->topk, kMaxTopk);
    ODISE_REQUIRE(d->num_categories >= 1 && d->num_categories <= kAccumMaxK, "%s: num_categories %d (1..%d)", what, d->num_categories,
                  kAccumMaxK);
    ODISE_REQUIRE(d->n_rec >= 1 && d->n_rec <= kAccumMaxRec, "%s: %d recall thresholds (1..%d)", what, d->n_rec, kAccumMaxRec);
    ODISE_REQUIRE(d->n_blocks >= 0 && (d->n_blocks == 0 || (d->rows && d->counts && d->slots)), "%s: %d blocks, null block table", what,
                  d->n_blocks);
    int64_t n_slots = 0;
    for (int b = 0; b < d->n_blocks; ++b) {
        ODISE_REQUIRE(d->slots[b] >= 0 && (d->slots[b] == 0 || (d->rows[b] && d->counts[b])), "%s: block %d: %d slots, null pointer", what, b,
                      d->slots[b]);
        n_slots += d->slots[b];
        ODISE_REQUIRE(n_slots * d->topk <= kAccumMaxRows, "%s: more than %lld rows", what, (long long)kAccumMaxRows);
    }
    ODISE_CHECK_HIP(hipSetDevice(ctx->device));
    const int K = d->num_categories, R = d->n_rec, topk = d->topk, S = (int)n_slots;
    const int N = S * topk;
    // scratch: status | slot records | the two sorts' buffers (the slot sort's lie inside the row sort's) | the words of the rows, twice
    const size_t n8 = (size_t)round_up((int64_t)N * 8, 256), n4 = (size_t)round_up((int64_t)N * 4, 256), s8 = (size_t)round_up((int64_t)S * 8, 256),
                 s4 = (size_t)round_up((int64_t)S * 4, 256), hb = (size_t)round_up((int64_t)std::max(sort_hist_bytes(N), sort_hist_bytes(S)), 256);
    ODISE_TRY(scratch_reserve(ctx->rle, 256 + 2 * s8 + 2 * s4 + s8 + s4 + 6 * n8 + 2 * n4 + hb, 8, drain_streams(ctx->stream), "rle"));
    char* p = (char*)ctx->rle.ptr;
    int* status = (int*)p; p += 256;
    SortBufs ss, rs;
    ss.keys[0] = (sort_key*)p; p += s8;
    ss.keys[1] = (sort_key*)p; p += s8;
    ss.vals[0] = (uint32_t*)p; p += s4;
    ss.vals[1] = (uint32_t*)p; p += s4;
    const odise_inst_eval_row** slot_rows = (const odise_inst_eval_row**)p; p += s8;
    int* slot_n = (int*)p; p += s4;
    rs.keys[0] = (sort_key*)p; p += n8;
    rs.keys[1] = (sort_key*)p; p += n8;
    u64* tpw = (u64*)p; p += n8;
    u64* fpw = (u64*)p; p += n8;
    u64* tps = (u64*)p; p += n8;
    u64* fps = (u64*)p; p += n8;
    rs.vals[0] = (uint32_t*)p; p += n4;
    rs.vals[1] = (uint32_t*)p; p += n4;
    ss.hist = rs.hist = (uint32_t*)p;
    ODISE_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), ctx->stream));
    int side = 0;
    if (N > 0) {
        AccumBlocks B;
        B.n = 0; B.slot0 = 0; B.first[0] = 0;
        int done = 0;   // slots described by earlier launches
        for (int b = 0; b <= d->n_blocks; ++b) {
            if (b < d->n_blocks && d->slots[b] > 0) {
                B.rows[B.n] = d->rows[b];
                B.counts[B.n] = d->counts[b];
                B.first[B.n + 1] = B.first[B.n] + d->slots[b];
                ++B.n;
            }
            if (B.n == kAccumChunkBlocks || (b == d->n_blocks && B.n > 0)) {
                const int here = B.first[B.n];
                B.slot0 = done;
                hipLaunchKernelGGL(accum_slots_kernel, dim3((unsigned)ceil_div(here, 256)), dim3(256), 0, ctx->stream, B, topk, slot_rows, slot_n,
                                   ss.keys[0], ss.vals[0]);
                ODISE_CHECK_HIP(hipGetLastError());
                done += here;
                B.n = 0;
            }
        }
        ODISE_TRY(radix_sort_pairs(ctx->stream, ss, S, 32, &side));
        hipLaunchKernelGGL((accum_rows_kernel<(kMaxTopk + 63) / 64, kM == 1>), dim3((unsigned)ceil_div(S, 4)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)ss.vals[side],
                           (const odise_inst_eval_row* const*)slot_rows, (const int*)slot_n, S, topk, K, rs.keys[0], rs.vals[0], tpw, fpw, status,
                           (int*)d->flags);
        ODISE_CHECK_HIP(hipGetLastError());
        int cat_bits = 1;
        while ((K >> cat_bits) != 0) ++cat_bits;   // the category K of the rows that do not count still fits
        ODISE_TRY(radix_sort_pairs(ctx->stream, rs, N, 32 + cat_bits, &side));
        hipLaunchKernelGGL(accum_permute_kernel, dim3((unsigned)ceil_div(N, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)rs.vals[side],
                           (const u64*)tpw, (const u64*)fpw, N, tps, fps);
        ODISE_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(accum_cells_kernel<kM>, dim3((unsigned)K, kAccumA * kM), dim3(64 * kAccumT), 0, ctx->stream, (const sort_key*)rs.keys[side],
                       (const u64*)tps, (const u64*)fps, N, K, R, (const long long*)d->npig, d->rec_thrs, (const int*)status, d->precision, d->recall);
    ODISE_CHECK_HIP(hipGetLastError());
    return ODISE_OK;
}

extern "C" int odise_hip_instance_accumulate(odise_hip_ctx* ctx, const odise_inst_accum_desc* d) {
    return accum_run<odise_inst_accum_desc, kAccumMaxTopk, kAccumM>(ctx, d, "instance_accumulate");
}

extern "C" int odise_hip_lvis_accumulate(odise_hip_ctx* ctx, const odise_lvis_accum_desc* d) {
    return accum_run<odise_lvis_accum_desc, kLvisAccumMaxTopk, 1>(ctx, d, "lvis_accumulate");
}
