// record.h — the table of the panoptic record, int32 [h*w | 1 | 3*ODISE_MAX_SEGMENTS] (include/odise_hip.h): behind the ids come n and the
// rows (id, isthing, category).  Its layout is stated here and nowhere else in the kernels.  Writers: classify_ops.hip
// (panoptic_decide_kernel), vis_inst.hip (sem_rank_kernel); readers: vis.hip, pq.hip, track.hip.  `table` points at n.
#pragma once
#include "common.h"

namespace odise {

enum RecordColumn { kRecordIsThing = 1, kRecordCategory = 2 };   // a row's columns behind its id

// rows of the table, whatever the memory holds: inside [0, ODISE_MAX_SEGMENTS]
__device__ __forceinline__ int record_rows(const int* __restrict__ table) {
    const int n = table[0];
    return n < 0 ? 0 : (n > ODISE_MAX_SEGMENTS ? ODISE_MAX_SEGMENTS : n);
}
__device__ __forceinline__ int record_id(const int* __restrict__ table, int i) { return table[1 + 3 * i]; }
__device__ __forceinline__ int record_isthing(const int* __restrict__ table, int i) { return table[2 + 3 * i]; }
__device__ __forceinline__ int record_category(const int* __restrict__ table, int i) { return table[3 + 3 * i]; }

__device__ __forceinline__ void record_set_row(int* table, int i, int id, int isthing, int category) {
    table[1 + 3 * i] = id; table[2 + 3 * i] = isthing; table[3 + 3 * i] = category;
}
// rows m .. cap - 1 = 0, shared among `step` threads of which the caller is number `first`
__device__ __forceinline__ void record_zero_rows(int* table, int m, int cap, int first, int step) {
    for (int i = 3 * m + first; i < 3 * cap; i += step) table[1 + i] = 0;
}

struct RecordKeepId {
    __device__ __forceinline__ int operator()(int, int id) const { return id; }
};
// Whole block, followed by the caller's __syncthreads(): ids[i] = keep(i, id of row i) and, when `second` is given, second[i] = that column.
template <class Keep = RecordKeepId>
__device__ __forceinline__ void record_load(const int* __restrict__ table, int n, int* ids, int* second = nullptr, RecordColumn col = kRecordIsThing,
                                            Keep keep = Keep()) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        ids[i] = keep(i, table[1 + 3 * i]);
        if (second) second[i] = table[1 + col + 3 * i];
    }
}

// the first of ids[0 .. n) that equals `id`, else -1.  What VOID (id 0) or a negative id maps to is the caller's rule.
__device__ __forceinline__ int record_find(const int* ids, int n, int id) {
    for (int r = 0; r < n; ++r)
        if (ids[r] == id) return r;
    return -1;
}

// A lane keeps its last translation, so on smooth maps the translation is a compare.  Starts as {0, what VOID maps to in the kernel}.
struct RecordMemo { int id, value; };
template <class Find>
__device__ __forceinline__ int record_memo(RecordMemo& M, int id, Find find) {
    if (id != M.id) { M.id = id; M.value = find(id); }
    return M.value;
}

}  // namespace odise
