// Windowed co-occurrence counting on gfx950 — the producer of the hot path's input format.
//
// Replaces the 85 M-row pandas self-join of the reference's data prep
// (reference src/data/text8.py:84-108: right-context pairs inside a window, value = sum of 1/distance,
// self pairs dropped, then the union with the swapped table is summed).  Integer / byte work, HBM-bound:
//   1. every (position, offset k <= context) with a != b emits BOTH orientations as one 64-bit key
//      ((a V + b) context + (k-1));
//   2. one LSD radix sort (rocPRIM) over the used key bits;
//   3. run-length encode -> n_k per (a, b, k); runs of one (a, b) are adjacent and at most `context` long;
//   4. per (a, b): count = sum_k n_k, value = sum_k n_k / k (k ascending, fp64), written in (a, b) order.
// count is bit-exact against the reference; value differs from pandas' position-order fp64 sum by rounding
// only (tests: rtol 1e-12).
#include "glove_common.h"
#include "glove_cooc_keys.h"

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace glove {

// the slot layout and the keys are glove_cooc_keys.h's (the chunk counter of libglove_prep_hip.so makes the same ones)
__global__ void cooc_emit_keys(const int32_t *__restrict__ tok, int64_t n, int32_t V, int32_t context,
                               uint64_t *__restrict__ keys)
{
    emit_slot_keys(tok, n, n, V, context, keys);
}

// head[i] = 1 where a new (a, b) starts among the unique (a, b, k) keys (the sentinel run is no head)
__global__ void cooc_mark_heads(const uint64_t *__restrict__ ukeys, const int64_t *__restrict__ n_unique,
                                int32_t context, int64_t *__restrict__ head)
{
    const int64_t m = *n_unique;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = ukeys[i];
        head[i] = (key != kNoKey && (i == 0 || ukeys[i - 1] / context != key / context)) ? 1 : 0;
    }
}

__global__ void cooc_aggregate(const uint64_t *__restrict__ ukeys, const int32_t *__restrict__ ucounts,
                               const int64_t *__restrict__ n_unique, const int64_t *__restrict__ head,
                               const int64_t *__restrict__ head_scan /* exclusive */, int32_t V, int32_t context,
                               int64_t cap, int32_t *__restrict__ out_row, int32_t *__restrict__ out_col,
                               int64_t *__restrict__ out_count, double *__restrict__ out_value,
                               int64_t *__restrict__ out_nnz)
{
    const int64_t m = *n_unique;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        if (!head[i]) continue;
        const uint64_t ab = ukeys[i] / context;
        int64_t cnt = 0;
        double val = 0.0;
        for (int64_t j = i; j < m && j < i + context; ++j) {
            const uint64_t key = ukeys[j];
            if (key == kNoKey || key / context != ab) break;
            const int k = (int)(key % context) + 1;
            cnt += ucounts[j];
            val += (double)ucounts[j] / (double)k;
        }
        const int64_t o = head_scan[i];
        if (o < cap) {
            out_row[o] = (int32_t)(ab / V);
            out_col[o] = (int32_t)(ab % V);
            out_count[o] = cnt;
            out_value[o] = val;
        }
    }
    // total number of (a, b) pairs = scan at the last element + its head flag
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_nnz = m > 0 ? head_scan[m - 1] + head[m - 1] : 0;
}

}  // namespace glove

using namespace glove;

extern "C" {

size_t glove_cooc_workspace_bytes(int64_t n_tokens, int32_t context)
{
    if (n_tokens < 0 || context <= 0) return 0;
    return carve_cooc_sort_ws(nullptr, n_tokens, context).bytes;
}

int glove_cooccurrence_i32(const int32_t *tokens, int64_t n, int32_t V, int32_t context, int32_t *out_row,
                           int32_t *out_col, int64_t *out_count, double *out_value, int64_t *out_nnz, int64_t cap,
                           void *ws, size_t ws_bytes, void *stream)
{
    if (n < 0 || bad_key_shape(V, context) || cap < 0 || !out_nnz || !ws) return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(zero_words(out_nnz, 2, st));
        return 0;
    }
    if (!tokens || !out_row || !out_col || !out_count || !out_value) return GLOVE_E_BADARG;
    const CoocSortWs w = carve_cooc_sort_ws(ws, n, context);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const size_t slots = (size_t)n * context * 2;
    hipLaunchKernelGGL(cooc_emit_keys, dim3(blocks_for(n * context, kBlock)), dim3(kBlock), 0, st, tokens, n, V, context,
                       w.keys);
    // all 64 bits: the sentinel (all ones) must sort behind every real key
    size_t need = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, need, w.keys, w.keys_sorted, slots, 0, 64, st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    HIP_TRY(rocprim::radix_sort_keys(w.prim, need, w.keys, w.keys_sorted, slots, 0, 64, st));
    if (slots > 0xffffffffull) return GLOVE_E_BADARG;
    int32_t *ucounts = (int32_t *)w.ucounts;      // cooc_aggregate reads the run lengths as int32
    HIP_TRY(rocprim::run_length_encode(nullptr, need, w.keys_sorted, (unsigned int)slots, w.ukeys, ucounts,
                                       w.n_unique, st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    HIP_TRY(rocprim::run_length_encode(w.prim, need, w.keys_sorted, (unsigned int)slots, w.ukeys, ucounts,
                                       w.n_unique, st));
    // n_unique lives on the device: size the follow-up launches by the worst case and let them read it
    const int nb = blocks_for((int64_t)slots, kBlock);
    hipLaunchKernelGGL(cooc_mark_heads, dim3(nb), dim3(kBlock), 0, st, w.ukeys, w.n_unique, context, w.head);
    HIP_TRY(rocprim::exclusive_scan(nullptr, need, w.head, w.head_scan, (int64_t)0, slots, rocprim::plus<int64_t>(), st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    // entries past n_unique are stale but never read: cooc_aggregate stops at n_unique
    HIP_TRY(rocprim::exclusive_scan(w.prim, need, w.head, w.head_scan, (int64_t)0, slots, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(cooc_aggregate, dim3(nb), dim3(kBlock), 0, st, w.ukeys, ucounts, w.n_unique, w.head, w.head_scan,
                       V, context, cap, out_row, out_col, out_count, out_value, out_nnz);
    return (int)hipGetLastError();
}

}  // extern "C"
