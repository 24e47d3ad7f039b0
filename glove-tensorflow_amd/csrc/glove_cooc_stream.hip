// Co-occurrence counting of a corpus of any length on gfx950 (include/glove_cooc_stream_hip.h, libglove_prep_hip.so).
//
// glove_cooc.hip counts a whole corpus in one call: 52 B of workspace per key slot, 2 context n slots.  Here the corpus
// arrives in chunks.  A chunk's keys are made, sorted and run-length encoded as there (glove_cooc_keys.h holds the keys and
// the workspace of both); the running state is one sorted table of (key, int64 count); a merge-path merge folds every chunk
// into it; the (row, col, count, value) table is made from the state at the end, by the expression and in the order of
// cooc_aggregate.  The state holds integers only, so the result is bit for bit that of the one-shot call however the corpus
// was cut.  The merge and the finalisation are glove_table_ops.hip's: the vocabulary merge of glove_text.hip and the weighted
// finalisation of glove_cooc_options.hip run the same kernels.
#include "glove_common.h"
#include "glove_cooc_keys.h"
#include "glove_table_ops.h"
#include "../../include/glove_cooc_stream_hip.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

namespace glove {

// ---- chunk keys ------------------------------------------------------------------------------------------------------
// the slots of the chunk's own positions; partners may lie in the halo
__global__ void chunk_emit_keys(const int32_t *__restrict__ tok, int64_t n_own, int64_t n_total, int32_t V, int32_t context,
                                uint64_t *__restrict__ keys)
{
    emit_slot_keys(tok, n_own, n_total, V, context, keys);
}

// the run-length encoded keys without the sentinel run, counts widened to int64, cut at cap
__global__ void chunk_copy_out(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ ucounts,
                               const int64_t *__restrict__ n_unique, uint64_t *__restrict__ keys_out,
                               int64_t *__restrict__ counts_out, int64_t *__restrict__ n_out, int64_t cap)
{
    copy_out_runs(ukeys, ucounts, n_unique, keys_out, counts_out, n_out, cap);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_cooc_stream_abi_version(void) { return GLOVE_COOC_STREAM_ABI_VERSION; }

size_t glove_cooc_chunk_workspace_bytes(int64_t n_total, int32_t context)
{
    if (n_total < 0 || context <= 0 || context > 255) return 0;
    if ((double)n_total * context * 2 > 4294967295.0) return 0;
    return carve_cooc_sort_ws(nullptr, n_total, context).bytes;
}

int glove_cooc_chunk_keys_i32(const int32_t *tokens, int64_t n_own, int64_t n_total, int32_t V, int32_t context,
                              uint64_t *keys_out, int64_t *counts_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes,
                              void *stream)
{
    if (n_own < 0 || n_total < n_own || bad_key_shape(V, context) || cap < 0 || !n_out || !ws) return GLOVE_E_BADARG;
    if ((double)n_total * context * 2 > 4294967295.0) return GLOVE_E_BADARG;      // the one-chunk slot limit
    hipStream_t st = (hipStream_t)stream;
    if (n_own == 0) {
        HIP_TRY(zero_words(n_out, 2, st));
        return 0;
    }
    if (!tokens || (cap > 0 && (!keys_out || !counts_out))) return GLOVE_E_BADARG;
    const CoocSortWs w = carve_cooc_sort_ws(ws, n_total, context);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const size_t slots = (size_t)n_own * context * 2;
    // all 64 bits: the sentinel (all ones) must sort behind every real key
    size_t need_sort = 0, need_rle = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, need_sort, w.keys, w.keys_sorted, slots, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(nullptr, need_rle, w.keys_sorted, (unsigned int)slots, w.ukeys, w.ucounts,
                                       w.n_unique, st));
    if (need_sort > w.prim_bytes || need_rle > w.prim_bytes) return GLOVE_E_WORKSPACE;
    hipLaunchKernelGGL(chunk_emit_keys, dim3(blocks_for(n_own * context, kBlock)), dim3(kBlock), 0, st, tokens, n_own, n_total,
                       V, context, w.keys);
    HIP_TRY(rocprim::radix_sort_keys(w.prim, need_sort, w.keys, w.keys_sorted, slots, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(w.prim, need_rle, w.keys_sorted, (unsigned int)slots, w.ukeys, w.ucounts,
                                       w.n_unique, st));
    // n_unique lives on the device: the copy is sized by the worst case and reads it
    hipLaunchKernelGGL(chunk_copy_out, dim3(blocks_for((int64_t)slots, kBlock)), dim3(kBlock), 0, st, w.ukeys, w.ucounts,
                       w.n_unique, keys_out, counts_out, n_out, cap);
    return (int)hipGetLastError();
}

size_t glove_cooc_merge_workspace_bytes(int64_t cap_a, int64_t cap_b) { return merge_workspace_bytes(cap_a, cap_b); }

int glove_cooc_merge_u64(const uint64_t *keys_a, const int64_t *counts_a, const int64_t *n_a, int64_t cap_a,
                         const uint64_t *keys_b, const int64_t *counts_b, const int64_t *n_b, int64_t cap_b,
                         uint64_t *keys_out, int64_t *counts_out, int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes,
                         void *stream)
{
    const MergeIn a = {keys_a, {counts_a, nullptr}, n_a, cap_a}, b = {keys_b, {counts_b, nullptr}, n_b, cap_b};
    const MergeOut out = {keys_out, {counts_out, nullptr}, n_out, cap_out};
    return merge_tables(a, b, out, 1, ws, ws_bytes, (hipStream_t)stream);
}

size_t glove_cooc_finalize_workspace_bytes(int64_t cap_keys) { return finalize_workspace_bytes(cap_keys); }

int glove_cooc_finalize(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                        int32_t context, int64_t min_count, int32_t *out_row, int32_t *out_col, int64_t *out_count,
                        double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws, size_t ws_bytes, void *stream)
{
    return finalize_table(keys, counts, n, cap_keys, V, context, min_count, kWindowHarmonic, out_row, out_col, out_count,
                          out_value, out_nnz, cap_out, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
