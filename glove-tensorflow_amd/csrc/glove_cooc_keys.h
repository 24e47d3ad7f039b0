// What the two co-occurrence counters share: glove_cooccurrence_i32 (glove_cooc.hip, libglove_hip.so) counts a corpus in one
// call, glove_cooc_chunk_keys_i32 (glove_cooc_stream.hip, libglove_prep_hip.so) one chunk of it, and the streamed table is the
// one-shot table bit for bit.  The key of a slot and the workspace of the sort are therefore written once, here.  The two
// objects lie in different libraries: each keeps a __global__ of its own around emit_slot_keys.
#pragma once
#include "glove_common.h"

namespace glove {

constexpr uint64_t kNoKey = ~0ull;      // unused key slots hold the sentinel (sorts last); all-ones never appears as a key

inline bool bad_key_shape(int32_t V, int32_t context)
{
    if (V <= 0 || context <= 0 || context > 255) return true;
    return (double)V * (double)V * (double)context >= 9.0e18;      // key must fit 63 bits
}

// Slot layout: own position p < n_own has 2 * context key slots, offset k = 1 .. context both ways round:
// ((a V + b) context + (k - 1)) and its mirror.  A partner may lie behind the own positions (a chunk's halo) but not behind
// n_total; a slot without a partner, or with a == b, holds the sentinel.  The grid's stride loop over the n_own * context slots.
__device__ inline void emit_slot_keys(const int32_t *__restrict__ tok, int64_t n_own, int64_t n_total, int32_t V, int32_t context,
                                      uint64_t *__restrict__ keys)
{
    const int64_t total = n_own * context;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / context;
        const int k = (int)(i - p * context) + 1;
        uint64_t fwd = kNoKey, bwd = kNoKey;
        if (p + k < n_total) {
            const int64_t a = tok[p], b = tok[p + k];
            if (a != b) {
                fwd = ((uint64_t)a * V + b) * context + (k - 1);
                bwd = ((uint64_t)b * V + a) * context + (k - 1);
            }
        }
        keys[2 * i] = fwd;
        keys[2 * i + 1] = bwd;
    }
}

// The run-length encoded keys of a sorted slot array without the sentinel run, counts widened to int64, cut at cap: what a
// chunk's table (glove_cooc_stream.hip) and a block's bigram table (glove_phrases.hip) are copied out by.  The grid's stride loop.
__device__ inline void copy_out_runs(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ ucounts,
                                     const int64_t *__restrict__ n_unique, uint64_t *__restrict__ keys_out,
                                     int64_t *__restrict__ counts_out, int64_t *__restrict__ n_out, int64_t cap)
{
    int64_t m = *n_unique;
    if (m > 0 && ukeys[m - 1] == kNoKey) --m;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = m;
    if (m > cap) m = cap;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        keys_out[i] = ukeys[i];
        counts_out[i] = (int64_t)ucounts[i];
    }
}

// Workspace of the sort and the run-length encoding of n positions' slots (52 B per slot and the scratch of rocPRIM).
// head and head_scan belong to the one-shot call's aggregation; a chunk leaves them unused, so both calls ask for the same bytes.
struct CoocSortWs {
    uint64_t *keys, *keys_sorted, *ukeys;
    uint32_t *ucounts;
    int64_t *head, *head_scan, *n_unique;
    void *prim;
    size_t prim_bytes, bytes;
};

inline CoocSortWs carve_cooc_sort_ws(void *ws, int64_t n, int32_t context)
{
    CoocSortWs w;
    WsCarver c{(char *)ws};
    const size_t slots = (size_t)(n > 0 ? n : 1) * context * 2;
    w.keys = c.take<uint64_t>(slots);
    w.keys_sorted = c.take<uint64_t>(slots);
    w.ukeys = w.keys;                       // the unsorted keys are dead once sorted
    w.ucounts = c.take<uint32_t>(slots);
    w.head = c.take<int64_t>(slots);
    w.head_scan = c.take<int64_t>(slots);
    w.n_unique = c.take<int64_t>(32);
    w.prim_bytes = (size_t)(16u << 20) + slots * 16;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

}  // namespace glove
