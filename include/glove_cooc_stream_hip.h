/*
 * glove_cooc_stream_hip.h — C ABI of libglove_prep_hip.so: windowed co-occurrence counting of a corpus of any length on
 * the MI355X (gfx950).  The corpus is counted chunk by chunk; the running state is ONE sorted table of
 * (row, col, distance) keys with integer counts on the device; every chunk's table is folded into it by a merge-path
 * merge; the (row, col, count, value) table is made from the state at the end.  The state holds integers only, so the
 * result does not depend on where the corpus was cut: it is bit for bit what glove_cooccurrence_i32 (glove_hip.h)
 * returns for the whole corpus in one call, `value` included.  glove_hip.h and the three glove_eval_*_hip.h headers stay
 * as they are and keep their own versions; the entry points below are versioned by GLOVE_COOC_STREAM_ABI_VERSION.
 *
 * Conventions (as the other headers):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, keeps no global state and
 *     never synchronizes; its own kernels clear nothing with memset nodes (rocPRIM's radix sort, which sorts a chunk's
 *     keys, zeroes its digit histograms with hipMemsetAsync once a chunk is too long for its merge sort);
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known capacities, never from counts the device computed;
 *   - sizes the device computed (n_out, n_a, n_b, n, out_nnz) are int64 in device memory; a size written by a call is
 *     the TRUE size even where it exceeds the capacity, and entries at or beyond the capacity are not written.
 *
 * Keys (those of csrc/glove_cooc.hip): a pair of tokens a != b at distance k in 1 .. context is the uint64
 *     ((a V + b) context + (k - 1)),
 * and BOTH orientations (a, b) and (b, a) are counted for every position pair.  All-ones never appears as a key.
 * Limits of every call that takes them: V >= 1, 1 <= context <= 255, V V context < 9e18 (a key fits 63 bits).
 */
#ifndef GLOVE_COOC_STREAM_HIP_H
#define GLOVE_COOC_STREAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_COOC_STREAM_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / an output aliases an input */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* Positions of the merged order one workgroup of the merge owns (a tile). */
#define GLOVE_COOC_MERGE_TILE 2048

int glove_cooc_stream_abi_version(void);

/* ---- one chunk -> its sorted distinct keys ---------------------------------------------------------------------------
 * Workspace of glove_cooc_chunk_keys_i32 for a chunk of n_total tokens (own + halo): a pure host function, 0 for sizes
 * the call would refuse (n_total < 0, context outside 1 .. 255, more than 2^32 - 1 key slots = 2 context n_total).  It is
 * laid out like glove_cooc_workspace_bytes(n_total, context) of glove_hip.h and costs the same: a chunk takes what a
 * one-shot call on as many tokens takes. */
size_t glove_cooc_chunk_workspace_bytes(int64_t n_total, int32_t context);

/* tokens[0 .. n_total): positions p < n_own are this chunk's own, the other n_total - n_own >= 0 are its halo (the
 * caller supplies min(context, tokens left in the corpus)).  For every own p and every k in 1 .. context with
 * p + k < n_total and tokens[p] != tokens[p + k] both orientations are emitted: a pair belongs to the chunk that owns its
 * LEFT position, so chunks that tile the corpus count every pair once.
 * Output: the distinct keys ascending in keys_out and how often each occurred in counts_out; *n_out = their number
 * (true size; only the first `cap` are written).  n_own == 0 writes *n_out = 0 and nothing else.
 * Radix sort and run-length encoding are rocPRIM's, as in glove_cooccurrence_i32. */
int glove_cooc_chunk_keys_i32(const int32_t *tokens, int64_t n_own, int64_t n_total, int32_t V, int32_t context,
                              uint64_t *keys_out, int64_t *counts_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes,
                              void *stream);

/* ---- merge -----------------------------------------------------------------------------------------------------------
 * Workspace of glove_cooc_merge_u64 (pure host function; 0 for negative capacities or cap_a + cap_b beyond 2^40):
 * with tiles = max(1, ceil((cap_a + cap_b) / GLOVE_COOC_MERGE_TILE)), int64 pieces, each rounded up to 256 B:
 *     split_a[tiles + 1] | split_b[tiles + 1] | count[tiles] | offset[tiles] | scan scratch[64 KiB + 8 tiles] */
size_t glove_cooc_merge_workspace_bytes(int64_t cap_a, int64_t cap_b);

/* A = (keys_a, counts_a)[0 .. min(*n_a, cap_a)) and B likewise, each STRICTLY ascending.  Output: the ascending union of
 * the keys; the count of a key present in both is the int64 sum of its two counts.  *n_out = the union's size (true
 * size; entries at or beyond cap_out are not written).  keys_out, counts_out and n_out must not overlap any input
 * (checked on the host over the capacities: GLOVE_E_BADARG).
 * A merge-path merge: a tile owns GLOVE_COOC_MERGE_TILE positions of the merged order (ties to A) and finds its start by
 * binary search; a tile boundary never separates an A entry from its equal B entry (the split moves one B entry forward);
 * one pass counts each tile's output entries, rocPRIM scans the tile counts, a second pass writes at the tile's offset.
 * Integer adds only, no atomics: the result does not depend on the grid.  The grid is sized from cap_a + cap_b; tiles
 * beyond the merged length return at once. */
int glove_cooc_merge_u64(const uint64_t *keys_a, const int64_t *counts_a, const int64_t *n_a, int64_t cap_a,
                         const uint64_t *keys_b, const int64_t *counts_b, const int64_t *n_b, int64_t cap_b,
                         uint64_t *keys_out, int64_t *counts_out, int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes,
                         void *stream);

/* ---- state -> (row, col, count, value) -------------------------------------------------------------------------------
 * Workspace of glove_cooc_finalize (pure host function; 0 for a negative cap_keys or one beyond 2^40): the head flags
 * and their running sum, int64[cap_keys] each, and the scan's scratch (1 MiB + cap_keys / 16 bytes). */
size_t glove_cooc_finalize_workspace_bytes(int64_t cap_keys);

/* (keys, counts)[0 .. min(*n, cap_keys)) ascending, as the calls above make them.  For every (a, b) among the keys, with
 * n_k the count of ((a V + b) context + (k - 1)):
 *     count = sum_k n_k,    value = sum_k (double)n_k / (double)k   (k ascending, starting from 0.0),
 * the expression and order of glove_cooccurrence_i32.  Pairs with count >= min_count are written in (a, b) order;
 * *out_nnz = their number (true size; only the first cap_out are written). */
int glove_cooc_finalize(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                        int32_t context, int64_t min_count, int32_t *out_row, int32_t *out_col, int64_t *out_count,
                        double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_COOC_STREAM_HIP_H */
