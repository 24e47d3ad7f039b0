/*
 * glove_cooc_options_hip.h — C ABI of libglove_prep_hip.so: the preprocessing options of the corpus-to-counts stage on
 * the MI355X (gfx950).  Two pieces sit around the calls of glove_cooc_stream_hip.h:
 *   - glove_token_filter_i32 removes tokens from the id stream BEFORE the window is laid ("dirty" subsampling, as word2vec
 *     and hyperwords do it: distances shrink across removed tokens; removing id 0 this way is rare-word deletion);
 *   - glove_cooc_finalize_weighted makes the (row, col, count, value) table from the key table with another distance
 *     weighting than the harmonic one.
 * glove_hip.h and the three other prep headers stay as they are and keep their own versions; the entry points below are
 * versioned by GLOVE_COOC_OPTIONS_ABI_VERSION.
 *
 * Conventions (those of glove_cooc_stream_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, keeps no global state, never
 *     synchronizes and issues no hipMemsetAsync of its own;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known sizes and capacities, never from counts the device computed;
 *   - sizes the device computed (n_out, out_nnz) are int64 in device memory; a size written by a call is the TRUE size
 *     even where it exceeds the capacity, and entries at or beyond the capacity are not written.
 */
#ifndef GLOVE_COOC_OPTIONS_HIP_H
#define GLOVE_COOC_OPTIONS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_COOC_OPTIONS_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / an output aliases an input */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* Tokens one workgroup of the filter owns (a tile). */
#define GLOVE_FILTER_TILE 4096

/* value of a pair from its counts n_k at the distances k = 1 .. context */
#define GLOVE_WINDOW_HARMONIC 0   /* sum_k (double)n_k / (double)k: glove_cooc_finalize, bit for bit */
#define GLOVE_WINDOW_UNIFORM  1   /* (double)count */
#define GLOVE_WINDOW_DYNAMIC  2   /* (double)(sum_k n_k (context - k + 1)) / (double)context */

int glove_cooc_options_abi_version(void);

/* ---- token filter ----------------------------------------------------------------------------------------------------
 * Workspace of glove_token_filter_i32 for a block of n tokens (a pure host function; 0 for n < 0 or n > 2^31 - 1):
 * with tiles = max(1, ceil(n / GLOVE_FILTER_TILE)), int64 pieces, each rounded up to 256 B:
 *     count[tiles] | offset[tiles] | scan scratch[64 KiB + 8 tiles] */
size_t glove_token_filter_workspace_bytes(int64_t n);

/* ids[0 .. n) is a block of a token stream; the token at block index i has the global position p = pos0 + i.  It is KEPT
 * iff
 *     thresholds[ids[i]] == 0xFFFFFFFF   or   u(seed, p) < thresholds[ids[i]],
 * where u is the high half of SplitMix64's finaliser over the position (all arithmetic mod 2^64):
 *     x = p + (seed + 1) * 0x9E3779B97F4A7C15
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9
 *     x ^= x >> 27;  x *= 0x94D049BB133111EB
 *     x ^= x >> 31;  u = x >> 32
 * A threshold of 0 always drops, one of 0xFFFFFFFF always keeps; floor(q 2^32) keeps with probability q.
 * Output: the kept ids in stream order (stable) in ids_out; *n_out = their number (true size; only the first `cap` are
 * written).  The rule uses integers only: the result is a function of (ids, pos0, thresholds, seed) alone, whatever the
 * grid or the tile size, and a token's fate does not depend on where the stream was cut into blocks — the survivors of
 * consecutive blocks, each called with the running pos0, concatenate to the survivors of the whole stream.
 * Limits: 0 <= n <= 2^31 - 1 (n == 0 writes *n_out = 0 and launches nothing else); pos0 >= 0 and pos0 + n <= 2^63 - 1;
 * V >= 1; cap >= 0.  ids_out and n_out must not overlap ids, thresholds or each other (checked on the host over the
 * capacities: GLOVE_E_BADARG).  Ids outside [0, V) are the caller's error (such a token is dropped, never used as an index).
 * One workgroup owns a tile of GLOVE_FILTER_TILE tokens: keep decisions are ranked inside a wave by ballot and popcount,
 * wave totals meet in LDS, one pass counts each tile's survivors, rocPRIM scans the tile counts, a second pass decides
 * again and writes at the tile's offset.  No atomics. */
int glove_token_filter_i32(const int32_t *ids, int64_t n, int64_t pos0, const uint32_t *thresholds /* [V] */, int32_t V,
                           uint64_t seed, int32_t *ids_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes,
                           void *stream);

/* ---- state -> (row, col, count, value), weighted ---------------------------------------------------------------------
 * Workspace of glove_cooc_finalize_weighted (pure host function; 0 for a negative cap_keys or one beyond 2^40): that of
 * glove_cooc_finalize — the head flags and their running sum, int64[cap_keys] each, and the scan's scratch
 * (1 MiB + cap_keys / 16 bytes). */
size_t glove_cooc_finalize_weighted_workspace_bytes(int64_t cap_keys);

/* The contract of glove_cooc_finalize (glove_cooc_stream_hip.h): the same inputs, outputs and (a, b) order, and the
 * min_count rule on `count` (never on `value`).  `value` follows `weighting` (a GLOVE_WINDOW_* constant; anything else is
 * GLOVE_E_BADARG): HARMONIC is glove_cooc_finalize's expression and order, so the output is bit for bit that call's;
 * UNIFORM and DYNAMIC sum in int64 and convert (DYNAMIC: divide) once. */
int glove_cooc_finalize_weighted(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                                 int32_t context, int64_t min_count, int32_t weighting, int32_t *out_row, int32_t *out_col,
                                 int64_t *out_count, double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws,
                                 size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_COOC_OPTIONS_HIP_H */
