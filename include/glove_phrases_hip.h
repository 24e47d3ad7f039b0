/*
 * glove_phrases_hip.h — C ABI of libglove_prep_hip.so, fifth header: phrase detection (word2phrase) on the MI355X (gfx950).
 * A corpus is rewritten in place, block by block: some single-space bytes between two tokens become a delimiter byte, as
 * word2phrase decides them, so that "new york" reaches the tokenizer of glove_text_hip.h as the one token "new_york".  The
 * entry points below count a block's adjacent id pairs, choose the accepted pairs from the merged counts, and join a block.
 * The other headers stay as they are and keep their versions; these entry points are versioned by GLOVE_PHRASES_ABI_VERSION.
 *
 * Conventions (those of glove_text_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, keeps no global state and
 *     never synchronizes; its own kernels clear their counters themselves (rocPRIM's radix sort, which sorts a block's
 *     keys, zeroes its digit histograms with hipMemsetAsync once a block holds too many for its merge sort);
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known capacities, never from counts the device computed; no kernel waits
 *     for another workgroup;
 *   - sizes the device computed (n_tokens, n, n_out, n_phrases) are int64 in device memory; a size written by a call is the
 *     TRUE size even where it exceeds the capacity, and entries at or beyond the capacity are not written;
 *   - integer arithmetic only, except the score; counters are integer atomics: no result depends on the grid, the tile or
 *     the order in which workgroups run.
 *
 * Semantics.  Tokens, separator bytes and ids are those of glove_text_hip.h: token t of a block is bytes[start[t] ..
 * start[t] + len[t]), ids[t] > 0 numbers a kept word, every other token has id 0 (a negative id counts as 0).
 *   plain pair   (t, t + 1) is PLAIN iff start[t + 1] == start[t] + len[t] + 1 and the byte between the two tokens,
 *                bytes[start[t] + len[t]], is 0x20: a longer separator run, a newline, a tab or a multi-byte separator
 *                breaks a phrase (word2phrase breaks at </s>);
 *   bigram key   ((uint64)ids[t] << 32) | (uint32)ids[t + 1], for plain pairs with both ids > 0; n_ab = how often it occurs;
 *   score        in IEEE double, in this order, every operation rounded once:
 *                    score = (double)(n_ab - min_count) / (double)n_a / (double)n_b * (double)N
 *                n_a = unigram[ids[t]], n_b = unigram[ids[t + 1]], N = total_tokens.  A bigram is ACCEPTED iff
 *                n_ab >= min_count and score > threshold (strictly);
 *   greedy join  cand[t] = pair (t, t + 1) is plain and its key is accepted; chosen[t] = cand[t] && !chosen[t - 1]: after
 *                a join the next pair is not scored (word2phrase's pa = 0).  Equivalently chosen[t] = cand[t] && (t - b(t))
 *                odd, b(t) = the last non-candidate index < t: of a run of candidates the 1st, 3rd, 5th ... are chosen;
 *   output       byte start[t] + len[t] becomes the delimiter for every chosen t.  No other byte changes.
 */
#ifndef GLOVE_PHRASES_HIP_H
#define GLOVE_PHRASES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_PHRASES_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size or option out of range / an output aliases an input */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* Tokens of a block one workgroup of glove_phrase_join_u8 owns (a tile): four rounds of 256 lanes. */
#define GLOVE_PHRASE_TILE 1024
/* Keys of a table one workgroup of glove_phrase_select owns: 256 lanes x 4 keys. */
#define GLOVE_PHRASE_SELECT_TILE 1024

int glove_phrases_abi_version(void);

/* ---- a block's adjacent pairs -> its bigram table --------------------------------------------------------------------
 * Workspace of glove_phrase_bigram_keys_i32 (pure host function; 0 for cap_tokens < 0 or cap_tokens > 2^31 - 1): for
 * n = max(1, cap_tokens), pieces rounded up to 256 B each:
 *     uint64 keys[n] | uint64 sorted keys[n] | uint32 run lengths[n] | int64 counter[32] | rocPRIM scratch[16 MiB + 16 n] */
size_t glove_phrase_bigram_workspace_bytes(int64_t cap_tokens);

/* (start, len, ids)[0 .. min(*n_tokens, cap_tokens)) as glove_text_tokenize_u8 and glove_text_token_ids_i32 wrote them for
 * bytes[0 .. n_bytes).  Output: the distinct bigram keys of ALL adjacent pairs of the block, ascending, and how often each
 * occurs.  *n_out = their number (true size; only the first `cap` are written).  Tables of different blocks are merged
 * with glove_cooc_merge_u64.
 * One kernel writes a key (or all-ones) per pair; rocPRIM sorts and run-length encodes, as in glove_cooc_chunk_keys_i32. */
int glove_phrase_bigram_keys_i32(const uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len,
                                 const int32_t *ids, const int64_t *n_tokens, int64_t cap_tokens, uint64_t *keys_out,
                                 int64_t *counts_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes, void *stream);

/* ---- the merged bigram table -> the accepted phrases -----------------------------------------------------------------
 * Workspace of glove_phrase_select (pure host function; 0 for cap_keys < 0 or cap_keys > 2^40): with
 * tiles = max(1, ceil(cap_keys / GLOVE_PHRASE_SELECT_TILE)), int64 pieces, each rounded up to 256 B:
 *     count[tiles] | offset[tiles] | scan scratch[64 KiB + 8 tiles] */
size_t glove_phrase_select_workspace_bytes(int64_t cap_keys);

/* (keys, counts)[0 .. min(*n, cap_keys)), keys ascending; unigram[0 .. V) the counts of the ids (V >= 1; a key with an id
 * outside [1, V) or a unigram count < 1 is not accepted); total_tokens >= 0, min_count >= 1, threshold finite and > 0.
 * Output: the accepted keys, ascending, their counts and their scores.  *n_out = their number (true size; only the first
 * cap_out are written).  No output may overlap an input or another output.
 * A count pass over tiles, rocPRIM's scan of the tile counts, a write pass. */
int glove_phrase_select(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys,
                        const int64_t *unigram, int32_t V, int64_t total_tokens, int64_t min_count, double threshold,
                        uint64_t *keys_out, int64_t *counts_out, double *score_out, int64_t *n_out, int64_t cap_out,
                        void *ws, size_t ws_bytes, void *stream);

/* ---- a block and the accepted phrases -> the joined block ------------------------------------------------------------
 * Workspace of glove_phrase_join_u8 (pure host function; 0 for cap_tokens < 0 or cap_tokens > 2^31 - 1): with
 * n = max(1, cap_tokens) and tiles = ceil(n / GLOVE_PHRASE_TILE), pieces rounded up to 256 B each:
 *     int32 slot[n] | int32 carry in[64] | int64 last[tiles] | int64 scanned[tiles] | scan scratch[64 KiB + 8 tiles] */
size_t glove_phrase_join_workspace_bytes(int64_t cap_tokens);

/* bytes[0 .. n_bytes) is rewritten IN PLACE: byte start[t] + len[t] becomes `delimiter` for every chosen t (above).
 * phrase_keys[0 .. min(*n_phrases, cap_phrases)) are the accepted keys, ascending.  delimiter: one byte in 0 .. 127 that is
 * no separator byte.  carry: one int32, read as chosen[-1] of the block (0 or not 0) and written as chosen[n - 2], so it
 * goes from block to block; a block of fewer than two tokens leaves it as it was.  joined[j] += how often accepted key j
 * was chosen (int64 [cap_phrases]; the caller zeroes it once per file); *n_joined = the block's joins.
 * Three passes over tiles of GLOVE_PHRASE_TILE tokens: one searches every plain pair's key in the accepted table, keeps
 * the slot it found and each tile's last non-candidate index; rocPRIM max-scans the tiles' values; the last one makes
 * b(t) inside the tile from the scanned value and a wave / LDS max-scan, stores the delimiters and counts the joins. */
int glove_phrase_join_u8(uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len, const int32_t *ids,
                         const int64_t *n_tokens, int64_t cap_tokens, const uint64_t *phrase_keys, const int64_t *n_phrases,
                         int64_t cap_phrases, int32_t delimiter, int32_t *carry, int64_t *joined, int64_t *n_joined,
                         void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_PHRASES_HIP_H */
