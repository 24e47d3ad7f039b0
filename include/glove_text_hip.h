/*
 * glove_text_hip.h — C ABI of libglove_prep_hip.so, second header: tokenizing and numbering a corpus on the MI355X
 * (gfx950).  A block of the file's raw bytes goes in; out come its whitespace-separated tokens (offset, length, 64-bit
 * hash), the block's vocabulary (distinct hashes with counts and first occurrences), the union of two vocabularies, and,
 * once the host has chosen the kept words, the int32 id of every token.  Bytes are never decoded on the device.
 * glove_cooc_stream_hip.h stays as it is and keeps its own version; the entry points below are versioned by
 * GLOVE_TEXT_ABI_VERSION.
 *
 * Conventions (those of glove_cooc_stream_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, keeps no global state and
 *     never synchronizes; its own kernels clear their counters themselves, with no memset nodes (rocPRIM's radix sort,
 *     which sorts a block's hashes, zeroes its digit histograms with hipMemsetAsync once a block holds too many tokens
 *     for its merge sort);
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known capacities, never from counts the device computed;
 *   - sizes the device computed (n_tokens, n_out, n_a, n_b) are int64 in device memory; a size written by a call is the
 *     TRUE size even where it exceeds the capacity, and entries at or beyond the capacity are not written;
 *   - integer arithmetic only; counters are integer atomics or block partials: no result depends on the grid or on the
 *     order in which workgroups run.
 *
 * Tokens.  Byte i of a block is a SEPARATOR BYTE if b[i] is one of 09 0A 0B 0C 0D 1C 1D 1E 1F 20, or if byte i lies inside
 * an occurrence, within the block, of one of the 19 sequences
 *     C2 85 | C2 A0 | E1 9A 80 | E2 80 80 .. E2 80 8A | E2 80 A8 | E2 80 A9 | E2 80 AF | E2 81 9F | E3 80 80
 * (the UTF-8 encodings of the str.isspace() characters beyond ASCII).  A token is a maximal run of non-separator bytes: on
 * valid UTF-8, exactly the tokens of Python's text.decode().split().
 *
 * Hashes.  64-bit FNV-1a (offset basis 0xcbf29ce484222325, prime 0x100000001b3) over the first
 * min(len, GLOVE_TEXT_MAX_TOKEN) bytes of the token; all-ones is replaced by all-ones - 1, so all-ones never appears.
 */
#ifndef GLOVE_TEXT_HIP_H
#define GLOVE_TEXT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_TEXT_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / an output aliases an input */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* Bytes of a block one workgroup of the tokenizer owns (a tile): 256 lanes x 16 B. */
#define GLOVE_TEXT_TILE_BYTES 4096
/* Bytes of a token the hash covers, and the longest length a `where` word can hold. */
#define GLOVE_TEXT_MAX_TOKEN 65535

int glove_text_abi_version(void);

/* ---- bytes -> tokens -------------------------------------------------------------------------------------------------
 * Workspace of glove_text_tokenize_u8 (pure host function; 0 for n_bytes < 0 or n_bytes > 2^31 - 1): with
 * tiles = max(1, ceil(n_bytes / GLOVE_TEXT_TILE_BYTES)), int64 pieces, each rounded up to 256 B:
 *     count[tiles] | offset[tiles] | scan scratch[64 KiB + 8 tiles] */
size_t glove_text_tokenize_workspace_bytes(int64_t n_bytes);

/* The tokens of bytes[0 .. n_bytes) in order: start[t] = the byte offset of token t inside the block, len[t] = its true
 * length, hash[t] as above.  *n_tokens = their number (true size; only the first `cap` are written; a block holds at most
 * (n_bytes + 1) / 2 tokens).  *n_long = how many of the written tokens are longer than GLOVE_TEXT_MAX_TOKEN (they are
 * still written, with their true length and the hash of their first GLOVE_TEXT_MAX_TOKEN bytes).  n_bytes == 0 writes the
 * two counters and nothing else.
 * One pass counts each tile's token starts (16 B per lane, three more bytes on each side for the flags of the neighbour
 * bytes), rocPRIM scans the tile counts, a second pass numbers the starts and writes each token's start and end, a third
 * one hashes the tokens. */
int glove_text_tokenize_u8(const uint8_t *bytes, int64_t n_bytes, int32_t *start, int32_t *len, uint64_t *hash,
                           int64_t *n_tokens, int64_t *n_long, int64_t cap, void *ws, size_t ws_bytes, void *stream);

/* ---- tokens -> the block's vocabulary --------------------------------------------------------------------------------
 * Workspace of glove_text_block_vocab (pure host function; 0 for cap_tokens < 0 or cap_tokens > 2^31 - 1): for
 * n = max(1, cap_tokens): two uint64[n] (hashes, sorted hashes), four uint32[n] (token indices, sorted indices, run
 * lengths, run starts), a counter, and the scratch of rocPRIM's sort, run-length encoding and scan (16 MiB + 24 n bytes). */
size_t glove_text_block_vocab_workspace_bytes(int64_t cap_tokens);

/* (hash, start, len)[0 .. min(*n_tokens, cap_tokens)) as glove_text_tokenize_u8 wrote them.  Output: the distinct hashes
 * ascending in keys, how often each occurred in counts, and
 *     where = ((base_offset + start of the hash's first occurrence in the block) << 16) | min(its len, 65535),
 * so with base_offset = the file offset of the block's first byte, `where` orders first occurrences over the whole file
 * and says where to read the word.  0 <= base_offset < 2^46.  *n_out = the number of distinct hashes (true size; only the
 * first cap_out are written).
 * A stable radix sort of (hash, token index) and run-length encoding, rocPRIM's, as in glove_cooc_chunk_keys_i32. */
int glove_text_block_vocab(const uint64_t *hash, const int32_t *start, const int32_t *len, const int64_t *n_tokens,
                           int64_t cap_tokens, int64_t base_offset, uint64_t *keys, int64_t *counts, int64_t *where,
                           int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes, void *stream);

/* ---- merge of two vocabularies ---------------------------------------------------------------------------------------
 * Workspace of glove_text_vocab_merge: that of glove_cooc_merge_u64 for the same capacities, laid out the same (tiles of
 * GLOVE_COOC_MERGE_TILE merged positions; 0 for negative capacities or cap_a + cap_b beyond 2^40). */
size_t glove_text_vocab_merge_workspace_bytes(int64_t cap_a, int64_t cap_b);

/* A = (keys_a, counts_a, where_a)[0 .. min(*n_a, cap_a)) and B likewise, keys STRICTLY ascending.  Output: the ascending
 * union of the keys; for a key present in both the count is the int64 sum and `where` the MINIMUM of the two, so the call
 * is commutative and a vocabulary does not depend on the order in which blocks were merged.  *n_out = the union's size
 * (true size; entries at or beyond cap_out are not written).  No output may overlap an input or another output (checked
 * on the host over the capacities: GLOVE_E_BADARG).  The merge-path merge of glove_cooc_merge_u64 with one more payload. */
int glove_text_vocab_merge(const uint64_t *keys_a, const int64_t *counts_a, const int64_t *where_a, const int64_t *n_a,
                           int64_t cap_a, const uint64_t *keys_b, const int64_t *counts_b, const int64_t *where_b,
                           const int64_t *n_b, int64_t cap_b, uint64_t *keys_out, int64_t *counts_out, int64_t *where_out,
                           int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes, void *stream);

/* ---- tokens -> ids ---------------------------------------------------------------------------------------------------
 * The kept words: kept_keys[0 .. n_kept) their hashes, STRICTLY ascending; kept_id their ids; word j's bytes are
 * kept_bytes[kept_off[j] .. kept_off[j + 1]) (kept_off holds n_kept + 1 ascending offsets).  For every token
 * t < min(*n_tokens, cap_tokens) of the block (bytes, start, len, hash as glove_text_tokenize_u8 wrote them):
 *     hash[t] not among kept_keys                          -> ids[t] = 0
 *     hash[t] == kept_keys[j], same length and same bytes  -> ids[t] = kept_id[j]
 *     hash[t] == kept_keys[j], another length or byte      -> ids[t] = 0 and *n_mismatch is incremented
 * (a token that does not lie inside bytes[0 .. n_bytes) counts as a mismatch too).  A mismatch is a 64-bit hash
 * collision.  n_kept == 0 is allowed (every id is 0).  No workspace. */
int glove_text_token_ids_i32(const uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len,
                             const uint64_t *hash, const int64_t *n_tokens, int64_t cap_tokens, const uint64_t *kept_keys,
                             const int32_t *kept_id, const int64_t *kept_off, const uint8_t *kept_bytes, int64_t n_kept,
                             int32_t *ids, int64_t *n_mismatch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_TEXT_HIP_H */
