/*
 * glove_vectors_hip.h — C ABI of libglove_prep_hip.so, third header: reading and writing word-vector text files
 * (`word v1 ... vd` per line: GloVe's vectors.txt, word2vec / fastText .vec) on the MI355X (gfx950).  A block of the file's
 * raw bytes goes in and its records and their float32 values come out; a float32 table and its words go in and the text of
 * the block comes out.  Both directions are exact integer problems; tests/vectors_ref.py restates the two rules.
 * glove_cooc_stream_hip.h and glove_text_hip.h stay as they are and keep their own versions; the entry points below are
 * versioned by GLOVE_VECTORS_ABI_VERSION.
 *
 * Conventions (those of glove_text_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, keeps no global state and
 *     never synchronizes; its kernels clear their counters themselves, with no memset nodes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns: grids are sized from
 *     host-known capacities, never from counts the device computed;
 *   - sizes the device computed (n_lines, n_fallback, n_host_rows, row_off[n_rows]) are int64 in device memory; a size
 *     written by a call is the TRUE size even where it exceeds the capacity, and nothing is written at or beyond a capacity;
 *   - counters are integer atomics: no result depends on the grid or on the order in which workgroups run (the ORDER of
 *     the fallback list does; its set does not).
 *
 * Fields and records.  The SEPARATOR bytes are 20, 0A and 0D, and no others: tab, NBSP (C2 A0) and the other Unicode
 * spaces are ordinary word bytes (glove.840B.300d has words that contain them, which is why the tokenizer of
 * glove_text_hip.h is not used here).  A field is a maximal run of non-separator bytes; a record is the fields between two
 * 0A bytes (or between an end of the block and a 0A); a line without fields is no record.  Field 0 is the word, fields
 * 1 .. d are the numbers.
 *
 * Decimal -> float32.  The value of a number token is np.float32(float(token)): rounded once to double, once to float.
 * The device computes it on Clinger's fast path only.  Grammar: an optional sign, decimal digits with at most one '.' and
 * at least one digit, an optional e / E with an optional sign and digits.  With the leading zeros stripped at most 15
 * significant digits may remain; they are the integer m (< 10^15 < 2^53); e10 = the written exponent minus the number of
 * fraction digits.  m == 0 gives +-0; 0 <= e10 <= 22 gives double(m) * 10^e10; -22 <= e10 < 0 gives double(m) / 10^-e10:
 * one correctly rounded IEEE double operation on exact operands, hence strtod's result; then the sign and (float).  Every
 * other token (16 or more digits, 1e23, 1e-45, nan, inf, 0x10, 1_0, --1, 1.2.3, ...) is a FALLBACK: the device writes
 * nothing for it and lists it, the host parses those few.
 *
 * float32 -> fixed decimal.  The text of x at precision p (0 .. 9) is "%.*f" % (p, x), correctly rounded, ties to even,
 * in integers: x = +-m 2^ex with m < 2^24 (subnormals: ex = -149); n = m 10^p < 2^54; ex >= 0 (up to 7: |x| < 2^31):
 * q = n << ex; ex < 0, s = -ex: s >= 64 gives q = 0, otherwise q = n >> s, r = n & (2^s - 1), one more if r > 2^(s-1) or
 * r == 2^(s-1) and q is odd.  The text is the sign ('-' where the sign bit is set, -0.0 included), q / 10^p, and for p > 0
 * a '.' and q % 10^p zero-padded to p digits.  A row that holds a NaN, an infinity or |x| >= 2^31 is a HOST ROW: the device
 * gives it length 0 and flags it, the host formats it.
 */
#ifndef GLOVE_VECTORS_HIP_H
#define GLOVE_VECTORS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_VECTORS_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / an output aliases an input */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* Bytes of a block one workgroup of glove_vectors_lines_u8 owns (a tile): 256 lanes x 16 B. */
#define GLOVE_VECTORS_TILE_BYTES 4096
/* The longest token length a fallback span can hold. */
#define GLOVE_VECTORS_MAX_SPAN 65535
/* The widest row: numbers per record, columns of a table. */
#define GLOVE_VECTORS_MAX_D 65536

int glove_vectors_abi_version(void);

/* ---- bytes -> records ------------------------------------------------------------------------------------------------
 * Workspace of glove_vectors_lines_u8 (pure host function; 0 for n_bytes < 0, n_bytes > 2^31 - 1 or cap < 0): with
 * tiles = max(1, ceil(n_bytes / GLOVE_VECTORS_TILE_BYTES)) and lines = max(1, min(cap, (n_bytes + 1) / 2)), each piece
 * rounded up to 256 B:
 *     tile summary[tiles] (16 B each) | tile prefix[tiles] (16 B each) | fields so far int32[lines] |
 *     scan scratch[64 KiB + 16 tiles] */
size_t glove_vectors_lines_workspace_bytes(int64_t n_bytes, int64_t cap);

/* The records of bytes[0 .. n_bytes) in order: line_start[r] = the byte offset of the first byte of record r's word,
 * line_fields[r] = its number of fields (the word included).  *n_lines = their number (true size; only the first `cap`
 * are written; a block holds at most (n_bytes + 1) / 2 records).  n_bytes == 0 writes the counter and nothing else.
 * A tile's summary says, for both states it can be entered in (the line has no field yet / has one), how many records
 * start in it and in which state it is left, and how many fields start in it; rocPRIM scans the summaries (composition
 * is associative), a second pass numbers the record starts and notes the fields so far at every record's end, a third
 * takes the differences.  A record may be longer than any number of tiles. */
int glove_vectors_lines_u8(const uint8_t *bytes, int64_t n_bytes, int32_t *line_start, int32_t *line_fields, int64_t *n_lines,
                           int64_t cap, void *ws, size_t ws_bytes, void *stream);

/* ---- records -> float32 ----------------------------------------------------------------------------------------------
 * For every record r < min(*n_lines, cap_lines) (line_start as glove_vectors_lines_u8 wrote it): fields 1 .. d parsed
 * into vec[r * ld + 0 .. d) by the rule above, columns d .. ld written as zero (ld % 4 == 0, ld >= d,
 * 1 <= d <= GLOVE_VECTORS_MAX_D), the columns of missing fields written as zero, fields beyond d ignored (the host has
 * refused such a record by its field count); word_len[r] = the length of the word.  A fallback token is not written to vec;
 * it is listed as fb_index = r * ld + column and fb_span = (its byte offset << 16) | min(its length, 65535), in no fixed
 * order.  *n_fallback = their number (true size; only the first cap_fb are listed).  No workspace.
 * One wave per record: 64 bytes per trip, the separators balloted, field starts numbered by a prefix popcount, the lane
 * that holds a field start parses its token. */
int glove_vectors_parse_f32(const uint8_t *bytes, int64_t n_bytes, const int32_t *line_start, const int64_t *n_lines,
                            int64_t cap_lines, int32_t d, int32_t ld, float *vec, int32_t *word_len, int64_t *fb_index,
                            int64_t *fb_span, int64_t *n_fallback, int64_t cap_fb, void *stream);

/* ---- float32 -> text -------------------------------------------------------------------------------------------------
 * Workspace of glove_vectors_format_f32 (pure host function; 0 for n_rows < 0, n_rows >= 2^31, d < 1 or
 * d > GLOVE_VECTORS_MAX_D): row lengths int64[n_rows + 1] rounded up to 256 B | scan scratch[64 KiB + 8 (n_rows + 1)]. */
size_t glove_vectors_format_workspace_bytes(int64_t n_rows, int32_t d);

/* Rows W[r * ld + 0 .. d), r < n_rows (ld >= d; any ld), whose words are word_bytes[word_off[r] .. word_off[r + 1])
 * (n_rows + 1 ascending offsets).  The text of row r is the word, then for each value a 20 byte and its decimal at
 * `precision` (0 .. 9) by the rule above, then 0A; it is written to out[row_off[r] .. row_off[r + 1]).  A host row has
 * length 0 and host_row[r] = 1 (every other row: 0); *n_host_rows counts them.  row_off[n_rows] = the block's size (true
 * size; bytes at or beyond cap_out are not written).  A row takes at most its word's bytes + d (precision + 13) + 1.
 * Pass one computes each row's length (one wave per row), rocPRIM scans the lengths, pass two writes. */
int glove_vectors_format_f32(const float *W, int64_t n_rows, int32_t d, int32_t ld, int32_t precision,
                             const uint8_t *word_bytes, const int64_t *word_off, uint8_t *out, int64_t *row_off,
                             uint8_t *host_row, int64_t *n_host_rows, int64_t cap_out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_VECTORS_HIP_H */
