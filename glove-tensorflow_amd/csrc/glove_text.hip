// Tokenizing and numbering a corpus on gfx950 (include/glove_text_hip.h, libglove_prep_hip.so).
//
// trainer.cooccur reads a corpus twice: pass one counts the vocabulary, pass two maps every token to its id.  Both were
// Python loops over str.split().  Here a block of the file's bytes is tokenized on the device:
//   text_count_starts   one workgroup per tile of 4096 bytes, 16 B per lane: separator flags, token starts per tile;
//   rocPRIM scan        of the tile counts;
//   text_emit_tokens    the same flags again; starts numbered by a block scan; every token's start and end written;
//   text_hash_tokens    one lane per token: length, FNV-1a hash;
// the block's vocabulary is a stable radix sort of (hash, token index) and a run-length encoding (rocPRIM, as
// glove_cooc_chunk_keys_i32), two vocabularies are merged by the merge-path merge of glove_table_ops.hip with `where` as a
// second payload word, and pass two looks every token's hash up in the sorted table of the kept words and compares the bytes.
// Integers only; the two counters (tokens too long, hash collisions) are integer atomics.
#include "glove_common.h"
#include "glove_table_ops.h"
#include "../../include/glove_cooc_stream_hip.h"
#include "../../include/glove_text_hip.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace glove {

// ---- tokenizer -------------------------------------------------------------------------------------------------------
constexpr int kTextTile = GLOVE_TEXT_TILE_BYTES;      // bytes per workgroup
constexpr int kLaneBytes = kTextTile / kBlock;        // ... per lane
static_assert(kLaneBytes == 16 && kLaneBytes * kBlock == kTextTile, "a lane reads one 16-B word");
constexpr int kHalo = 3;      // a flag looks two bytes to each side, a start / an end at the flag of the byte beside it
constexpr int64_t kMaxTextBytes = 2147483647;
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;

__device__ inline bool ascii_separator(uint32_t c) { return (c >= 0x09 && c <= 0x0D) || (c >= 0x1C && c <= 0x20); }

// the length of the separator sequence that starts with the bytes a b c, 0 where none does
__device__ inline int separator_sequence(uint32_t a, uint32_t b, uint32_t c)
{
    if (a == 0xC2) return (b == 0x85 || b == 0xA0) ? 2 : 0;
    if (a == 0xE1) return (b == 0x9A && c == 0x80) ? 3 : 0;
    if (a == 0xE2) {
        if (b == 0x80) return ((c >= 0x80 && c <= 0x8A) || c == 0xA8 || c == 0xA9 || c == 0xAF) ? 3 : 0;
        return (b == 0x81 && c == 0x9F) ? 3 : 0;
    }
    if (a == 0xE3) return (b == 0x80 && c == 0x80) ? 3 : 0;
    return 0;
}

// The tile's bytes into LDS (sb[16 + i] = byte i of the tile, kHalo bytes of the neighbours on each side; bytes outside
// the block read as 00, which neither separates nor belongs to a sequence), then this lane's flags: bit i of `starts`
// (`ends`) is set where the lane's byte i is the first (last) byte of a token.  Holds a __syncthreads.
__device__ inline void tile_flags(const uint8_t *__restrict__ bytes, int64_t n, int64_t tile, uint8_t *sb, uint32_t &starts,
                                  uint32_t &ends)
{
    const int tid = threadIdx.x;
    const int64_t t0 = tile * kTextTile, base = t0 + (int64_t)tid * kLaneBytes;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (((uintptr_t)bytes & 15) == 0 && base + kLaneBytes <= n) {
        v = *(const uint4 *)(bytes + base);
    } else if (base < n) {                  // the block's tail, or a block that does not start on a 16-B boundary
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < kLaneBytes && base + i < n; ++i) word[i >> 2] |= (uint32_t)bytes[base + i] << (8 * (i & 3));
        v = make_uint4(word[0], word[1], word[2], word[3]);
    }
    *(uint4 *)(sb + 16 + tid * kLaneBytes) = v;
    if (tid < 2 * kHalo) {
        const int64_t p = tid < kHalo ? t0 - kHalo + tid : t0 + kTextTile + (tid - kHalo);
        sb[tid < kHalo ? 16 - kHalo + tid : 16 + kTextTile + (tid - kHalo)] = (p >= 0 && p < n) ? bytes[p] : (uint8_t)0;
    }
    __syncthreads();

    // w[j] = byte base - kHalo + j; bit j of sep: that byte is a separator byte (j = 2 .. 19 are complete)
    uint32_t w[kLaneBytes + 2 * kHalo];
#pragma unroll
    for (int j = 0; j < kLaneBytes + 2 * kHalo; ++j) w[j] = sb[16 - kHalo + tid * kLaneBytes + j];
    uint32_t sep = 0;
#pragma unroll
    for (int j = 0; j < kLaneBytes + 2 * kHalo - 2; ++j) {
        if (ascii_separator(w[j])) sep |= 1u << j;
        const int L = separator_sequence(w[j], w[j + 1], w[j + 2]);
        if (L) sep |= ((1u << L) - 1u) << j;
    }
    const uint32_t own = base + kLaneBytes <= n ? 0xFFFFu : (base < n ? (1u << (int)(n - base)) - 1u : 0u);
    const uint32_t tok = ~(sep >> kHalo) & own;                 // bit i: the lane's byte i is a token byte
    uint32_t before = sep >> (kHalo - 1), after = sep >> (kHalo + 1);      // bit i: the byte before / after it separates
    if (base == 0) before |= 1u;                                // the block's first byte starts a token if it is one
    if (n - base >= 1 && n - base <= kLaneBytes) after |= 1u << (int)(n - 1 - base);      // ... its last byte ends one
    starts = tok & before;
    ends = tok & after;
}

__global__ __launch_bounds__(kBlock) void text_count_starts(const uint8_t *__restrict__ bytes, int64_t n,
                                                            int64_t *__restrict__ tile_count, int64_t *__restrict__ n_long)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[16 + kTextTile + 16];
    __shared__ int s_wave[kBlock / 64];
    uint32_t starts, ends;
    tile_flags(bytes, n, blockIdx.x, sb, starts, ends);
    int before, total;
    block_exclusive_scan(__popc(starts), s_wave, before, total);
    if (threadIdx.x == 0) {
        tile_count[blockIdx.x] = total;
        if (blockIdx.x == 0) *n_long = 0;          // text_hash_tokens counts into it
    }
}

// start[t] = the token's first byte; len[t] = one past its last byte for now (text_hash_tokens makes it the length).  The
// token that ends at a byte is the last one that started: number (starts so far) - 1, wherever it started.
__global__ __launch_bounds__(kBlock) void text_emit_tokens(const uint8_t *__restrict__ bytes, int64_t n,
                                                           const int64_t *__restrict__ tile_count,
                                                           const int64_t *__restrict__ tile_offset, int32_t *__restrict__ start,
                                                           int32_t *__restrict__ len, int64_t *__restrict__ n_tokens, int64_t cap)
{
    __shared__ __attribute__((aligned(16))) uint8_t sb[16 + kTextTile + 16];
    __shared__ int s_wave[kBlock / 64];
    uint32_t starts, ends;
    tile_flags(bytes, n, blockIdx.x, sb, starts, ends);
    int before, total;
    block_exclusive_scan(__popc(starts), s_wave, before, total);
    const int64_t tile = blockIdx.x;
    if (threadIdx.x == 0 && tile == (int64_t)gridDim.x - 1) *n_tokens = tile_offset[tile] + tile_count[tile];
    int64_t t = tile_offset[tile] + before;       // tokens that started in front of this lane's bytes
    const int64_t base = tile * kTextTile + (int64_t)threadIdx.x * kLaneBytes;
#pragma unroll
    for (int i = 0; i < kLaneBytes; ++i) {
        if ((starts >> i) & 1u) {
            if (t < cap) start[t] = (int32_t)(base + i);
            ++t;
        }
        if (((ends >> i) & 1u) && t > 0 && t - 1 < cap) len[t - 1] = (int32_t)(base + i + 1);
    }
}

__device__ inline uint64_t fnv1a(const uint8_t *__restrict__ p, int n)
{
    uint64_t h = kFnvBasis;
    for (int i = 0; i < n; ++i) h = (h ^ p[i]) * kFnvPrime;
    return h == kNoKey ? kNoKey - 1 : h;
}

__global__ void text_hash_tokens(const uint8_t *__restrict__ bytes, const int32_t *__restrict__ start, int32_t *__restrict__ len,
                                 uint64_t *__restrict__ hash, const int64_t *__restrict__ n_tokens, int64_t cap,
                                 int64_t *__restrict__ n_long)
{
    const int64_t m = clamp_count(n_tokens, cap);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t s = start[t], L = len[t] - s;
        len[t] = L;
        hash[t] = fnv1a(bytes + s, L < GLOVE_TEXT_MAX_TOKEN ? L : GLOVE_TEXT_MAX_TOKEN);
        if (L > GLOVE_TEXT_MAX_TOKEN) atomicAdd((unsigned long long *)n_long, 1ull);
    }
}

// ---- block vocabulary ------------------------------------------------------------------------------------------------
// the sort's input: (hash, token index); slots behind the tokens hold the sentinel, which sorts last
__global__ void vocab_sort_input(const uint64_t *__restrict__ hash, const int64_t *__restrict__ n_tokens, int64_t cap_tokens,
                                 uint64_t *__restrict__ keys, uint32_t *__restrict__ index)
{
    const int64_t m = clamp_count(n_tokens, cap_tokens);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap_tokens; i += (int64_t)gridDim.x * blockDim.x) {
        keys[i] = i < m ? hash[i] : kNoKey;
        index[i] = (uint32_t)i;
    }
}

// the runs without the sentinel's, cut at cap_out; the sort is stable, so a run starts with the hash's first occurrence
__global__ void vocab_copy_out(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ ucounts,
                               const uint32_t *__restrict__ run_start, const uint32_t *__restrict__ sorted_index,
                               const int64_t *__restrict__ n_unique, const int32_t *__restrict__ start,
                               const int32_t *__restrict__ len, int64_t base_offset, uint64_t *__restrict__ keys,
                               int64_t *__restrict__ counts, int64_t *__restrict__ where, int64_t *__restrict__ n_out,
                               int64_t cap_out)
{
    int64_t m = *n_unique;
    if (m > 0 && ukeys[m - 1] == kNoKey) --m;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = m;
    if (m > cap_out) m = cap_out;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t t = sorted_index[run_start[i]];
        const int64_t L = len[t];
        keys[i] = ukeys[i];
        counts[i] = (int64_t)ucounts[i];
        where[i] = ((base_offset + start[t]) << 16) | (L < GLOVE_TEXT_MAX_TOKEN ? L : GLOVE_TEXT_MAX_TOKEN);
    }
}

struct VocabWs {
    uint64_t *keys, *keys_sorted, *ukeys;
    uint32_t *index, *index_sorted, *ucounts, *run_start;
    int64_t *n_unique;
    void *prim;
    size_t prim_bytes, bytes;
};

static VocabWs carve_vocab_ws(void *ws, int64_t cap_tokens)
{
    VocabWs w;
    WsCarver c{(char *)ws};
    const size_t n = (size_t)(cap_tokens > 0 ? cap_tokens : 1);
    w.keys = c.take<uint64_t>(n);
    w.keys_sorted = c.take<uint64_t>(n);
    w.ukeys = w.keys;                       // the unsorted hashes are dead once sorted
    w.index = c.take<uint32_t>(n);
    w.index_sorted = c.take<uint32_t>(n);
    w.ucounts = c.take<uint32_t>(n);
    w.run_start = c.take<uint32_t>(n);
    w.n_unique = c.take<int64_t>(32);
    w.prim_bytes = (size_t)(16u << 20) + n * 24;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

// ---- token ids -------------------------------------------------------------------------------------------------------
__global__ void text_token_ids(const uint8_t *__restrict__ bytes, int64_t n_bytes, const int32_t *__restrict__ start,
                               const int32_t *__restrict__ len, const uint64_t *__restrict__ hash,
                               const int64_t *__restrict__ n_tokens, int64_t cap_tokens, const uint64_t *__restrict__ kept_keys,
                               const int32_t *__restrict__ kept_id, const int64_t *__restrict__ kept_off,
                               const uint8_t *__restrict__ kept_bytes, int64_t n_kept, int32_t *__restrict__ ids,
                               int64_t *__restrict__ n_mismatch)
{
    const int64_t m = clamp_count(n_tokens, cap_tokens);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m; t += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = hash[t];
        int64_t lo = 0, hi = n_kept;            // the first kept key >= h
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (kept_keys[mid] < h) lo = mid + 1; else hi = mid;
        }
        int32_t id = 0;
        if (lo < n_kept && kept_keys[lo] == h) {
            const int64_t s = start[t], L = len[t], k0 = kept_off[lo];
            bool same = s >= 0 && L >= 0 && s + L <= n_bytes && kept_off[lo + 1] - k0 == L;
            for (int64_t i = 0; same && i < L; ++i) same = bytes[s + i] == kept_bytes[k0 + i];
            if (same) id = kept_id[lo];
            else atomicAdd((unsigned long long *)n_mismatch, 1ull);
        }
        ids[t] = id;
    }
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_text_abi_version(void) { return GLOVE_TEXT_ABI_VERSION; }

size_t glove_text_tokenize_workspace_bytes(int64_t n_bytes)
{
    if (n_bytes < 0 || n_bytes > kMaxTextBytes) return 0;
    return tile_counts_bytes(tiles_of(n_bytes, kTextTile));
}

int glove_text_tokenize_u8(const uint8_t *bytes, int64_t n_bytes, int32_t *start, int32_t *len, uint64_t *hash,
                           int64_t *n_tokens, int64_t *n_long, int64_t cap, void *ws, size_t ws_bytes, void *stream)
{
    if (n_bytes < 0 || n_bytes > kMaxTextBytes || cap < 0 || !n_tokens || !n_long || !ws) return GLOVE_E_BADARG;
    if (overlap(n_tokens, 8, n_long, 8)) return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_bytes == 0) {
        HIP_TRY(zero_words(n_tokens, 2, st));
        HIP_TRY(zero_words(n_long, 2, st));
        return 0;
    }
    if (!bytes || (cap > 0 && (!start || !len || !hash))) return GLOVE_E_BADARG;
    WsCarver c{(char *)ws};
    const TileCounts w = carve_tile_counts(c, tiles_of(n_bytes, kTextTile));
    if (c.off > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need;
    if (const int rc = tile_scan_query(w, need, st)) return rc;
    const dim3 grid((unsigned int)w.tiles);
    hipLaunchKernelGGL(text_count_starts, grid, dim3(kBlock), 0, st, bytes, n_bytes, w.count, n_long);
    HIP_TRY(tile_scan(w, w.prim, need, st));
    hipLaunchKernelGGL(text_emit_tokens, grid, dim3(kBlock), 0, st, bytes, n_bytes, w.count, w.offset, start, len, n_tokens, cap);
    // n_tokens lives on the device: the hashing pass is sized by the capacity (and by the most tokens the bytes can hold)
    const int64_t most = cap < (n_bytes + 1) / 2 ? cap : (n_bytes + 1) / 2;
    hipLaunchKernelGGL(text_hash_tokens, dim3(blocks_for(most, kBlock)), dim3(kBlock), 0, st, bytes, start, len, hash, n_tokens,
                       cap, n_long);
    return (int)hipGetLastError();
}

size_t glove_text_block_vocab_workspace_bytes(int64_t cap_tokens)
{
    if (cap_tokens < 0 || cap_tokens > kMaxTextBytes) return 0;
    return carve_vocab_ws(nullptr, cap_tokens).bytes;
}

int glove_text_block_vocab(const uint64_t *hash, const int32_t *start, const int32_t *len, const int64_t *n_tokens,
                           int64_t cap_tokens, int64_t base_offset, uint64_t *keys, int64_t *counts, int64_t *where,
                           int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes, void *stream)
{
    if (cap_tokens < 0 || cap_tokens > kMaxTextBytes || cap_out < 0 || base_offset < 0 || base_offset >= ((int64_t)1 << 46) ||
        !n_tokens || !n_out || !ws)
        return GLOVE_E_BADARG;
    if ((cap_tokens > 0 && (!hash || !start || !len)) || (cap_out > 0 && (!keys || !counts || !where))) return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cap_tokens == 0) {
        HIP_TRY(zero_words(n_out, 2, st));
        return 0;
    }
    const VocabWs w = carve_vocab_ws(ws, cap_tokens);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const size_t n = (size_t)cap_tokens;
    size_t need_sort = 0, need_rle = 0, need_scan = 0;
    // all 64 bits: the sentinel (all ones) must sort behind every hash
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, need_sort, w.keys, w.keys_sorted, w.index, w.index_sorted, n, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(nullptr, need_rle, w.keys_sorted, (unsigned int)n, w.ukeys, w.ucounts, w.n_unique, st));
    HIP_TRY(rocprim::exclusive_scan(nullptr, need_scan, w.ucounts, w.run_start, 0u, n, rocprim::plus<uint32_t>(), st));
    if (need_sort > w.prim_bytes || need_rle > w.prim_bytes || need_scan > w.prim_bytes) return GLOVE_E_WORKSPACE;
    const dim3 grid(blocks_for(cap_tokens, kBlock));
    hipLaunchKernelGGL(vocab_sort_input, grid, dim3(kBlock), 0, st, hash, n_tokens, cap_tokens, w.keys, w.index);
    HIP_TRY(rocprim::radix_sort_pairs(w.prim, need_sort, w.keys, w.keys_sorted, w.index, w.index_sorted, n, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(w.prim, need_rle, w.keys_sorted, (unsigned int)n, w.ukeys, w.ucounts, w.n_unique, st));
    // run lengths behind *n_unique are stale; the starts of the runs in front of it do not depend on them
    HIP_TRY(rocprim::exclusive_scan(w.prim, need_scan, w.ucounts, w.run_start, 0u, n, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(vocab_copy_out, grid, dim3(kBlock), 0, st, w.ukeys, w.ucounts, w.run_start, w.index_sorted, w.n_unique,
                       start, len, base_offset, keys, counts, where, n_out, cap_out);
    return (int)hipGetLastError();
}

size_t glove_text_vocab_merge_workspace_bytes(int64_t cap_a, int64_t cap_b) { return merge_workspace_bytes(cap_a, cap_b); }

int glove_text_vocab_merge(const uint64_t *keys_a, const int64_t *counts_a, const int64_t *where_a, const int64_t *n_a,
                           int64_t cap_a, const uint64_t *keys_b, const int64_t *counts_b, const int64_t *where_b,
                           const int64_t *n_b, int64_t cap_b, uint64_t *keys_out, int64_t *counts_out, int64_t *where_out,
                           int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes, void *stream)
{
    // summed counts, the smaller `where`: the word's first occurrence in the file
    const MergeIn a = {keys_a, {counts_a, where_a}, n_a, cap_a}, b = {keys_b, {counts_b, where_b}, n_b, cap_b};
    const MergeOut out = {keys_out, {counts_out, where_out}, n_out, cap_out};
    return merge_tables(a, b, out, 2, ws, ws_bytes, (hipStream_t)stream);
}

int glove_text_token_ids_i32(const uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len,
                             const uint64_t *hash, const int64_t *n_tokens, int64_t cap_tokens, const uint64_t *kept_keys,
                             const int32_t *kept_id, const int64_t *kept_off, const uint8_t *kept_bytes, int64_t n_kept,
                             int32_t *ids, int64_t *n_mismatch, void *stream)
{
    if (n_bytes < 0 || n_bytes > kMaxTextBytes || cap_tokens < 0 || cap_tokens > kMaxTextBytes || n_kept < 0 ||
        n_kept > kMaxTextBytes || !n_tokens || !n_mismatch || !kept_off)
        return GLOVE_E_BADARG;
    if ((n_kept > 0 && (!kept_keys || !kept_id || !kept_bytes)) || (cap_tokens > 0 && (!start || !len || !hash || !ids)) ||
        (cap_tokens > 0 && n_bytes > 0 && !bytes))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(zero_words(n_mismatch, 2, st));
    if (cap_tokens == 0) return 0;
    hipLaunchKernelGGL(text_token_ids, dim3(blocks_for(cap_tokens, kBlock)), dim3(kBlock), 0, st, bytes, n_bytes, start, len, hash,
                       n_tokens, cap_tokens, kept_keys, kept_id, kept_off, kept_bytes, n_kept, ids, n_mismatch);
    return (int)hipGetLastError();
}

}  // extern "C"
