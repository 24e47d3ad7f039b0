// Phrase detection (word2phrase) on gfx950 (include/glove_phrases_hip.h, libglove_prep_hip.so): a block's adjacent id pairs
// counted, the accepted pairs chosen from the merged counts, and a block's chosen separators rewritten.
//
// Everything streams.  Per token of a block:
//   bigram keys   12 B in (start, len, id) and one separator byte, 8 B out; then rocPRIM's sort and run-length encoding of
//                 the 8-B keys, as glove_cooc_chunk_keys_i32 does with its slots (glove_cooc_keys.h copies both out);
//   join_mark     the same 12 B and the byte, a binary search in the accepted table (small: it stays in the caches), 4 B out
//                 (the slot found, or -1), and 8 B per tile: its last non-candidate index;
//   rocPRIM scan  the running maximum of those, over tiles;
//   join_write    4 B in; for a chosen pair 8 B more, one byte out and one integer atomic.
// select walks the merged table twice (16 B per key and two unigram loads) around rocPRIM's scan of the tile counts.
// No kernel waits for another workgroup: the order between tiles comes from the scans, which are launches of their own.
#include "glove_common.h"
#include "glove_cooc_keys.h"
#include "glove_table_ops.h"
#include "../../include/glove_phrases_hip.h"

#include <cmath>
#include <initializer_list>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

namespace glove {

constexpr int64_t kMaxPhraseTokens = 2147483647;          // tokens and bytes of a block, keys of the accepted table
constexpr int64_t kMaxSelectKeys = (int64_t)1 << 40;
constexpr int kJoinTile = GLOVE_PHRASE_TILE;              // tokens per workgroup
constexpr int kJoinRounds = kJoinTile / kBlock;           // ... in rounds of one token per lane: token order is lane order
constexpr int kSelectTile = GLOVE_PHRASE_SELECT_TILE;     // keys per workgroup
constexpr int kLaneKeys = kSelectTile / kBlock;           // ... consecutive ones per lane
static_assert(kJoinRounds * kBlock == kJoinTile && kLaneKeys * kBlock == kSelectTile, "tiles are whole rounds of the workgroup");
constexpr int kNoIndex = -3;                              // no non-candidate so far (-1 and -2 stand in front of the block)

// the key of pair (t, t + 1), t + 1 < n; all-ones where the pair is not plain or an id is not a kept word's
__device__ inline uint64_t pair_key(const uint8_t *__restrict__ bytes, int64_t n_bytes, const int32_t *__restrict__ start,
                                    const int32_t *__restrict__ len, const int32_t *__restrict__ ids, int64_t t)
{
    const int32_t a = ids[t], b = ids[t + 1];
    if (a <= 0 || b <= 0) return kNoKey;
    const int64_t sep = (int64_t)start[t] + len[t];
    if (sep < 0 || sep >= n_bytes || (int64_t)start[t + 1] != sep + 1 || bytes[sep] != 0x20) return kNoKey;
    return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
}

// ---- bigram keys -----------------------------------------------------------------------------------------------------
// one key slot per token: pair (t, t + 1) in slot t, the sentinel behind the last pair
__global__ void bigram_emit_keys(const uint8_t *__restrict__ bytes, int64_t n_bytes, const int32_t *__restrict__ start,
                                 const int32_t *__restrict__ len, const int32_t *__restrict__ ids,
                                 const int64_t *__restrict__ n_tokens, int64_t cap_tokens, int64_t slots, uint64_t *__restrict__ keys)
{
    const int64_t n = clamp_count(n_tokens, cap_tokens);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < slots; t += (int64_t)gridDim.x * blockDim.x)
        keys[t] = t + 1 < n ? pair_key(bytes, n_bytes, start, len, ids, t) : kNoKey;
}

__global__ void bigram_copy_out(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ ucounts,
                                const int64_t *__restrict__ n_unique, uint64_t *__restrict__ keys_out,
                                int64_t *__restrict__ counts_out, int64_t *__restrict__ n_out, int64_t cap)
{
    copy_out_runs(ukeys, ucounts, n_unique, keys_out, counts_out, n_out, cap);
}

struct BigramWs {
    uint64_t *keys, *keys_sorted, *ukeys;
    uint32_t *ucounts;
    int64_t *n_unique;
    void *prim;
    size_t prim_bytes, bytes;
};

inline BigramWs carve_bigram_ws(void *ws, int64_t cap_tokens)
{
    BigramWs w;
    WsCarver c{(char *)ws};
    const size_t slots = (size_t)(cap_tokens > 0 ? cap_tokens : 1);
    w.keys = c.take<uint64_t>(slots);
    w.keys_sorted = c.take<uint64_t>(slots);
    w.ukeys = w.keys;                       // the unsorted keys are dead once sorted
    w.ucounts = c.take<uint32_t>(slots);
    w.n_unique = c.take<int64_t>(32);
    w.prim_bytes = (size_t)(16u << 20) + slots * 16;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

// ---- select ----------------------------------------------------------------------------------------------------------
// the header's score and acceptance: every operation in double, rounded once, in this order
__device__ inline bool phrase_accepted(uint64_t key, int64_t n_ab, const int64_t *__restrict__ unigram, int32_t V, int64_t N,
                                       int64_t min_count, double threshold, double &score)
{
    const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
    if (n_ab < min_count || a == 0 || b == 0 || a >= (uint32_t)V || b >= (uint32_t)V) return false;
    const int64_t n_a = unigram[a], n_b = unigram[b];
    if (n_a < 1 || n_b < 1) return false;
    score = (double)(n_ab - min_count) / (double)n_a / (double)n_b * (double)N;
    return score > threshold;
}

// WRITE = false: count[tile] = the tile's accepted keys.  WRITE = true: they are written from offset[tile] on.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void select_tiles(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts,
                                                       const int64_t *__restrict__ n_keys, int64_t cap_keys,
                                                       const int64_t *__restrict__ unigram, int32_t V, int64_t N, int64_t min_count,
                                                       double threshold, int64_t *__restrict__ tile_count,
                                                       const int64_t *__restrict__ tile_offset, uint64_t *__restrict__ keys_out,
                                                       int64_t *__restrict__ counts_out, double *__restrict__ score_out,
                                                       int64_t *__restrict__ n_out, int64_t cap_out)
{
    __shared__ int s_wave[kBlock / 64];
    const int64_t n = clamp_count(n_keys, cap_keys);
    const int64_t tile = blockIdx.x, first = tile * kSelectTile + (int64_t)threadIdx.x * kLaneKeys;
    double score[kLaneKeys];
    unsigned take = 0;
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kLaneKeys; ++j) {
        score[j] = 0.0;
        if (first + j < n && phrase_accepted(keys[first + j], counts[first + j], unigram, V, N, min_count, threshold, score[j])) {
            take |= 1u << j;
            ++mine;
        }
    }
    int before, total;
    block_exclusive_scan(mine, s_wave, before, total);
    if (!WRITE) {
        if (threadIdx.x == 0) tile_count[tile] = total;
        return;
    }
    if (tile == (int64_t)gridDim.x - 1 && threadIdx.x == 0) *n_out = tile_offset[tile] + total;
    int64_t at = tile_offset[tile] + before;
#pragma unroll
    for (int j = 0; j < kLaneKeys; ++j) {
        if (!((take >> j) & 1u)) continue;
        if (at < cap_out) {
            keys_out[at] = keys[first + j];
            counts_out[at] = counts[first + j];
            score_out[at] = score[j];
        }
        ++at;
    }
}

// ---- join ------------------------------------------------------------------------------------------------------------
__device__ inline int wave_max_int(int v)
{
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) v = max(v, __shfl_xor(v, dlt, 64));
    return v;
}

// slot[t] = where pair (t, t + 1)'s key lies in the accepted table, -1 where the pair is no candidate; last[tile] = the
// tile's last non-candidate index (kNoIndex: every pair of the tile is a candidate).  Workgroup 0 also takes the carry word
// aside (join_write overwrites it while other workgroups still need it) and clears the join counter.
__global__ __launch_bounds__(kBlock) void join_mark(const uint8_t *__restrict__ bytes, int64_t n_bytes, const int32_t *__restrict__ start,
                                                    const int32_t *__restrict__ len, const int32_t *__restrict__ ids,
                                                    const int64_t *__restrict__ n_tokens, int64_t cap_tokens,
                                                    const uint64_t *__restrict__ phrase_keys, const int64_t *__restrict__ n_phrases,
                                                    int64_t cap_phrases, const int32_t *__restrict__ carry, int32_t *__restrict__ slot,
                                                    int32_t *__restrict__ carry_in, int64_t *__restrict__ tile_last,
                                                    int64_t *__restrict__ n_joined)
{
    __shared__ int s_wave[kBlock / 64];
    const int64_t n = clamp_count(n_tokens, cap_tokens), m = clamp_count(n_phrases, cap_phrases);
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) {
        *carry_in = *carry != 0;
        *n_joined = 0;
    }
    int last = kNoIndex;
#pragma unroll
    for (int r = 0; r < kJoinRounds; ++r) {
        const int64_t t = (int64_t)blockIdx.x * kJoinTile + r * kBlock + tid;
        if (t >= cap_tokens) continue;
        int32_t found = -1;
        const uint64_t key = t + 1 < n ? pair_key(bytes, n_bytes, start, len, ids, t) : kNoKey;
        if (key != kNoKey) {
            int64_t lo = 0, hi = m;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (phrase_keys[mid] < key) lo = mid + 1; else hi = mid;
            }
            if (lo < m && phrase_keys[lo] == key) found = (int32_t)lo;
        }
        slot[t] = found;
        if (found < 0) last = (int)t;           // (t ascends with r: the lane's last one stays)
    }
    last = wave_max_int(last);
    if ((tid & 63) == 0) s_wave[tid >> 6] = last;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int wv = 1; wv < kBlock / 64; ++wv) last = max(last, s_wave[wv]);
        tile_last[blockIdx.x] = last;
    }
}

// chosen[t] = candidate and (t - b(t)) odd; b(t) = the largest non-candidate index < t: that of the tiles in front
// (scanned[tile], or what the carry word says stands in front of the block), of the rounds in front, of the waves in front
// (LDS) and of the lanes in front (a wave scan).  A chosen pair's separator becomes the delimiter.
__global__ __launch_bounds__(kBlock) void join_write(uint8_t *__restrict__ bytes, const int32_t *__restrict__ start,
                                                     const int32_t *__restrict__ len, const int64_t *__restrict__ n_tokens,
                                                     int64_t cap_tokens, uint8_t delimiter, const int32_t *__restrict__ slot,
                                                     const int32_t *__restrict__ carry_in, const int64_t *__restrict__ scanned,
                                                     int32_t *__restrict__ carry, int64_t *__restrict__ joined,
                                                     int64_t *__restrict__ n_joined)
{
    __shared__ int s_wave[kJoinRounds][kBlock / 64];
    const int64_t n = clamp_count(n_tokens, cap_tokens);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t prev = scanned[blockIdx.x];
    // chosen[-1] set: index -1 is a chosen candidate behind the non-candidate -2; clear: -1 is the non-candidate
    int run = prev == kNoIndex ? (*carry_in ? -2 : -1) : (int)prev;
    int count = 0;
#pragma unroll
    for (int r = 0; r < kJoinRounds; ++r) {
        const int64_t t = (int64_t)blockIdx.x * kJoinTile + r * kBlock + tid;
        const bool pair = t + 1 < n;
        const int32_t s = pair ? slot[t] : -1;
        int incl = pair && s < 0 ? (int)t : kNoIndex;
#pragma unroll
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int up = __shfl_up(incl, dlt, 64);
            if (lane >= dlt) incl = max(incl, up);
        }
        int b = __shfl_up(incl, 1, 64);
        if (lane == 0) b = kNoIndex;
        if (lane == 63) s_wave[r][wave] = incl;
        __syncthreads();
        b = max(b, run);
#pragma unroll
        for (int wv = 0; wv < kBlock / 64; ++wv) {
            if (wv < wave) b = max(b, s_wave[r][wv]);
            run = max(run, s_wave[r][wv]);
        }
        const bool chosen = s >= 0 && ((t - b) & 1);
        if (chosen) {
            bytes[(int64_t)start[t] + len[t]] = delimiter;      // (inside the block: join_mark found the 0x20 there)
            atomicAdd((unsigned long long *)(joined + s), 1ull);
            ++count;
        }
        if (pair && t == n - 2) *carry = chosen ? 1 : 0;
    }
    count = wave_sum_int(count);
    if (lane == 0 && count) atomicAdd((unsigned long long *)n_joined, (unsigned long long)count);
}

struct JoinWs {
    int32_t *slot, *carry_in;
    TileCounts tiles;      // count: every tile's last non-candidate index; offset: the running maximum in front of the tile
    size_t bytes;
};

inline JoinWs carve_join_ws(void *ws, int64_t cap_tokens)
{
    JoinWs w;
    WsCarver c{(char *)ws};
    w.slot = c.take<int32_t>((size_t)(cap_tokens > 0 ? cap_tokens : 1));
    w.carry_in = c.take<int32_t>(64);
    w.tiles = carve_tile_counts(c, tiles_of(cap_tokens, kJoinTile));
    w.bytes = c.off;
    return w;
}

inline hipError_t join_scan(const JoinWs &w, void *prim, size_t &need, hipStream_t st)
{
    return rocprim::exclusive_scan(prim, need, w.tiles.count, w.tiles.offset, (int64_t)kNoIndex, (size_t)w.tiles.tiles,
                                   rocprim::maximum<int64_t>(), st);
}

// ---- argument checks -------------------------------------------------------------------------------------------------
struct Span {
    const void *p;
    size_t bytes;
};

// an output that overlaps an input or another output
inline bool outputs_overlap(std::initializer_list<Span> outs, std::initializer_list<Span> ins)
{
    for (const Span *o = outs.begin(); o != outs.end(); ++o) {
        if (!o->p || !o->bytes) continue;
        for (const Span &i : ins)
            if (i.p && i.bytes && overlap(o->p, o->bytes, i.p, i.bytes)) return true;
        for (const Span *q = o + 1; q != outs.end(); ++q)
            if (q->p && q->bytes && overlap(o->p, o->bytes, q->p, q->bytes)) return true;
    }
    return false;
}

// a separator byte of glove_text_hip.h
inline bool separator_byte(int32_t b) { return (b >= 0x09 && b <= 0x0D) || (b >= 0x1C && b <= 0x20); }

// the block's arrays as the three entry points take them
inline bool bad_block(const void *bytes, int64_t n_bytes, const void *start, const void *len, const void *ids, const void *n_tokens,
                      int64_t cap_tokens)
{
    if (n_bytes < 0 || n_bytes > kMaxPhraseTokens || cap_tokens < 0 || cap_tokens > kMaxPhraseTokens || !n_tokens) return true;
    return cap_tokens > 0 && (!start || !len || !ids || (n_bytes > 0 && !bytes));
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_phrases_abi_version(void) { return GLOVE_PHRASES_ABI_VERSION; }

size_t glove_phrase_bigram_workspace_bytes(int64_t cap_tokens)
{
    if (cap_tokens < 0 || cap_tokens > kMaxPhraseTokens) return 0;
    return carve_bigram_ws(nullptr, cap_tokens).bytes;
}

int glove_phrase_bigram_keys_i32(const uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len,
                                 const int32_t *ids, const int64_t *n_tokens, int64_t cap_tokens, uint64_t *keys_out,
                                 int64_t *counts_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes, void *stream)
{
    if (bad_block(bytes, n_bytes, start, len, ids, n_tokens, cap_tokens) || cap < 0 || !n_out || !ws) return GLOVE_E_BADARG;
    if (cap > 0 && (!keys_out || !counts_out)) return GLOVE_E_BADARG;
    const size_t tok4 = (size_t)cap_tokens * 4;
    if (outputs_overlap({{keys_out, (size_t)cap * 8}, {counts_out, (size_t)cap * 8}, {n_out, 8}},
                        {{bytes, (size_t)n_bytes}, {start, tok4}, {len, tok4}, {ids, tok4}, {n_tokens, 8}}))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cap_tokens == 0) {
        HIP_TRY(zero_words(n_out, 2, st));
        return 0;
    }
    const BigramWs w = carve_bigram_ws(ws, cap_tokens);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const size_t slots = (size_t)cap_tokens;
    // all 64 bits: the sentinel (all ones) must sort behind every real key
    size_t need_sort = 0, need_rle = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, need_sort, w.keys, w.keys_sorted, slots, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(nullptr, need_rle, w.keys_sorted, (unsigned int)slots, w.ukeys, w.ucounts, w.n_unique, st));
    if (need_sort > w.prim_bytes || need_rle > w.prim_bytes) return GLOVE_E_WORKSPACE;
    hipLaunchKernelGGL(bigram_emit_keys, dim3(blocks_for(cap_tokens, kBlock)), dim3(kBlock), 0, st, bytes, n_bytes, start, len, ids,
                       n_tokens, cap_tokens, (int64_t)slots, w.keys);
    HIP_TRY(rocprim::radix_sort_keys(w.prim, need_sort, w.keys, w.keys_sorted, slots, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(w.prim, need_rle, w.keys_sorted, (unsigned int)slots, w.ukeys, w.ucounts, w.n_unique, st));
    // n_unique lives on the device: the copy is sized by the worst case and reads it
    hipLaunchKernelGGL(bigram_copy_out, dim3(blocks_for(cap_tokens, kBlock)), dim3(kBlock), 0, st, w.ukeys, w.ucounts, w.n_unique,
                       keys_out, counts_out, n_out, cap);
    return (int)hipGetLastError();
}

size_t glove_phrase_select_workspace_bytes(int64_t cap_keys)
{
    if (cap_keys < 0 || cap_keys > kMaxSelectKeys) return 0;
    return tile_counts_bytes(tiles_of(cap_keys, kSelectTile));
}

int glove_phrase_select(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys,
                        const int64_t *unigram, int32_t V, int64_t total_tokens, int64_t min_count, double threshold,
                        uint64_t *keys_out, int64_t *counts_out, double *score_out, int64_t *n_out, int64_t cap_out,
                        void *ws, size_t ws_bytes, void *stream)
{
    if (cap_keys < 0 || cap_keys > kMaxSelectKeys || V < 1 || total_tokens < 0 || min_count < 1 || !std::isfinite(threshold) ||
        !(threshold > 0.0) || cap_out < 0 || cap_out > kMaxSelectKeys || !n || !unigram || !n_out || !ws)
        return GLOVE_E_BADARG;
    if ((cap_keys > 0 && (!keys || !counts)) || (cap_out > 0 && (!keys_out || !counts_out || !score_out))) return GLOVE_E_BADARG;
    const size_t in8 = (size_t)cap_keys * 8, out8 = (size_t)cap_out * 8;
    if (outputs_overlap({{keys_out, out8}, {counts_out, out8}, {score_out, out8}, {n_out, 8}},
                        {{keys, in8}, {counts, in8}, {n, 8}, {unigram, (size_t)V * 8}}))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cap_keys == 0) {
        HIP_TRY(zero_words(n_out, 2, st));
        return 0;
    }
    WsCarver c{(char *)ws};
    const TileCounts w = carve_tile_counts(c, tiles_of(cap_keys, kSelectTile));
    if (c.off > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need;
    if (const int rc = tile_scan_query(w, need, st)) return rc;
    const dim3 grid((unsigned int)w.tiles);
    hipLaunchKernelGGL(select_tiles<false>, grid, dim3(kBlock), 0, st, keys, counts, n, cap_keys, unigram, V, total_tokens,
                       min_count, threshold, w.count, w.offset, keys_out, counts_out, score_out, n_out, cap_out);
    HIP_TRY(tile_scan(w, w.prim, need, st));
    hipLaunchKernelGGL(select_tiles<true>, grid, dim3(kBlock), 0, st, keys, counts, n, cap_keys, unigram, V, total_tokens,
                       min_count, threshold, w.count, w.offset, keys_out, counts_out, score_out, n_out, cap_out);
    return (int)hipGetLastError();
}

size_t glove_phrase_join_workspace_bytes(int64_t cap_tokens)
{
    if (cap_tokens < 0 || cap_tokens > kMaxPhraseTokens) return 0;
    return carve_join_ws(nullptr, cap_tokens).bytes;
}

int glove_phrase_join_u8(uint8_t *bytes, int64_t n_bytes, const int32_t *start, const int32_t *len, const int32_t *ids,
                         const int64_t *n_tokens, int64_t cap_tokens, const uint64_t *phrase_keys, const int64_t *n_phrases,
                         int64_t cap_phrases, int32_t delimiter, int32_t *carry, int64_t *joined, int64_t *n_joined,
                         void *ws, size_t ws_bytes, void *stream)
{
    if (bad_block(bytes, n_bytes, start, len, ids, n_tokens, cap_tokens) || cap_phrases < 0 || cap_phrases > kMaxPhraseTokens ||
        delimiter < 0 || delimiter > 127 || separator_byte(delimiter) || !n_phrases || !carry || !n_joined || !ws)
        return GLOVE_E_BADARG;
    if (cap_phrases > 0 && (!phrase_keys || !joined)) return GLOVE_E_BADARG;
    const size_t tok4 = (size_t)cap_tokens * 4, phr8 = (size_t)cap_phrases * 8;
    if (outputs_overlap({{bytes, (size_t)n_bytes}, {joined, phr8}, {carry, 4}, {n_joined, 8}},
                        {{start, tok4}, {len, tok4}, {ids, tok4}, {n_tokens, 8}, {phrase_keys, phr8}, {n_phrases, 8}}))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cap_tokens == 0) {
        HIP_TRY(zero_words(n_joined, 2, st));
        return 0;
    }
    const JoinWs w = carve_join_ws(ws, cap_tokens);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need = 0;
    HIP_TRY(join_scan(w, nullptr, need, st));
    if (need > w.tiles.prim_bytes) return GLOVE_E_WORKSPACE;
    const dim3 grid((unsigned int)w.tiles.tiles);
    hipLaunchKernelGGL(join_mark, grid, dim3(kBlock), 0, st, bytes, n_bytes, start, len, ids, n_tokens, cap_tokens, phrase_keys,
                       n_phrases, cap_phrases, carry, w.slot, w.carry_in, w.tiles.count, n_joined);
    HIP_TRY(join_scan(w, w.tiles.prim, need, st));
    hipLaunchKernelGGL(join_write, grid, dim3(kBlock), 0, st, bytes, start, len, n_tokens, cap_tokens, (uint8_t)delimiter, w.slot,
                       w.carry_in, w.tiles.offset, carry, joined, n_joined);
    return (int)hipGetLastError();
}

}  // extern "C"
