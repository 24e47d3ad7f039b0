// The preprocessing options of the corpus-to-counts stage on gfx950 (include/glove_cooc_options_hip.h,
// libglove_prep_hip.so): a stream compaction of the token ids under a per-position keep decision, and the finalisation of
// glove_table_ops.hip with other distance weightings.
//
// The filter reads 4 B per token and writes 4 B per survivor, twice over the input:
//   filter_tiles<0>   one workgroup per tile of GLOVE_FILTER_TILE tokens: every lane decides four consecutive tokens, a wave
//                     ranks the decisions by ballot and popcount, the four wave totals meet in LDS; count[tile] = the survivors;
//   rocPRIM scan      of the tile counts;
//   filter_tiles<1>   the same decisions again (a hash of the position and one threshold load: cheaper than keeping them);
//                     survivors go to LDS at their rank and leave at offset[tile] in 16-B stores.
// The decision is a function of the token's id and its GLOBAL position: nothing depends on the grid, the tile or the block cut.
#include "glove_common.h"
#include "glove_table_ops.h"
#include "../../include/glove_cooc_options_hip.h"

namespace glove {

static_assert(kWindowHarmonic == GLOVE_WINDOW_HARMONIC && kWindowUniform == GLOVE_WINDOW_UNIFORM &&
              kWindowDynamic == GLOVE_WINDOW_DYNAMIC, "glove_table_ops.h names the header's weightings");

// ---- token filter ----------------------------------------------------------------------------------------------------
constexpr int kFilterTile = GLOVE_FILTER_TILE;            // tokens per workgroup
constexpr int kLaneTokens = 4;                            // ... per lane and round: one 16-B load
constexpr int kRoundTokens = 64 * kLaneTokens;            // ... per wave and round
constexpr int kWaveTokens = kFilterTile / (kBlock / 64);  // a wave owns a contiguous quarter of the tile
constexpr int kRounds = kWaveTokens / kRoundTokens;
static_assert(kRounds * kRoundTokens * (kBlock / 64) == kFilterTile && kRounds == 4, "a wave walks its quarter in four rounds");
constexpr int64_t kMaxFilterTokens = 2147483647;

// u(seed, p) of the header; x0 = p + (seed + 1) * 0x9E3779B97F4A7C15 (the host folds pos0 and the seed into one addend)
__device__ inline uint32_t filter_u(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (uint32_t)(x >> 32);
}

// the threshold of a token: 0 (always dropped) for an id outside [0, V) — the caller's error, never an index
__device__ inline uint32_t filter_threshold(int32_t id, const uint32_t *__restrict__ thresholds, int32_t V)
{
    return (uint32_t)id < (uint32_t)V ? thresholds[id] : 0u;
}

// n survivors from LDS to g: 16 B per lane from the first 16-B aligned element on
__device__ inline void store_ids(int32_t *__restrict__ g, int n, const int32_t *s)
{
    int head = (int)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int quads = (n - head) >> 2, tail = head + 4 * quads;
    if ((int)threadIdx.x < head) g[threadIdx.x] = s[threadIdx.x];
    int4 *g4 = (int4 *)(g + head);
    for (int q = threadIdx.x; q < quads; q += kBlock) {
        const int *e = s + head + 4 * q;
        g4[q] = make_int4(e[0], e[1], e[2], e[3]);
    }
    if ((int)threadIdx.x < n - tail) g[tail + threadIdx.x] = s[tail + threadIdx.x];
}

// WRITE = false: count[tile] = the tile's number of survivors.  WRITE = true: the survivors, at offset[tile].
// hash_add = pos0 + (seed + 1) * 0x9E3779B97F4A7C15 (mod 2^64): token i of the block hashes hash_add + i.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void filter_tiles(const int32_t *__restrict__ ids, int64_t n, uint64_t hash_add,
                                                       const uint32_t *__restrict__ thresholds, int32_t V,
                                                       int64_t *__restrict__ tile_count, const int64_t *__restrict__ tile_offset,
                                                       int32_t *__restrict__ ids_out, int64_t *__restrict__ n_out, int64_t cap)
{
    __shared__ __attribute__((aligned(16))) int32_t s_out[WRITE ? kFilterTile : 4];
    __shared__ int s_wave[kBlock / 64];

    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (WRITE && tile == (int64_t)gridDim.x - 1 && tid == 0) *n_out = tile_offset[tile] + tile_count[tile];
    const bool aligned = ((uintptr_t)ids & 15) == 0;      // a tile starts a multiple of 16 KiB behind ids
    const unsigned long long lower = (1ull << lane) - 1ull;

    int32_t id[kRounds][kLaneTokens];
    uint32_t thr[kRounds][kLaneTokens];
    int rank[kRounds];                                    // survivors of the wave in front of this lane's four tokens
    unsigned keep[kRounds];                               // bit j: the lane's token j of the round survives
    int wave_total = 0;
    const int64_t first = tile * kFilterTile + wave * kWaveTokens + lane * kLaneTokens;
    // every round's ids, then every token's threshold, are in flight before the first decision; slots beyond n hold id -1
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i0 = first + r * kRoundTokens;
        if (aligned && i0 + kLaneTokens <= n) {
            const int4 v = *(const int4 *)(ids + i0);
            id[r][0] = v.x; id[r][1] = v.y; id[r][2] = v.z; id[r][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < kLaneTokens; ++j) id[r][j] = i0 + j < n ? ids[i0 + j] : -1;
        }
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r)
#pragma unroll
        for (int j = 0; j < kLaneTokens; ++j) thr[r][j] = filter_threshold(id[r][j], thresholds, V);
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t x0 = hash_add + (uint64_t)(first + r * kRoundTokens);
        unsigned bits = 0;
        int before = wave_total;
#pragma unroll
        for (int j = 0; j < kLaneTokens; ++j) {           // no branch: the hash costs less than a divergent wave
            const bool k = thr[r][j] == 0xFFFFFFFFu || filter_u(x0 + j) < thr[r][j];
            const unsigned long long b = __ballot(k);
            bits |= (k ? 1u : 0u) << j;
            before += __popcll(b & lower);
            wave_total += __popcll(b);
        }
        keep[r] = bits;
        rank[r] = before;
    }
    if (lane == 0) s_wave[wave] = wave_total;
    __syncthreads();
    int in_front = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) {
        if (wv < wave) in_front += s_wave[wv];
        total += s_wave[wv];
    }
    if (!WRITE) {
        if (tid == 0) tile_count[tile] = total;
        return;
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        int at = in_front + rank[r];
#pragma unroll
        for (int j = 0; j < kLaneTokens; ++j)
            if ((keep[r] >> j) & 1u) s_out[at++] = id[r][j];
    }
    __syncthreads();
    const int64_t off = tile_offset[tile];
    const int64_t room = cap - off;
    if (room <= 0) return;
    store_ids(ids_out + off, room < total ? (int)room : total, s_out);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_cooc_options_abi_version(void) { return GLOVE_COOC_OPTIONS_ABI_VERSION; }

size_t glove_token_filter_workspace_bytes(int64_t n)
{
    if (n < 0 || n > kMaxFilterTokens) return 0;
    return tile_counts_bytes(tiles_of(n, kFilterTile));
}

int glove_token_filter_i32(const int32_t *ids, int64_t n, int64_t pos0, const uint32_t *thresholds, int32_t V, uint64_t seed,
                           int32_t *ids_out, int64_t *n_out, int64_t cap, void *ws, size_t ws_bytes, void *stream)
{
    if (n < 0 || n > kMaxFilterTokens || pos0 < 0 || pos0 > INT64_MAX - n || V <= 0 || cap < 0 || !n_out || !ws)
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIP_TRY(zero_words(n_out, 2, st));
        return 0;
    }
    if (!ids || !thresholds || (cap > 0 && !ids_out)) return GLOVE_E_BADARG;
    // survivors are written while other tiles still read the ids
    const size_t out_bytes = (size_t)cap * 4;
    if (out_bytes && (overlap(ids_out, out_bytes, ids, (size_t)n * 4) || overlap(ids_out, out_bytes, thresholds, (size_t)V * 4) ||
                      overlap(ids_out, out_bytes, n_out, 8)))
        return GLOVE_E_BADARG;
    if (overlap(n_out, 8, ids, (size_t)n * 4) || overlap(n_out, 8, thresholds, (size_t)V * 4)) return GLOVE_E_BADARG;
    WsCarver c{(char *)ws};
    const TileCounts w = carve_tile_counts(c, tiles_of(n, kFilterTile));
    if (c.off > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need;
    if (const int rc = tile_scan_query(w, need, st)) return rc;
    const uint64_t hash_add = (uint64_t)pos0 + (seed + 1ull) * 0x9E3779B97F4A7C15ull;
    const dim3 grid((unsigned int)w.tiles);
    hipLaunchKernelGGL(filter_tiles<false>, grid, dim3(kBlock), 0, st, ids, n, hash_add, thresholds, V, w.count, w.offset, ids_out,
                       n_out, cap);
    HIP_TRY(tile_scan(w, w.prim, need, st));
    hipLaunchKernelGGL(filter_tiles<true>, grid, dim3(kBlock), 0, st, ids, n, hash_add, thresholds, V, w.count, w.offset, ids_out,
                       n_out, cap);
    return (int)hipGetLastError();
}

size_t glove_cooc_finalize_weighted_workspace_bytes(int64_t cap_keys) { return finalize_workspace_bytes(cap_keys); }

int glove_cooc_finalize_weighted(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                                 int32_t context, int64_t min_count, int32_t weighting, int32_t *out_row, int32_t *out_col,
                                 int64_t *out_count, double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws,
                                 size_t ws_bytes, void *stream)
{
    // (a weighting the header does not name is refused there, with the other arguments)
    return finalize_table(keys, counts, n, cap_keys, V, context, min_count, weighting, out_row, out_col, out_count, out_value,
                          out_nnz, cap_out, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
