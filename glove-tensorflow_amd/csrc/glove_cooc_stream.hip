// Co-occurrence counting of a corpus of any length on gfx950 (include/glove_cooc_stream_hip.h, libglove_prep_hip.so).
//
// glove_cooc.hip counts a whole corpus in one call: 52 B of workspace per key slot, 2 context n slots.  Here the corpus
// arrives in chunks.  A chunk's keys are made, sorted and run-length encoded as there; the running state is one sorted
// table of (key, int64 count); a merge-path merge folds every chunk into it; the (row, col, count, value) table is made
// from the state at the end, by the expression and in the order of cooc_aggregate.  The state holds integers only, so the
// result is bit for bit that of the one-shot call however the corpus was cut.
//
// The merge is the part that runs once per chunk over the whole state.  It streams 16 B per entry in and out:
//   merge_partition   one thread per tile boundary: binary search on the boundary's diagonal (ties to A), then the twin rule;
//   merge_tiles<0>    one workgroup per tile: keys into LDS, 8 merged positions per thread, the tile's number of outputs;
//   rocPRIM scan      of the tile counts;
//   merge_tiles<1>    the same walk with the counts beside the keys; outputs go to LDS at their rank and leave in 16-B stores.
#include "glove_common.h"
#include "glove_merge_path.h"
#include "glove_cooc_finalize.h"
#include "../../include/glove_cooc_stream_hip.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

namespace glove {

// ---- chunk keys ------------------------------------------------------------------------------------------------------
// slot layout of glove_cooc.hip: own position p has 2 context slots; partners may lie in the halo
__global__ void chunk_emit_keys(const int32_t *__restrict__ tok, int64_t n_own, int64_t n_total, int32_t V, int32_t context,
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

// the run-length encoded keys without the sentinel run, counts widened to int64, cut at cap
__global__ void chunk_copy_out(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ ucounts,
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

struct ChunkWs {
    uint64_t *keys, *keys_sorted, *ukeys;
    uint32_t *ucounts;
    int64_t *n_unique;
    void *prim;
    size_t prim_bytes, bytes;
};

// the pieces of glove_cooc.hip's carve_cooc_ws, byte for byte (the two flag arrays of its aggregation go unused here)
static ChunkWs carve_chunk_ws(void *ws, int64_t n, int32_t context)
{
    ChunkWs w;
    size_t off = 0;
    char *base = (char *)ws;
    auto take = [&](size_t bytes) { void *q = base + off; off += align_up(bytes, 256); return q; };
    const size_t slots = (size_t)(n > 0 ? n : 1) * context * 2;
    w.keys = (uint64_t *)take(slots * 8);
    w.keys_sorted = (uint64_t *)take(slots * 8);
    w.ukeys = w.keys;                       // the unsorted keys are dead once sorted
    w.ucounts = (uint32_t *)take(slots * 4);
    take(slots * 8);
    take(slots * 8);
    w.n_unique = (int64_t *)take(256);
    w.prim_bytes = (size_t)(16u << 20) + slots * 16;
    w.prim = take(w.prim_bytes);
    w.bytes = off;
    return w;
}

// ---- merge -----------------------------------------------------------------------------------------------------------
constexpr int kTile = GLOVE_COOC_MERGE_TILE;      // merged positions per workgroup
constexpr int kVT = kTile / kBlock;               // ... per thread
static_assert(kVT * kBlock == kTile && kVT == 8, "a thread walks 8 merged positions");

// split_a[t], split_b[t]: where tile t starts in A and in B.  Each input is duplicate-free, so a run of equal keys in the
// merged order is one A entry followed by its B twin: a split that would fall between them moves one B entry forward.
__global__ void merge_partition(const uint64_t *__restrict__ keys_a, const int64_t *__restrict__ n_a, int64_t cap_a,
                                const uint64_t *__restrict__ keys_b, const int64_t *__restrict__ n_b, int64_t cap_b,
                                int64_t tiles, int64_t *__restrict__ split_a, int64_t *__restrict__ split_b)
{
    const int64_t na = clamp_count(n_a, cap_a), nb = clamp_count(n_b, cap_b), L = na + nb;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= tiles; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t diag = t * kTile < L ? t * kTile : L;
        const int64_t ai = merge_path<int64_t>(keys_a, na, keys_b, nb, diag);
        int64_t bi = diag - ai;
        if (ai > 0 && bi < nb && keys_a[ai - 1] == keys_b[bi]) ++bi;
        split_a[t] = ai;
        split_b[t] = bi;
    }
}

// WRITE = false: count[tile] = the tile's number of output entries.  WRITE = true: the entries, at offset[tile].
// A tile holds at most kTile + 1 input entries (its start and its end may each have moved one B entry forward), a
// thread's stretch at most kVT + 1, for the same reason.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void merge_tiles(
    const uint64_t *__restrict__ keys_a, const int64_t *__restrict__ counts_a, const int64_t *__restrict__ n_a, int64_t cap_a,
    const uint64_t *__restrict__ keys_b, const int64_t *__restrict__ counts_b, const int64_t *__restrict__ n_b, int64_t cap_b,
    const int64_t *__restrict__ split_a, const int64_t *__restrict__ split_b, int64_t *__restrict__ tile_count,
    const int64_t *__restrict__ tile_offset, uint64_t *__restrict__ keys_out, int64_t *__restrict__ counts_out,
    int64_t *__restrict__ n_out, int64_t cap_out)
{
    __shared__ __attribute__((aligned(16))) uint64_t sk[kTile + 2];
    __shared__ __attribute__((aligned(16))) uint64_t sc[WRITE ? kTile + 2 : 2];
    __shared__ int s_ai[kBlock + 1], s_bi[kBlock + 1];
    __shared__ int s_wave[kBlock / 64];

    const int64_t L = clamp_count(n_a, cap_a) + clamp_count(n_b, cap_b);
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    if (WRITE && tile == (int64_t)gridDim.x - 1 && tid == 0) *n_out = tile_offset[tile] + tile_count[tile];
    if (tile * kTile >= L) {              // beyond the merged length
        if (!WRITE && tid == 0) tile_count[tile] = 0;
        return;
    }
    const int64_t a0 = split_a[tile], b0 = split_b[tile];
    const int nat = (int)(split_a[tile + 1] - a0), nbt = (int)(split_b[tile + 1] - b0), nt = nat + nbt;
    load_words(keys_a + a0, nat, sk);
    load_words(keys_b + b0, nbt, sk + nat);
    if (WRITE) {
        load_words((const uint64_t *)(counts_a + a0), nat, sc);
        load_words((const uint64_t *)(counts_b + b0), nbt, sc + nat);
    }
    __syncthreads();

    const uint64_t *A = sk, *B = sk + nat;
    {
        const int d = tid * kVT < nt ? tid * kVT : nt;
        const int ai = merge_path<int>(A, nat, B, nbt, d);
        int bi = d - ai;
        if (ai > 0 && bi < nbt && A[ai - 1] == B[bi]) ++bi;
        s_ai[tid] = ai;
        s_bi[tid] = bi;
        if (tid == 0) { s_ai[kBlock] = nat; s_bi[kBlock] = nbt; }
    }
    __syncthreads();
    int i = s_ai[tid], j = s_bi[tid];
    const int ie = s_ai[tid + 1], je = s_bi[tid + 1];

    // the thread's stretch: an A entry takes its B twin with it; a B entry reached on its own has none
    uint64_t ok[kVT + 1];
    int64_t oc[kVT + 1];
    int mine = 0;
#pragma unroll
    for (int s = 0; s < kVT + 1; ++s) {
        const bool live = i < ie || j < je;
        const bool has_a = i < ie, has_b = j < je;
        const uint64_t ka = has_a ? A[i] : kNoKey, kb = has_b ? B[j] : kNoKey;
        const bool take_a = has_a && (!has_b || ka <= kb);
        const bool twin = take_a && has_b && ka == kb;
        if (WRITE) {
            const int64_t ca = has_a ? (int64_t)sc[i] : 0, cb = has_b ? (int64_t)sc[nat + j] : 0;
            ok[s] = take_a ? ka : kb;
            oc[s] = take_a ? (twin ? ca + cb : ca) : cb;
        }
        if (live) {
            ++mine;
            if (take_a) { ++i; if (twin) ++j; } else ++j;
        }
    }

    // block-wide exclusive scan of `mine` (wave scan, then the four wave totals)
    const int lane = tid & 63, wave = tid >> 6;
    int incl = mine;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const int up = __shfl_up(incl, dlt, 64);
        if (lane >= dlt) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();                      // also: every thread is done reading sk / sc
    int before = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < kBlock / 64; ++wv) {
        if (wv < wave) before += s_wave[wv];
        total += s_wave[wv];
    }
    if (!WRITE) {
        if (tid == 0) tile_count[tile] = total;
        return;
    }
    const int rank = before + incl - mine;
#pragma unroll
    for (int s = 0; s < kVT + 1; ++s) {
        if (s < mine) {
            sk[rank + s] = ok[s];
            sc[rank + s] = (uint64_t)oc[s];
        }
    }
    __syncthreads();
    const int64_t off = tile_offset[tile];
    int64_t room = cap_out - off;
    if (room <= 0) return;
    const int n = room < total ? (int)room : total;
    store_words(keys_out + off, n, sk);
    store_words((uint64_t *)(counts_out + off), n, sc);
}

struct MergeWs {
    int64_t *split_a, *split_b, *count, *offset;
    void *prim;
    size_t prim_bytes, bytes;
    int64_t tiles;
};

static MergeWs carve_merge_ws(void *ws, int64_t cap_a, int64_t cap_b)
{
    MergeWs w;
    size_t off = 0;
    char *base = (char *)ws;
    auto take = [&](size_t bytes) { void *q = base + off; off += align_up(bytes, 256); return q; };
    w.tiles = (cap_a + cap_b + kTile - 1) / kTile;
    if (w.tiles < 1) w.tiles = 1;
    w.split_a = (int64_t *)take((size_t)(w.tiles + 1) * 8);
    w.split_b = (int64_t *)take((size_t)(w.tiles + 1) * 8);
    w.count = (int64_t *)take((size_t)w.tiles * 8);
    w.offset = (int64_t *)take((size_t)w.tiles * 8);
    w.prim_bytes = (size_t)(64u << 10) + (size_t)w.tiles * 8;
    w.prim = take(w.prim_bytes);
    w.bytes = off;
    return w;
}

// ---- finalize --------------------------------------------------------------------------------------------------------
// (the head rule, the pair's sums and the workspace are glove_cooc_finalize.h's: glove_cooc_options.hip weights them otherwise)
__global__ void finalize_mark(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts,
                              const int64_t *__restrict__ n, int64_t cap_keys, int32_t context, int64_t min_count,
                              int64_t *__restrict__ flag)
{
    const int64_t m = clamp_count(n, cap_keys);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        flag[i] = finalize_head_flag(keys, counts, m, i, context, min_count);
}

// incl = the inclusive scan of flag: entry i is a written head where flag is set, at output position incl[i] - 1
__global__ void finalize_aggregate(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts,
                                   const int64_t *__restrict__ n, int64_t cap_keys, const int64_t *__restrict__ flag,
                                   const int64_t *__restrict__ incl,
                                   int32_t V, int32_t context, int64_t cap, int32_t *__restrict__ out_row,
                                   int32_t *__restrict__ out_col, int64_t *__restrict__ out_count,
                                   double *__restrict__ out_value, int64_t *__restrict__ out_nnz)
{
    const int64_t m = clamp_count(n, cap_keys);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        if (!flag[i]) continue;
        const uint64_t ab = keys[i] / context;
        int64_t cnt;
        double val;
        finalize_pair<kWindowHarmonic>(keys, counts, m, i, context, cnt, val);
        const int64_t o = incl[i] - 1;
        if (o < cap) {
            out_row[o] = (int32_t)(ab / V);
            out_col[o] = (int32_t)(ab % V);
            out_count[o] = cnt;
            out_value[o] = val;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_nnz = m > 0 ? incl[m - 1] : 0;
}

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

}  // namespace glove

using namespace glove;

extern "C" {

int glove_cooc_stream_abi_version(void) { return GLOVE_COOC_STREAM_ABI_VERSION; }

size_t glove_cooc_chunk_workspace_bytes(int64_t n_total, int32_t context)
{
    if (n_total < 0 || context <= 0 || context > 255) return 0;
    if ((double)n_total * context * 2 > 4294967295.0) return 0;
    return carve_chunk_ws(nullptr, n_total, context).bytes;
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
    const ChunkWs w = carve_chunk_ws(ws, n_total, context);
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

size_t glove_cooc_merge_workspace_bytes(int64_t cap_a, int64_t cap_b)
{
    if (cap_a < 0 || cap_b < 0 || cap_a > kMaxStateCap || cap_b > kMaxStateCap || cap_a + cap_b > kMaxStateCap) return 0;
    return carve_merge_ws(nullptr, cap_a, cap_b).bytes;
}

int glove_cooc_merge_u64(const uint64_t *keys_a, const int64_t *counts_a, const int64_t *n_a, int64_t cap_a,
                         const uint64_t *keys_b, const int64_t *counts_b, const int64_t *n_b, int64_t cap_b,
                         uint64_t *keys_out, int64_t *counts_out, int64_t *n_out, int64_t cap_out, void *ws, size_t ws_bytes,
                         void *stream)
{
    if (cap_a < 0 || cap_b < 0 || cap_out < 0 || cap_a > kMaxStateCap || cap_b > kMaxStateCap ||
        cap_a + cap_b > kMaxStateCap || !n_a || !n_b || !n_out || !ws)
        return GLOVE_E_BADARG;
    if ((cap_a > 0 && (!keys_a || !counts_a)) || (cap_b > 0 && (!keys_b || !counts_b)) ||
        (cap_out > 0 && (!keys_out || !counts_out)))
        return GLOVE_E_BADARG;
    // the outputs are written while other tiles still read the inputs
    const struct { const void *p; size_t n; } ins[] = {{keys_a, (size_t)cap_a * 8}, {counts_a, (size_t)cap_a * 8},
                                                       {keys_b, (size_t)cap_b * 8}, {counts_b, (size_t)cap_b * 8},
                                                       {n_a, 8}, {n_b, 8}},
                                              outs[] = {{keys_out, (size_t)cap_out * 8}, {counts_out, (size_t)cap_out * 8},
                                                        {n_out, 8}};
    for (const auto &o : outs)
        for (const auto &i : ins)
            if (o.n && i.n && overlap(o.p, o.n, i.p, i.n)) return GLOVE_E_BADARG;
    if ((cap_out > 0 && overlap(keys_out, (size_t)cap_out * 8, counts_out, (size_t)cap_out * 8)) ||
        overlap(n_out, 8, keys_out, (size_t)cap_out * 8) || overlap(n_out, 8, counts_out, (size_t)cap_out * 8))
        return GLOVE_E_BADARG;
    const MergeWs w = carve_merge_ws(ws, cap_a, cap_b);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    size_t need = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, need, w.count, w.offset, (int64_t)0, (size_t)w.tiles, rocprim::plus<int64_t>(), st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    hipLaunchKernelGGL(merge_partition, dim3(blocks_for(w.tiles + 1, kBlock)), dim3(kBlock), 0, st, keys_a, n_a, cap_a, keys_b,
                       n_b, cap_b, w.tiles, w.split_a, w.split_b);
    const dim3 grid((unsigned int)w.tiles);
    hipLaunchKernelGGL(merge_tiles<false>, grid, dim3(kBlock), 0, st, keys_a, counts_a, n_a, cap_a, keys_b, counts_b, n_b,
                       cap_b, w.split_a, w.split_b, w.count, w.offset, keys_out, counts_out, n_out, cap_out);
    HIP_TRY(rocprim::exclusive_scan(w.prim, need, w.count, w.offset, (int64_t)0, (size_t)w.tiles, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(merge_tiles<true>, grid, dim3(kBlock), 0, st, keys_a, counts_a, n_a, cap_a, keys_b, counts_b, n_b,
                       cap_b, w.split_a, w.split_b, w.count, w.offset, keys_out, counts_out, n_out, cap_out);
    return (int)hipGetLastError();
}

size_t glove_cooc_finalize_workspace_bytes(int64_t cap_keys)
{
    if (cap_keys < 0 || cap_keys > kMaxStateCap) return 0;
    return carve_finalize_ws(nullptr, cap_keys).bytes;
}

int glove_cooc_finalize(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V,
                        int32_t context, int64_t min_count, int32_t *out_row, int32_t *out_col, int64_t *out_count,
                        double *out_value, int64_t *out_nnz, int64_t cap_out, void *ws, size_t ws_bytes, void *stream)
{
    if (finalize_bad_args(keys, counts, n, cap_keys, V, context, out_row, out_col, out_count, out_value, out_nnz, cap_out, ws))
        return GLOVE_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cap_keys == 0) {
        HIP_TRY(zero_words(out_nnz, 2, st));
        return 0;
    }
    const FinalizeWs w = carve_finalize_ws(ws, cap_keys);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, need, w.flag, w.incl, (size_t)cap_keys, rocprim::plus<int64_t>(), st));
    if (need > w.prim_bytes) return GLOVE_E_WORKSPACE;
    const int nb = blocks_for(cap_keys, kBlock);
    hipLaunchKernelGGL(finalize_mark, dim3(nb), dim3(kBlock), 0, st, keys, counts, n, cap_keys, context, min_count, w.flag);
    // entries past *n are stale but never read: finalize_aggregate stops at *n
    HIP_TRY(rocprim::inclusive_scan(w.prim, need, w.flag, w.incl, (size_t)cap_keys, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(finalize_aggregate, dim3(nb), dim3(kBlock), 0, st, keys, counts, n, cap_keys, w.flag, w.incl, V, context, cap_out,
                       out_row, out_col, out_count, out_value, out_nnz);
    return (int)hipGetLastError();
}

}  // extern "C"
