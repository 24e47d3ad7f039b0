// The operations on a sorted (key, payload) table that several entry points of libglove_prep_hip.so run (glove_table_ops.h):
// the merge-path merge of glove_cooc_merge_u64 and glove_text_vocab_merge, and the finalisation of glove_cooc_finalize and
// glove_cooc_finalize_weighted.  Every kernel here is compiled into this object alone.
//
// The merge is what runs once per chunk over the whole state.  It streams 8 (1 + NPAY) B per entry in and out:
//   merge_partition   one thread per tile boundary: binary search on the boundary's diagonal (ties to A), then the twin rule;
//   merge_tiles<0>    one workgroup per tile: keys into LDS, 8 merged positions per thread, the tile's number of outputs;
//   rocPRIM scan      of the tile counts;
//   merge_tiles<1>    the same walk with the payloads beside the keys; outputs go to LDS at their rank and leave in 16-B stores.
#include "glove_common.h"
#include "glove_table_ops.h"
#include "../../include/glove_cooc_stream_hip.h"

namespace glove {

constexpr int64_t kMaxStateCap = (int64_t)1 << 40;

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
// NPAY payload words ride beside a key; where A and B hold the same key, payload 0 adds and payload 1 keeps the smaller.
// A tile holds at most kTile + 1 input entries (its start and its end may each have moved one B entry forward), a
// thread's stretch at most kVT + 1, for the same reason.
template <bool WRITE, int NPAY>
__global__ __launch_bounds__(kBlock) void merge_tiles(MergeIn a, MergeIn b, const int64_t *__restrict__ split_a,
                                                      const int64_t *__restrict__ split_b, int64_t *__restrict__ tile_count,
                                                      const int64_t *__restrict__ tile_offset, uint64_t *__restrict__ keys_out,
                                                      int64_t *__restrict__ pay_out0, int64_t *__restrict__ pay_out1,
                                                      int64_t *__restrict__ n_out, int64_t cap_out)
{
    // (the outputs as __restrict__ parameters, not as a MergeOut: only then does the compiler know that the store to *n_out
    // leaves the inputs alone, and keep load_words' single-word loads of the tile's ends scalar)
    static_assert(NPAY >= 1 && NPAY <= kMaxPayloads, "payload 0 adds, payload 1 takes the minimum");
    __shared__ __attribute__((aligned(16))) uint64_t sk[kTile + 2];
    __shared__ __attribute__((aligned(16))) uint64_t sp[NPAY][WRITE ? kTile + 2 : 2];
    __shared__ int s_ai[kBlock + 1], s_bi[kBlock + 1];
    __shared__ int s_wave[kBlock / 64];

    const int64_t L = clamp_count(a.n, a.cap) + clamp_count(b.n, b.cap);
    const int64_t tile = blockIdx.x;
    const int tid = threadIdx.x;
    if (WRITE && tile == (int64_t)gridDim.x - 1 && tid == 0) *n_out = tile_offset[tile] + tile_count[tile];
    if (tile * kTile >= L) {              // beyond the merged length
        if (!WRITE && tid == 0) tile_count[tile] = 0;
        return;
    }
    const int64_t a0 = split_a[tile], b0 = split_b[tile];
    const int nat = (int)(split_a[tile + 1] - a0), nbt = (int)(split_b[tile + 1] - b0), nt = nat + nbt;
    load_words(a.keys + a0, nat, sk);
    load_words(b.keys + b0, nbt, sk + nat);
    if (WRITE) {
#pragma unroll
        for (int p = 0; p < NPAY; ++p) {
            load_words((const uint64_t *)(a.pay[p] + a0), nat, sp[p]);
            load_words((const uint64_t *)(b.pay[p] + b0), nbt, sp[p] + nat);
        }
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
    int64_t op[NPAY][kVT + 1];
    int mine = 0;
#pragma unroll
    for (int s = 0; s < kVT + 1; ++s) {
        const bool live = i < ie || j < je;
        const bool has_a = i < ie, has_b = j < je;
        const uint64_t ka = has_a ? A[i] : kNoKey, kb = has_b ? B[j] : kNoKey;
        const bool take_a = has_a && (!has_b || ka <= kb);
        const bool twin = take_a && has_b && ka == kb;
        if (WRITE) {
            // Straight-line, the step's LDS reads in front of its results.  (A loop over the payloads here, however it was
            // spelled, cost merge_tiles<true, 2> 35 more VGPRs: profiles/r13_prep_table_ops_resource_usage.txt.)
            const int64_t ca = has_a ? (int64_t)sp[0][i] : 0, cb = has_b ? (int64_t)sp[0][nat + j] : 0;
            int64_t wa = 0, wb = 0;
            if constexpr (NPAY > 1) {
                wa = has_a ? (int64_t)sp[1][i] : 0;
                wb = has_b ? (int64_t)sp[1][nat + j] : 0;
            }
            ok[s] = take_a ? ka : kb;
            op[0][s] = take_a ? (twin ? ca + cb : ca) : cb;
            if constexpr (NPAY > 1) op[1][s] = take_a ? (twin && wb < wa ? wb : wa) : wb;
        }
        if (live) {
            ++mine;
            if (take_a) { ++i; if (twin) ++j; } else ++j;
        }
    }

    int before, total;
    block_exclusive_scan(mine, s_wave, before, total);      // its barrier: every thread is done reading sk / sp
    if (!WRITE) {
        if (tid == 0) tile_count[tile] = total;
        return;
    }
#pragma unroll
    for (int s = 0; s < kVT + 1; ++s) {
        if (s < mine) {
            sk[before + s] = ok[s];
#pragma unroll
            for (int p = 0; p < NPAY; ++p) sp[p][before + s] = (uint64_t)op[p][s];
        }
    }
    __syncthreads();
    const int64_t off = tile_offset[tile];
    const int64_t room = cap_out - off;
    if (room <= 0) return;
    const int n = room < total ? (int)room : total;
    store_words(keys_out + off, n, sk);
    store_words((uint64_t *)(pay_out0 + off), n, sp[0]);
    if constexpr (NPAY > 1) store_words((uint64_t *)(pay_out1 + off), n, sp[1]);
}

// split_a[tiles + 1] | split_b[tiles + 1] | the tile counts
struct MergeWs {
    int64_t *split_a, *split_b;
    TileCounts t;
    size_t bytes;
};

static MergeWs carve_merge_ws(void *ws, int64_t cap_a, int64_t cap_b)
{
    MergeWs w;
    WsCarver c{(char *)ws};
    const int64_t tiles = tiles_of(cap_a + cap_b, kTile);
    w.split_a = c.take<int64_t>((size_t)tiles + 1);
    w.split_b = c.take<int64_t>((size_t)tiles + 1);
    w.t = carve_tile_counts(c, tiles);
    w.bytes = c.off;
    return w;
}

static bool bad_merge_caps(int64_t cap_a, int64_t cap_b)
{
    return cap_a < 0 || cap_b < 0 || cap_a > kMaxStateCap || cap_b > kMaxStateCap || cap_a + cap_b > kMaxStateCap;
}

struct Range { const void *p; size_t n; };

// does an output overlap an input or another output?  (empty ranges overlap nothing)
template <size_t NO, size_t NI>
static bool outputs_alias(const Range (&outs)[NO], const Range (&ins)[NI])
{
    for (size_t o = 0; o < NO; ++o) {
        if (!outs[o].n) continue;
        for (size_t i = 0; i < NI; ++i)
            if (ins[i].n && overlap(outs[o].p, outs[o].n, ins[i].p, ins[i].n)) return true;
        for (size_t q = o + 1; q < NO; ++q)
            if (outs[q].n && overlap(outs[o].p, outs[o].n, outs[q].p, outs[q].n)) return true;
    }
    return false;
}

template <int NPAY>
static int launch_merge(const MergeIn &a, const MergeIn &b, const MergeOut &out, const MergeWs &w, size_t need, hipStream_t st)
{
    hipLaunchKernelGGL(merge_partition, dim3(blocks_for(w.t.tiles + 1, kBlock)), dim3(kBlock), 0, st, a.keys, a.n, a.cap, b.keys,
                       b.n, b.cap, w.t.tiles, w.split_a, w.split_b);
    const dim3 grid((unsigned int)w.t.tiles);
    hipLaunchKernelGGL((merge_tiles<false, NPAY>), grid, dim3(kBlock), 0, st, a, b, w.split_a, w.split_b, w.t.count, w.t.offset,
                       out.keys, out.pay[0], out.pay[1], out.n, out.cap);
    HIP_TRY(tile_scan(w.t, w.t.prim, need, st));
    hipLaunchKernelGGL((merge_tiles<true, NPAY>), grid, dim3(kBlock), 0, st, a, b, w.split_a, w.split_b, w.t.count, w.t.offset,
                       out.keys, out.pay[0], out.pay[1], out.n, out.cap);
    return (int)hipGetLastError();
}

size_t merge_workspace_bytes(int64_t cap_a, int64_t cap_b)
{
    return bad_merge_caps(cap_a, cap_b) ? 0 : carve_merge_ws(nullptr, cap_a, cap_b).bytes;
}

int merge_tables(const MergeIn &a, const MergeIn &b, const MergeOut &out, int npay, void *ws, size_t ws_bytes, hipStream_t st)
{
    if (npay < 1 || npay > kMaxPayloads || bad_merge_caps(a.cap, b.cap) || out.cap < 0 || !a.n || !b.n || !out.n || !ws)
        return GLOVE_E_BADARG;
    // the outputs are written while other tiles still read the inputs; a payload the tables do not carry is an empty range
    const size_t ba = (size_t)a.cap * 8, bb = (size_t)b.cap * 8, bo = (size_t)out.cap * 8;
    Range ins[2 + 2 * (1 + kMaxPayloads)] = {{a.n, 8}, {b.n, 8}, {a.keys, ba}, {b.keys, bb}};
    Range outs[2 + kMaxPayloads] = {{out.n, 8}, {out.keys, bo}};
    bool missing = (ba && !a.keys) || (bb && !b.keys) || (bo && !out.keys);
    for (int p = 0; p < npay; ++p) {
        missing = missing || (ba && !a.pay[p]) || (bb && !b.pay[p]) || (bo && !out.pay[p]);
        ins[4 + 2 * p] = {a.pay[p], ba};
        ins[5 + 2 * p] = {b.pay[p], bb};
        outs[2 + p] = {out.pay[p], bo};
    }
    if (missing || outputs_alias(outs, ins)) return GLOVE_E_BADARG;
    const MergeWs w = carve_merge_ws(ws, a.cap, b.cap);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    size_t need;
    if (const int rc = tile_scan_query(w.t, need, st)) return rc;
    return npay == 1 ? launch_merge<1>(a, b, out, w, need, st) : launch_merge<2>(a, b, out, w, need, st);
}

// ---- finalize --------------------------------------------------------------------------------------------------------
// flag of entry i: 1 where a new (a, b) starts whose count reaches min_count (at most `context` keys share one (a, b))
__global__ void finalize_mark(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts,
                              const int64_t *__restrict__ n, int64_t cap_keys, int32_t context, int64_t min_count,
                              int64_t *__restrict__ flag)
{
    const int64_t m = clamp_count(n, cap_keys);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t ab = keys[i] / context;
        int64_t head = 0;
        if (i == 0 || keys[i - 1] / context != ab) {
            int64_t cnt = 0;
            for (int64_t j = i; j < m && j < i + context && keys[j] / context == ab; ++j) cnt += counts[j];
            head = cnt >= min_count ? 1 : 0;
        }
        flag[i] = head;
    }
}

// incl = the inclusive scan of flag: entry i is a written head where flag is set, at output position incl[i] - 1.
// count and value of the (a, b) that starts there.  HARMONIC: sum_k (double)n_k / (double)k, k ascending from 0.0 (the
// expression and order of cooc_aggregate in glove_cooc.hip); UNIFORM and DYNAMIC sum integers and convert once.
template <int WEIGHTING>
__global__ void finalize_aggregate(const uint64_t *__restrict__ keys, const int64_t *__restrict__ counts,
                                   const int64_t *__restrict__ n, int64_t cap_keys, const int64_t *__restrict__ flag,
                                   const int64_t *__restrict__ incl, int32_t V, int32_t context, int64_t cap,
                                   int32_t *__restrict__ out_row, int32_t *__restrict__ out_col,
                                   int64_t *__restrict__ out_count, double *__restrict__ out_value,
                                   int64_t *__restrict__ out_nnz)
{
    const int64_t m = clamp_count(n, cap_keys);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        if (!flag[i]) continue;
        const uint64_t ab = keys[i] / context;
        int64_t cnt = 0, weighted = 0;
        double val = 0.0;
        for (int64_t j = i; j < m && j < i + context; ++j) {
            const uint64_t key = keys[j];
            if (key / context != ab) break;
            const int k = (int)(key % context) + 1;
            cnt += counts[j];
            if (WEIGHTING == kWindowHarmonic) val += (double)counts[j] / (double)k;
            if (WEIGHTING == kWindowDynamic) weighted += counts[j] * (int64_t)(context - k + 1);
        }
        if (WEIGHTING == kWindowUniform) val = (double)cnt;
        if (WEIGHTING == kWindowDynamic) val = (double)weighted / (double)context;
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

struct FinalizeWs {
    int64_t *flag, *incl;
    void *prim;
    size_t prim_bytes, bytes;
};

static FinalizeWs carve_finalize_ws(void *ws, int64_t cap_keys)
{
    FinalizeWs w;
    WsCarver c{(char *)ws};
    const size_t n = (size_t)(cap_keys > 0 ? cap_keys : 1);
    w.flag = c.take<int64_t>(n);
    w.incl = c.take<int64_t>(n);
    w.prim_bytes = (size_t)(1u << 20) + n / 16;
    w.prim = c.take<char>(w.prim_bytes);
    w.bytes = c.off;
    return w;
}

size_t finalize_workspace_bytes(int64_t cap_keys)
{
    return cap_keys < 0 || cap_keys > kMaxStateCap ? 0 : carve_finalize_ws(nullptr, cap_keys).bytes;
}

int finalize_table(const uint64_t *keys, const int64_t *counts, const int64_t *n, int64_t cap_keys, int32_t V, int32_t context,
                   int64_t min_count, int weighting, int32_t *out_row, int32_t *out_col, int64_t *out_count, double *out_value,
                   int64_t *out_nnz, int64_t cap_out, void *ws, size_t ws_bytes, hipStream_t st)
{
    if (cap_keys < 0 || cap_keys > kMaxStateCap || bad_key_shape(V, context) || cap_out < 0 || !n || !out_nnz || !ws)
        return GLOVE_E_BADARG;
    if (weighting != kWindowHarmonic && weighting != kWindowUniform && weighting != kWindowDynamic) return GLOVE_E_BADARG;
    if ((cap_keys > 0 && (!keys || !counts)) || (cap_out > 0 && (!out_row || !out_col || !out_count || !out_value)))
        return GLOVE_E_BADARG;
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
    // entries past *n are stale but never read: the aggregation stops at *n
    HIP_TRY(rocprim::inclusive_scan(w.prim, need, w.flag, w.incl, (size_t)cap_keys, rocprim::plus<int64_t>(), st));
#define GLOVE_AGGREGATE(W)                                                                                                      \
    hipLaunchKernelGGL(finalize_aggregate<W>, dim3(nb), dim3(kBlock), 0, st, keys, counts, n, cap_keys, w.flag, w.incl, V, context, \
                       cap_out, out_row, out_col, out_count, out_value, out_nnz)
    if (weighting == kWindowHarmonic) GLOVE_AGGREGATE(kWindowHarmonic);
    else if (weighting == kWindowUniform) GLOVE_AGGREGATE(kWindowUniform);
    else GLOVE_AGGREGATE(kWindowDynamic);
#undef GLOVE_AGGREGATE
    return (int)hipGetLastError();
}

}  // namespace glove
