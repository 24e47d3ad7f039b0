// Kernels and host helpers that libglove_hip.so (the PREDICT path, glove_predict.hip) and libglove_eval_hip.so
// (glove_analogy.hip, glove_cosmul.hip, glove_kmeans.hip) share.  Each library compiles its own copy: kernels are
// shared, state is not (there is none).
//
//   load_row_p / store_row_p / row_sumsq / clamped_inv_norm / clamp_cos   a lane group's view of one row
//   inv_norm_kernel / gathered_inv_norm_kernel   1 / |R_v| per row (tf.math.l2_normalize's clamp)
//   cosine_mfma_kernel   the n x V similarity GEMM on the matrix cores (the tile loop: glove_sim_gemm.h), over where the
//                        query operand comes from
//   topk_select_kernel   staged top-k selection in the order of tf.math.top_k
//   launch_topk_stages   the host loop that runs the selection until one segment is left
//   sim_table_ok / topk_k_ok   the size checks of the entry points
#pragma once
#include "glove_common.h"
#include "glove_sim_gemm.h"

namespace glove {

template <int LPR, int NV>
__device__ inline void load_row_p(f4 (&dst)[NV], const float *table, int32_t id, int d4, int lg)
{
    const f4 *p = reinterpret_cast<const f4 *>(table) + (size_t)id * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        dst[k] = (i4 < d4) ? p[i4] : f4{0.f, 0.f, 0.f, 0.f};
    }
}

// ... and its mirror (lanes beyond the row store nothing)
template <int LPR, int NV>
__device__ inline void store_row_p(float *table, int64_t id, int d4, int lg, const f4 (&src)[NV])
{
    f4 *p = reinterpret_cast<f4 *>(table) + (size_t)id * d4;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i4 = lg + k * LPR;
        if (i4 < d4) p[i4] = src[k];
    }
}

// |r|^2 of the row a lane group holds: one fma chain per lane, one butterfly per group — a fixed summation order
template <int LPR, int NV>
__device__ inline float row_sumsq(const f4 (&r)[NV])
{
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) s += dot4(r[k], r[k]);
    return group_sum<LPR>(s);
}

// 1/sqrt(max(|r|^2, 1e-12))  (tf.math.l2_normalize epsilon)
__device__ inline float clamped_inv_norm(float sumsq) { return 1.0f / sqrtf(fmaxf(sumsq, 1e-12f)); }

__device__ inline float clamp_cos(float c) { return fminf(fmaxf(c, -1.0f), 1.0f); }

// out[v] = clamped_inv_norm of row ids[v] of R (row v itself where ids is null), v < n: one lane group per row
template <int LPR, int NV>
__device__ inline void inv_norm_rows(const float *R, const int32_t *ids, int32_t n, int d4, float *out)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int v = blockIdx.x * GPB + grp; v < n; v += gridDim.x * GPB) {
        f4 r[NV];
        load_row_p<LPR, NV>(r, R, ids ? ids[v] : v, d4, lg);
        const float s = row_sumsq<LPR, NV>(r);
        if (lg == 0) out[v] = clamped_inv_norm(s);
    }
}

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void inv_norm_kernel(const float *__restrict__ R, int32_t V, int d4,
                                                          float *__restrict__ inv_norm)
{
    inv_norm_rows<LPR, NV>(R, nullptr, V, d4, inv_norm);
}

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void gathered_inv_norm_kernel(const float *__restrict__ W, int d4,
                                                                   const int32_t *__restrict__ ids, int32_t n,
                                                                   float *__restrict__ pinv)
{
    inv_norm_rows<LPR, NV>(W, ids, n, d4, pinv);
}

// Where the query operand of the similarity GEMM comes from.
//   GatheredQueries  table rows by id (PREDICT: a token's neighbours); scaled by inv_norm[qid] in the epilogue
//   DenseQueries     rows of a dense [n, d] matrix with their own inverse norms (the analogy queries b - a + c); the
//                    epilogue writes -inf where the vocabulary row is one of the question's own three words
struct GatheredQueries {
    static constexpr bool kDense = false;
    const int32_t *qid;         // [n]
};
struct DenseQueries {
    static constexpr bool kDense = true;
    const float *Q;             // [n, d]
    const float *q_inv;         // [n]
    const int32_t *abc;         // [n, 3] ids never returned for question q
};

// sims[q, v] = (query_q . R[v]) q_inv[q] inv_norm[v]: the one GEMM-shaped piece of the path
// (tf.matmul of the l2-normalised query rows with all rows, utils.py:12-19), on the matrix cores in exact f32.
// Workgroup = 128 queries x 128 vocabulary rows, four waves of 2 x 2 MFMA blocks (64 accumulator VGPRs) through
// sim_tile_gemm.  One call reads R once per 128 queries instead of once per 4.
constexpr int kSimTile = 128;

template <class Src>
__global__ __launch_bounds__(kBlock) void cosine_mfma_kernel(const float *__restrict__ R, int32_t V, int32_t d,
                                                             const Src src, int32_t n,
                                                             const float *__restrict__ inv_norm,
                                                             float *__restrict__ sims /* [n,V] */)
{
    __shared__ float Qs[kSimTile][kSimK + 1];
    __shared__ float Rs[kSimTile][kSimK + 1];
    __shared__ float q_inv[kSimTile];                      // inverse norms of this tile's queries, for the epilogue
    __shared__ int32_t q_excl[Src::kDense ? kSimTile : 1][3];   // dense queries: the three ids a question never returns
    const int v0 = blockIdx.x * kSimTile, q0 = blockIdx.y * kSimTile;
    if constexpr (Src::kDense) {
        if (threadIdx.x < kSimTile) {
            const bool in = q0 + threadIdx.x < n;
            q_inv[threadIdx.x] = in ? src.q_inv[q0 + threadIdx.x] : 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j) q_excl[threadIdx.x][j] = in ? src.abc[(size_t)(q0 + threadIdx.x) * 3 + j] : -1;
        }
    } else {
        if (threadIdx.x < kSimTile) q_inv[threadIdx.x] = q0 + threadIdx.x < n ? inv_norm[src.qid[q0 + threadIdx.x]] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;               // this wave's 64 x 64 quadrant of the tile
    const int r32 = lane & 31, kh = lane >> 5;
    f32x16 acc[2][2];
    const auto q_id = [&](int row) -> int32_t {
        if (q0 + row >= n) return -1;
        if constexpr (Src::kDense) return q0 + row;
        else return src.qid[q0 + row];
    };
    const float *Q = R;
    if constexpr (Src::kDense) Q = src.Q;
    sim_tile_gemm(Qs, Rs, acc, Q, R, d, q_id, [&](int row) { return v0 + row < V ? v0 + row : -1; }, wm * 64, 32, wn * 64);
    // C/D map: column = vocabulary row, row = query
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int v = v0 + wn * 64 + b * 32 + r32;
        const float iv = v < V ? inv_norm[v] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int ql = wm * 64 + a * 32 + sim_cd_row(reg, kh), q = q0 + ql;
                if constexpr (Src::kDense) {
                    // the exclusion rides in the one store of (q, v): no second writer to sims, no ordering question
                    const bool own = v == q_excl[ql][0] || v == q_excl[ql][1] || v == q_excl[ql][2];
                    if (q < n && v < V) sims[(size_t)q * V + v] = own ? -INFINITY : acc[a][b][reg] * q_inv[ql] * iv;
                } else {
                    if (q < n && v < V) sims[(size_t)q * V + v] = acc[a][b][reg] * q_inv[ql] * iv;
                }
            }
        }
    }
}

// What the entry points take for a table: rows of d floats, d a multiple of 4 that some row shape covers
inline bool sim_table_ok(int32_t V, int32_t d) { return V > 0 && d > 0 && (d % 4) == 0 && pick_row_shape(d / 4).lpr != 0; }

// ... and for k, where a query never returns `excluded` ids of its own (3 for an analogy question, 0 for PREDICT):
// k <= V - excluded, so at least k candidates carry a finite score.  The selection (topk_select_kernel) orders a -inf
// score with a valid id behind every finite score and ahead of its empty slots only (id 0x7fffffff, what `none`
// tests): an excluded id can be handed from one stage to the next by a segment with fewer than k finite candidates,
// but the last stage sees all V - excluded >= k finite ones first and never writes it.
inline bool topk_k_ok(int32_t k, int32_t V, int32_t excluded)
{
    return k >= 1 && k <= 1024 && (int64_t)k <= (int64_t)V - excluded;
}

// order of tf.math.top_k: larger similarity first, ties -> lower index first
__device__ inline bool topk_before(float s1, int i1, float s2, int i2) { return s1 > s2 || (s1 == s2 && i1 < i2); }

// Top-k of a query's candidates by selection.  Workgroup = (query, segment of kTopkSeg candidates): every thread
// holds kTopkPer of them in registers and the workgroup runs k rounds of arg-max over the threads' best remaining
// candidates in the order of tf.math.top_k — one barrier per round, nothing sorted and no memory traffic after the
// first load.  A vocabulary larger than one segment is reduced in stages: each launch turns
// `len` candidates per query into ceil(len / kTopkSeg) * k winners (values + vocabulary ids) until one segment is
// left.  (A per-thread sorted list of the best k, the first form of this kernel, cost ~2,300 instructions per
// inserted element and took 9 ms per 256 queries at V = 400 k; this takes 0.1 ms.)
constexpr int kTopkPer = 16;
constexpr int kTopkSeg = kBlock * kTopkPer;

static __global__ __launch_bounds__(kBlock) void topk_select_kernel(const float *__restrict__ vals,
                                                             const int32_t *__restrict__ ids, int64_t row_stride,
                                                             int32_t len, int32_t k, float *__restrict__ out_val,
                                                             int32_t *__restrict__ out_idx)
{
    __shared__ float s_val[2][kBlock / 64];
    __shared__ int s_idx[2][kBlock / 64];
    const float *row = vals + (size_t)blockIdx.x * row_stride;
    const int32_t *row_ids = ids ? ids + (size_t)blockIdx.x * row_stride : nullptr;
    const size_t out_row = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * k;
    float sv[kTopkPer];
    int id[kTopkPer];
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e) {
        const int p = blockIdx.y * kTopkSeg + e * kBlock + threadIdx.x;
        const bool in = p < len;
        const int v = in ? (row_ids ? row_ids[p] : p) : -1;
        sv[e] = (in && v >= 0) ? row[p] : -INFINITY;       // v < 0: an empty slot of a short earlier segment
        id[e] = v >= 0 ? v : 0x7fffffff;
    }
    // every thread keeps its best remaining candidate; a round is one workgroup arg-max over those 256, and only the
    // thread that owned the winner rescans its 16 registers for its next best (the rest of its wave idles through it):
    // ~260 wave-instructions per round instead of ~1,000 when every thread rescanned every round
    float mine = -INFINITY;
    int mine_id = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < kTopkPer; ++e)
        if (topk_before(sv[e], id[e], mine, mine_id)) { mine = sv[e]; mine_id = id[e]; }
    for (int t = 0; t < k; ++t) {
        float best = mine;
        int bi = mine_id;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ob = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (topk_before(ob, oi, best, bi)) { best = ob; bi = oi; }
        }
        const int buf = t & 1;                              // double-buffered: one barrier per round
        if ((threadIdx.x & 63) == 0) { s_val[buf][threadIdx.x >> 6] = best; s_idx[buf][threadIdx.x >> 6] = bi; }
        __syncthreads();
        best = s_val[buf][0];
        bi = s_idx[buf][0];
#pragma unroll
        for (int wv = 1; wv < kBlock / 64; ++wv)
            if (topk_before(s_val[buf][wv], s_idx[buf][wv], best, bi)) { best = s_val[buf][wv]; bi = s_idx[buf][wv]; }
        const bool none = bi == 0x7fffffff;                 // fewer than k candidates in this segment
        if (threadIdx.x == 0) {
            out_val[out_row + t] = none ? -INFINITY : best;
            out_idx[out_row + t] = none ? -1 : bi;
        }
        if (!none && mine_id == bi) {                       // ids are unique: exactly one thread owned the winner
            mine = -INFINITY;
            mine_id = 0x7fffffff;
#pragma unroll
            for (int e = 0; e < kTopkPer; ++e) {
                const bool behind = sv[e] < best || (sv[e] == best && id[e] > bi);
                if (behind && topk_before(sv[e], id[e], mine, mine_id)) { mine = sv[e]; mine_id = id[e]; }
            }
        }
    }
}

// winners the first top-k stage leaves per query (the later stages only shrink)
inline size_t topk_stage_items(int32_t V, int32_t k) { return (size_t)((V + kTopkSeg - 1) / kTopkSeg) * (size_t)k; }

// bytes of the two ping-pong buffers of winners (values + ids) behind the similarity matrix
inline size_t topk_pingpong_bytes(int32_t n, int32_t V, int32_t k)
{
    const size_t cand = (size_t)n * topk_stage_items(V, k);
    return 2 * (align_up(cand * sizeof(float), 256) + align_up(cand * sizeof(int32_t), 256));
}

// Top k of each of the n rows of sims [n, V] into sims_out / idx_out [n, k]: reduce in stages until one segment holds a
// query's candidates; the last stage writes the outputs.  `pingpong`: topk_pingpong_bytes(n, V, k) bytes.
inline void launch_topk_stages(const float *sims, int32_t n, int32_t V, int32_t k, float *sims_out, int32_t *idx_out,
                               void *pingpong, hipStream_t st)
{
    const size_t cand = (size_t)n * topk_stage_items(V, k);
    char *pp = (char *)pingpong;
    float *cv[2];
    int32_t *ci[2];
    for (int b = 0; b < 2; ++b) {
        cv[b] = (float *)pp;
        pp += align_up(cand * sizeof(float), 256);
        ci[b] = (int32_t *)pp;
        pp += align_up(cand * sizeof(int32_t), 256);
    }
    const float *src_v = sims;
    const int32_t *src_i = nullptr;
    int64_t stride = V;
    int32_t len = V;
    for (int stage = 0;; ++stage) {
        const int nseg = (len + kTopkSeg - 1) / kTopkSeg;
        const bool last = nseg == 1;
        float *dv = last ? sims_out : cv[stage & 1];
        int32_t *di = last ? idx_out : ci[stage & 1];
        hipLaunchKernelGGL(topk_select_kernel, dim3(n, nseg), dim3(kBlock), 0, st, src_v, src_i, stride, len, k, dv, di);
        if (last) break;
        src_v = dv;
        src_i = di;
        stride = len = nseg * k;
    }
}

}  // namespace glove
