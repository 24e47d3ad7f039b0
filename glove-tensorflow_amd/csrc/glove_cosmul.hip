// 3CosMul word analogies and the cosine of word pairs on gfx950: the second object of libglove_eval_hip.so,
// include/glove_eval_sim_hip.h.
//
//   glove_cosmul_topk_f32    for questions a : b :: c : ?, the k vocabulary rows with the largest
//                            s(b, v) s(c, v) / (s(a, v) + eps), s = (1 + cos) / 2, the question's own three words left
//                            out (Levy & Goldberg 2014, gensim most_similar_cosmul).
//   glove_pair_cosine_f32    the cosine of pairs of rows (word-similarity datasets, gensim evaluate_word_pairs).
//
// Three pieces on one stream: inverse row norms, the similarity GEMM whose epilogue combines the three cosines of a
// (question, v) pair, and the staged top-k selection, the first and the last shared with glove_predict.hip and
// glove_analogy.hip through glove_topk_kernels.h, the GEMM's tile loop through glove_sim_gemm.h.
#include "glove_common.h"
#include "glove_topk_kernels.h"
#include "../../include/glove_eval_sim_hip.h"

namespace glove {

// scores[q, v] = s(b, v) s(c, v) / (s(a, v) + eps): sim_tile_gemm with table rows gathered by the question's three ids
// on the A side.  Workgroup = 64 questions x 128 vocabulary rows; a wave owns 32 questions and 64 vocabulary rows as
// three 32-row MFMA blocks (the a rows, the b rows and the c rows of the SAME 32 questions) times two 32-column blocks:
// acc[3][2], 96 accumulators.  In the C/D map the three dot products of (question, v) then sit at the same lane and
// register index: the epilogue scales them by the inverse norms of both operands, clamps, combines them and writes
// (q, v) once, the exclusion riding in that one store.  No intermediate matrix goes through memory; one call reads W
// once per 64 questions.
// Grid: one dimension, vocabulary tile fastest (n <= 65535 * 128 is more question tiles of 64 than gridDim.y takes).
constexpr int kMulQ = 64, kMulV = 128;

__global__ __launch_bounds__(kBlock) void cosmul_mfma_kernel(const float *__restrict__ R, int32_t V, int32_t d,
                                                             const int32_t *__restrict__ abc, int32_t n,
                                                             const float *__restrict__ inv_norm, float eps, int32_t nvt,
                                                             float *__restrict__ scores /* [n,V] */)
{
    __shared__ float Qs[3][kMulQ][kSimK + 1];              // the a rows, the b rows, the c rows
    __shared__ float Rs[kMulV][kSimK + 1];
    __shared__ int32_t q_id[kMulQ][3];                     // the tile's questions: -1 beyond n
    __shared__ float q_inv[kMulQ][3];
    const int v0 = (int)(blockIdx.x % (uint32_t)nvt) * kMulV, q0 = (int)(blockIdx.x / (uint32_t)nvt) * kMulQ;
    if (threadIdx.x < kMulQ * 3) {
        const int ql = threadIdx.x / 3, j = threadIdx.x % 3;
        const int32_t id = q0 + ql < n ? abc[(size_t)(q0 + ql) * 3 + j] : -1;
        q_id[ql][j] = id;
        q_inv[ql][j] = id >= 0 ? inv_norm[id] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;               // this wave's 32 questions and 64 vocabulary rows
    const int r32 = lane & 31, kh = lane >> 5;
    f32x16 acc[3][2];
    sim_tile_gemm(reinterpret_cast<float (&)[3 * kMulQ][kSimK + 1]>(Qs), Rs, acc, R, R, d,
                  [&](int row) { return q_id[row % kMulQ][row / kMulQ]; },       // row of Qs seen as [3 * kMulQ][kSimK + 1]
                  [&](int row) { return v0 + row < V ? v0 + row : -1; }, wm * 32, kMulQ, wn * 64);
    // C/D map: column = vocabulary row, row = question
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int v = v0 + wn * 64 + b * 32 + r32;
        const float iv = v < V ? inv_norm[v] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int ql = wm * 32 + sim_cd_row(reg, kh), q = q0 + ql;
            const float sa = 0.5f * (1.0f + clamp_cos(acc[0][b][reg] * q_inv[ql][0] * iv));
            const float sb = 0.5f * (1.0f + clamp_cos(acc[1][b][reg] * q_inv[ql][1] * iv));
            const float sc = 0.5f * (1.0f + clamp_cos(acc[2][b][reg] * q_inv[ql][2] * iv));
            // the exclusion rides in the one store of (q, v): no second writer to scores, no ordering question
            const bool own = v == q_id[ql][0] || v == q_id[ql][1] || v == q_id[ql][2];
            if (q < n && v < V) scores[(size_t)q * V + v] = own ? -INFINITY : sb * sc / (sa + eps);
        }
    }
}

// cos_out[p] = cos(x, y) of pair p = (x, y), one lane group per pair.  The three sums are one fma chain per lane and one
// butterfly per group: the summation order is fixed, the result repeatable bit for bit whatever the grid.
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void pair_cosine_kernel(const float *__restrict__ W, int d4,
                                                             const int32_t *__restrict__ pairs, int32_t n,
                                                             float *__restrict__ cos_out)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int p = blockIdx.x * GPB + grp; p < n; p += gridDim.x * GPB) {
        f4 x[NV], y[NV];
        load_row_p<LPR, NV>(x, W, pairs[(size_t)p * 2], d4, lg);
        load_row_p<LPR, NV>(y, W, pairs[(size_t)p * 2 + 1], d4, lg);
        float xy = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) xy += dot4(x[k], y[k]);
        xy = group_sum<LPR>(xy);
        const float xx = row_sumsq<LPR, NV>(x), yy = row_sumsq<LPR, NV>(y);
        if (lg == 0) cos_out[p] = clamp_cos(xy * clamped_inv_norm(xx) * clamped_inv_norm(yy));
    }
}

// the workspace: inv_norm[V] | scores[n V] | two ping-pong buffers of winners, each piece 256-B aligned
struct CosmulWs {
    float *inv_norm, *scores;
    void *pingpong;
    size_t bytes;
};

static CosmulWs carve_cosmul_ws(void *ws, int32_t n, int32_t V, int32_t k)
{
    WsCarver c{(char *)ws};
    CosmulWs s;
    s.inv_norm = c.take<float>((size_t)V);
    s.scores = c.take<float>((size_t)n * V);
    s.pingpong = c.take<char>(topk_pingpong_bytes(n, V, k));
    s.bytes = c.off;
    return s;
}

// vocabulary tiles x question tiles of the GEMM's one-dimensional grid
static int64_t cosmul_tiles(int32_t n, int32_t V)
{
    return (int64_t)((V + kMulV - 1) / kMulV) * (int64_t)((n + kMulQ - 1) / kMulQ);
}

// What both cosmul entry points refuse.  k <= V - 3 (topk_k_ok): every score is finite and >= 0, an excluded id is
// -inf, and the last selection stage sees V - 3 >= k finite candidates first.  (The tile count cannot reach 2^31
// with a score matrix that fits any memory; it is checked because the grid is computed from it.)
static bool cosmul_sizes_ok(int32_t n, int32_t V, int32_t d, int32_t k)
{
    if (n < 0 || n > 65535 * 128 || !sim_table_ok(V, d) || !topk_k_ok(k, V, 3)) return false;
    return cosmul_tiles(n, V) <= 0x7fffffff;
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_eval_sim_abi_version(void) { return GLOVE_EVAL_SIM_ABI_VERSION; }

size_t glove_cosmul_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t k)
{
    if (!cosmul_sizes_ok(n, V, d, k)) return 0;
    return carve_cosmul_ws(nullptr, n, V, k).bytes;
}

int glove_cosmul_topk_f32(const float *W, int32_t V, int32_t d, const int32_t *abc, int32_t n, int32_t k, float eps,
                          float *sims_out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!cosmul_sizes_ok(n, V, d, k)) return GLOVE_E_BADARG;
    if (!(eps > 0.f && eps <= 1.f)) return GLOVE_E_BADARG;             // (NaN fails both comparisons)
    if (n == 0) return 0;
    if (!W || !abc || !sims_out || !idx_out || !ws) return GLOVE_E_BADARG;
    const CosmulWs w = carve_cosmul_ws(ws, n, V, k);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nbv = blocks_for(V, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV) hipLaunchKernelGGL((inv_norm_kernel<LPR, NV>), dim3(nbv), dim3(kBlock), 0, st, W, V, d4, w.inv_norm)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    const int32_t nvt = (V + kMulV - 1) / kMulV;
    hipLaunchKernelGGL(cosmul_mfma_kernel, dim3((uint32_t)cosmul_tiles(n, V)), dim3(kBlock), 0, st, W, V, d, abc, n,
                       w.inv_norm, eps, nvt, w.scores);
    launch_topk_stages(w.scores, n, V, k, sims_out, idx_out, w.pingpong, st);
    return (int)hipGetLastError();
}

int glove_pair_cosine_f32(const float *W, int32_t V, int32_t d, const int32_t *pairs, int32_t n, float *cos_out,
                          void *stream)
{
    if (n < 0 || !sim_table_ok(V, d)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!W || !pairs || !cos_out) return GLOVE_E_BADARG;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nb = blocks_for(n, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV) hipLaunchKernelGGL((pair_cosine_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, W, d4, pairs, n, cos_out)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

}  // extern "C"
