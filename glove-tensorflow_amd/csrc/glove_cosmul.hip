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
// glove_analogy.hip through glove_topk_kernels.h (which this file leaves as it is).
#include "glove_common.h"
#include "glove_topk_kernels.h"
#include "../../include/glove_eval_sim_hip.h"

namespace glove {

__device__ inline float clamp_cos(float c) { return fminf(fmaxf(c, -1.0f), 1.0f); }

// scores[q, v] = s(b, v) s(c, v) / (s(a, v) + eps): the similarity GEMM of glove_topk_kernels.h with a third query source,
// table rows gathered by the question's three ids.  Workgroup = 64 questions x 128 vocabulary rows; a wave owns 32
// questions and 64 vocabulary rows as three 32-row MFMA blocks (the a rows, the b rows and the c rows of the SAME 32
// questions) times two 32-column blocks: acc[3][2], 96 accumulators, on v_mfma_f32_32x32x2_f32 — a k-ordered fmaf chain,
// so a dot product's bits do not depend on where in a tile or a batch the question sits.  In the C/D map the three dot
// products of (question, v) then sit at the same lane and register index: the epilogue scales them by the inverse
// norms of both operands, clamps, combines them and writes (q, v) once, the exclusion riding in that one store.  No
// intermediate matrix goes through memory.  The operands go through LDS in slabs of 32 columns as in
// cosine_mfma_kernel (row stride 33 floats); one call reads W once per 64 questions.
// Grid: one dimension, vocabulary tile fastest (n <= 65535 * 128 is more question tiles of 64 than gridDim.y takes).
constexpr int kMulQ = 64, kMulV = 128;

__global__ __launch_bounds__(kBlock) void cosmul_mfma_kernel(const float *__restrict__ R, int32_t V, int32_t d,
                                                             const int32_t *__restrict__ abc, int32_t n,
                                                             const float *__restrict__ inv_norm, float eps, int32_t nvt,
                                                             float *__restrict__ scores /* [n,V] */)
{
    __shared__ float Qs[3][kMulQ][kSimK + 1];
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
    const int r32 = lane & 31, kh = lane >> 5;             // operand maps: A[i = lane & 31][k = lane >> 5], B likewise
    f32x16 acc[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][b][i] = 0.f;

    // a slab = 3 x 64 gathered rows and 128 vocabulary rows x 32 columns: 8 threads x 16 B per row, zero beyond n / V / d.
    // The next slab's global loads are issued before the MFMAs of the current one and land in LDS after them.
    constexpr int kPerQ = 3 * kMulQ * (kSimK / 4) / kBlock, kPerR = kMulV * (kSimK / 4) / kBlock;
    f4 qn[kPerQ], rn[kPerR];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int x = 0; x < kPerQ; ++x) {
            const int i = threadIdx.x + x * kBlock;
            const int row = i / (kSimK / 4), c = (i % (kSimK / 4)) * 4;
            const int32_t id = q_id[row % kMulQ][row / kMulQ];
            qn[x] = f4{0.f, 0.f, 0.f, 0.f};
            if (k0 + c < d && id >= 0) qn[x] = *reinterpret_cast<const f4 *>(R + (size_t)id * d + k0 + c);
        }
#pragma unroll
        for (int x = 0; x < kPerR; ++x) {
            const int i = threadIdx.x + x * kBlock;
            const int row = i / (kSimK / 4), c = (i % (kSimK / 4)) * 4;
            rn[x] = f4{0.f, 0.f, 0.f, 0.f};
            if (k0 + c < d && v0 + row < V) rn[x] = *reinterpret_cast<const f4 *>(R + (size_t)(v0 + row) * d + k0 + c);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += kSimK) {
#pragma unroll
        for (int x = 0; x < kPerQ; ++x) {
            const int i = threadIdx.x + x * kBlock;
            const int row = i / (kSimK / 4), c = (i % (kSimK / 4)) * 4;
            float *q = &Qs[row / kMulQ][row % kMulQ][c];
            q[0] = qn[x].x; q[1] = qn[x].y; q[2] = qn[x].z; q[3] = qn[x].w;
        }
#pragma unroll
        for (int x = 0; x < kPerR; ++x) {
            const int i = threadIdx.x + x * kBlock;
            const int row = i / (kSimK / 4), c = (i % (kSimK / 4)) * 4;
            Rs[row][c] = rn[x].x; Rs[row][c + 1] = rn[x].y; Rs[row][c + 2] = rn[x].z; Rs[row][c + 3] = rn[x].w;
        }
        __syncthreads();
        if (k0 + kSimK < d) fetch(k0 + kSimK);
#pragma unroll 4
        for (int kk = 0; kk < kSimK; kk += 2) {
            const float a = Qs[0][wm * 32 + r32][kk + kh], b = Qs[1][wm * 32 + r32][kk + kh], c = Qs[2][wm * 32 + r32][kk + kh];
            const float r0 = Rs[wn * 64 + r32][kk + kh], r1 = Rs[wn * 64 + 32 + r32][kk + kh];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, r0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, r1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, r0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, r1, acc[1][1], 0, 0, 0);
            acc[2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(c, r0, acc[2][0], 0, 0, 0);
            acc[2][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(c, r1, acc[2][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: column (vocabulary row) = lane & 31, row (question) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int v = v0 + wn * 64 + b * 32 + r32;
        const float iv = v < V ? inv_norm[v] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int ql = wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh, q = q0 + ql;
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
        float xy = 0.f, xx = 0.f, yy = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            xy += dot4(x[k], y[k]);
            xx += dot4(x[k], x[k]);
            yy += dot4(y[k], y[k]);
        }
        xy = group_sum<LPR>(xy);
        xx = group_sum<LPR>(xx);
        yy = group_sum<LPR>(yy);
        if (lg == 0) cos_out[p] = clamp_cos(xy * (1.0f / sqrtf(fmaxf(xx, 1e-12f))) * (1.0f / sqrtf(fmaxf(yy, 1e-12f))));
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
    CosmulWs s;
    size_t off = 0;
    auto take = [&](size_t nfloats) {
        float *p = (float *)((char *)ws + off);
        off += align_up(nfloats * sizeof(float), 256);
        return p;
    };
    s.inv_norm = take((size_t)V);
    s.scores = take((size_t)n * V);
    s.pingpong = (char *)ws + off;
    s.bytes = off + topk_pingpong_bytes(n, V, k);
    return s;
}

static bool sim_table_ok(int32_t V, int32_t d)
{
    return V > 0 && d > 0 && (d % 4) == 0 && pick_row_shape(d / 4).lpr != 0;
}

// vocabulary tiles x question tiles of the GEMM's one-dimensional grid
static int64_t cosmul_tiles(int32_t n, int32_t V)
{
    return (int64_t)((V + kMulV - 1) / kMulV) * (int64_t)((n + kMulQ - 1) / kMulQ);
}

// What both cosmul entry points refuse.  k <= V - 3 as in glove_analogy.hip: every score is finite and >= 0, an excluded
// id is -inf, and the last selection stage sees V - 3 >= k finite candidates first.  (The tile count cannot reach 2^31
// with a score matrix that fits any memory; it is checked because the grid is computed from it.)
static bool cosmul_sizes_ok(int32_t n, int32_t V, int32_t d, int32_t k)
{
    if (n < 0 || n > 65535 * 128 || !sim_table_ok(V, d)) return false;
    if (k < 1 || k > 1024 || (int64_t)k > (int64_t)V - 3) return false;
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
