// Word-analogy evaluation (3CosAdd) of finished embeddings on gfx950: libglove_eval_hip.so, include/glove_eval_hip.h.
//
//   glove_analogy_topk_f32   for questions a : b :: c : ?, the k vocabulary rows closest by cosine to
//                            w^_b - w^_a + w^_c, the question's own three words left out (GloVe's
//                            eval/python/evaluate.py, gensim most_similar).
//
// Four pieces on one stream: inverse row norms, the dense query rows, the n x V similarity GEMM (the kernel of the
// PREDICT path with a dense query operand, the exclusion in its epilogue) and the staged top-k selection, all but the
// second shared with glove_predict.hip through glove_topk_kernels.h.
#include "glove_common.h"
#include "glove_topk_kernels.h"
#include "../../include/glove_eval_hip.h"

namespace glove {

// Q[q] = w^_b - w^_a + w^_c and q_inv[q] = 1/sqrt(max(|Q[q]|^2, 1e-12)), one lane group per question.  The three
// products are spelled out as one fma chain per element, the sum of squares is row_sumsq's: the summation order is
// fixed, the result repeatable bit for bit whatever the grid.
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void analogy_query_kernel(const float *__restrict__ W, int d4,
                                                               const int32_t *__restrict__ abc, int32_t n,
                                                               const float *__restrict__ inv_norm,
                                                               float *__restrict__ Q, float *__restrict__ q_inv)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    for (int q = blockIdx.x * GPB + grp; q < n; q += gridDim.x * GPB) {
        const int32_t ia = abc[(size_t)q * 3], ib = abc[(size_t)q * 3 + 1], ic = abc[(size_t)q * 3 + 2];
        const float na = inv_norm[ia], nb = inv_norm[ib], nc = inv_norm[ic];
        f4 a[NV], b[NV], c[NV], x[NV];
        load_row_p<LPR, NV>(a, W, ia, d4, lg);
        load_row_p<LPR, NV>(b, W, ib, d4, lg);
        load_row_p<LPR, NV>(c, W, ic, d4, lg);
#pragma unroll
        for (int k = 0; k < NV; ++k) {                  // (lanes beyond the row hold zeros)
            x[k].x = __builtin_fmaf(c[k].x, nc, __builtin_fmaf(-a[k].x, na, b[k].x * nb));
            x[k].y = __builtin_fmaf(c[k].y, nc, __builtin_fmaf(-a[k].y, na, b[k].y * nb));
            x[k].z = __builtin_fmaf(c[k].z, nc, __builtin_fmaf(-a[k].z, na, b[k].z * nb));
            x[k].w = __builtin_fmaf(c[k].w, nc, __builtin_fmaf(-a[k].w, na, b[k].w * nb));
        }
        store_row_p<LPR, NV>(Q, q, d4, lg, x);
        const float s = row_sumsq<LPR, NV>(x);
        if (lg == 0) q_inv[q] = clamped_inv_norm(s);
    }
}

// the workspace: inv_norm[V] | Q[n d] | q_inv[n] | sims[n V] | two ping-pong buffers of winners, each 256-B aligned
struct AnalogyWs {
    float *inv_norm, *Q, *q_inv, *sims;
    void *pingpong;
    size_t bytes;
};

static AnalogyWs carve_analogy_ws(void *ws, int32_t n, int32_t V, int32_t d, int32_t k)
{
    WsCarver c{(char *)ws};
    AnalogyWs s;
    s.inv_norm = c.take<float>((size_t)V);
    s.Q = c.take<float>((size_t)n * d);
    s.q_inv = c.take<float>((size_t)n);
    s.sims = c.take<float>((size_t)n * V);
    s.pingpong = c.take<char>(topk_pingpong_bytes(n, V, k));
    s.bytes = c.off;
    return s;
}

// What both entry points refuse (k <= V - 3: topk_k_ok says why)
static bool analogy_sizes_ok(int32_t n, int32_t V, int32_t d, int32_t k)
{
    return n >= 0 && n <= 65535 * kSimTile && sim_table_ok(V, d) && topk_k_ok(k, V, 3);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_eval_abi_version(void) { return GLOVE_EVAL_ABI_VERSION; }

size_t glove_analogy_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t k)
{
    if (!analogy_sizes_ok(n, V, d, k)) return 0;
    return carve_analogy_ws(nullptr, n, V, d, k).bytes;
}

int glove_analogy_topk_f32(const float *W, int32_t V, int32_t d, const int32_t *abc, int32_t n, int32_t k,
                           float *sims_out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!analogy_sizes_ok(n, V, d, k)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!W || !abc || !sims_out || !idx_out || !ws) return GLOVE_E_BADARG;
    const AnalogyWs w = carve_analogy_ws(ws, n, V, d, k);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nbv = blocks_for(V, kBlock / shape.lpr), nbq = blocks_for(n, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV)                                                                                                  \
    hipLaunchKernelGGL((inv_norm_kernel<LPR, NV>), dim3(nbv), dim3(kBlock), 0, st, W, V, d4, w.inv_norm);              \
    hipLaunchKernelGGL((analogy_query_kernel<LPR, NV>), dim3(nbq), dim3(kBlock), 0, st, W, d4, abc, n, w.inv_norm, w.Q, \
                       w.q_inv)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    const DenseQueries src{w.Q, w.q_inv, abc};
    hipLaunchKernelGGL(cosine_mfma_kernel<DenseQueries>, dim3((V + kSimTile - 1) / kSimTile, (n + kSimTile - 1) / kSimTile),
                       dim3(kBlock), 0, st, W, V, d, src, n, w.inv_norm, w.sims);
    launch_topk_stages(w.sims, n, V, k, sims_out, idx_out, w.pingpong, st);
    return (int)hipGetLastError();
}

}  // extern "C"
