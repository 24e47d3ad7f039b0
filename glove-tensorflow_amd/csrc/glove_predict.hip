// EVAL and PREDICT modes of the reference model_fn on gfx950.
//
//   glove_eval_f32         RegressionHead eval metrics (reference src/models/estimator.py:48-56:
//                          average_loss / prediction/mean / label/mean are weighted sums over the
//                          eval pass) — forward only, tables untouched.
//   glove_topk_cosine_f32  get_predictions (src/models/model_utils.py:81-110): cosine_similarity
//                          (src/models/utils.py:12-19) of query ROW embeddings against all V row
//                          embeddings + tf.math.top_k (descending, ties -> lower index).  Its kernels
//                          are those of glove_topk_kernels.h, shared with libglove_eval_hip.so; the GEMM's
//                          tile loop is glove_sim_gemm.h.
#include "glove_common.h"
#include "glove_topk_kernels.h"

namespace glove {

__device__ inline double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void eval_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                      const float *__restrict__ w, const float *__restrict__ y,
                                                      int64_t B, const float *__restrict__ R,
                                                      const float *__restrict__ C, const float *__restrict__ br,
                                                      const float *__restrict__ bc, const float *__restrict__ scalars,
                                                      int d4, double *__restrict__ sums, int head)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const float g = scalars[0];
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0;
    for (int64_t i = (int64_t)blockIdx.x * GPB + grp; i < B; i += (int64_t)gridDim.x * GPB) {
        const int32_t u = row[i], v = col[i];
        f4 r[NV], c[NV];
        load_row_p<LPR, NV>(r, R, u, d4, lg);
        load_row_p<LPR, NV>(c, C, v, d4, lg);
        float dp = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) dp += dot4(r[k], c[k]);
        const float p = group_sum<LPR>(dp) + br[u] + bc[v] + g;
        if (lg == 0 && head == GLOVE_HEAD_REGRESSION) {
            const double wi = w[i], yi = y[i], diff = (double)p - yi;
            a0 += wi * diff * diff; a1 += wi; a2 += wi * (double)p; a3 += wi * yi;
        } else if (lg == 0) {
            // w = positive weight (label 1), y = negative weight (label 0); sigmoid cross-entropy of one logit
            const double pos = w[i], neg = y[i], x = p;
            const double lse = log1p(exp(-fabs(x))), sg = 1.0 / (1.0 + exp(-x));
            a0 += pos * (fmax(-x, 0.0) + lse); a1 += pos; a2 += neg * (fmax(x, 0.0) + lse); a3 += neg;
            a4 += pos * sg; a5 += neg * sg;
        }
    }
    a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2); a3 = wave_sum_f64(a3);
    if (head != GLOVE_HEAD_REGRESSION) { a4 = wave_sum_f64(a4); a5 = wave_sum_f64(a5); }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sums[0], a0); atomicAdd(&sums[1], a1); atomicAdd(&sums[2], a2); atomicAdd(&sums[3], a3);
        if (head != GLOVE_HEAD_REGRESSION) { atomicAdd(&sums[4], a4); atomicAdd(&sums[5], a5); }
    }
}

// the workspace: inv_norm[V] | sims[n V] | two ping-pong buffers of winners, each piece 256-B aligned
struct TopkWs {
    float *inv_norm, *sims;
    void *pingpong;
    size_t bytes;
};

static TopkWs carve_topk_ws(void *ws, int32_t n, int32_t V, int32_t k)
{
    WsCarver c{(char *)ws};
    TopkWs s;
    s.inv_norm = c.take<float>((size_t)V);
    s.sims = c.take<float>((size_t)n * V);
    s.pingpong = c.take<char>(topk_pingpong_bytes(n, V, k));
    s.bytes = c.off;
    return s;
}

}  // namespace glove

using namespace glove;

extern "C" {

static int launch_eval(const int32_t *row, const int32_t *col, const float *w, const float *y, int64_t B,
                       const glove_tables *t, double *sums_out, void *stream, int head);

int glove_eval_f32(const int32_t *row, const int32_t *col, const float *w, const float *y, int64_t B,
                   const glove_tables *t, double *sums_out, void *stream)
{
    return launch_eval(row, col, w, y, B, t, sums_out, stream, GLOVE_HEAD_REGRESSION);
}

int glove_eval_logistic_f32(const int32_t *row, const int32_t *col, const float *pos, const float *neg, int64_t B,
                            const glove_tables *t, double *sums_out, void *stream)
{
    return launch_eval(row, col, pos, neg, B, t, sums_out, stream, GLOVE_HEAD_LOGISTIC);
}

static int launch_eval(const int32_t *row, const int32_t *col, const float *w, const float *y, int64_t B,
                       const glove_tables *t, double *sums_out, void *stream, int head)
{
    if (!t || !sums_out || B < 0 || t->V <= 0 || t->d <= 0 || (t->d % 4) != 0) return GLOVE_E_BADARG;
    if (!t->R || !t->C || !t->br || !t->bc || !t->scalars) return GLOVE_E_BADARG;
    if (B == 0) return 0;
    if (!row || !col || !w || !y) return GLOVE_E_BADARG;
    const int d4 = t->d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nb = blocks_for(B, kBlock / (shape.lpr ? shape.lpr : 64));
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV)                                                                                           \
    hipLaunchKernelGGL((eval_kernel<LPR, NV>), dim3(nb), dim3(kBlock), 0, st, row, col, w, y, B, t->R, t->C, \
                       t->br, t->bc, t->scalars, d4, sums_out, head)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

size_t glove_topk_workspace_bytes(int32_t n, int32_t V, int32_t k)
{
    if (n < 0 || V <= 0 || k < 0) return 0;
    return carve_topk_ws(nullptr, n, V, k).bytes;
}

int glove_topk_cosine_f32(const float *R, int32_t V, int32_t d, const int32_t *query_ids, int32_t n, int32_t k,
                          float *sims_out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream)
{
    // (not sim_table_ok: a d beyond the widest row shape is refused behind the workspace check, as it always was)
    if (!R || V <= 0 || d <= 0 || (d % 4) != 0 || n < 0 || n > 65535 * kSimTile || !topk_k_ok(k, V, 0)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!query_ids || !sims_out || !idx_out || !ws) return GLOVE_E_BADARG;
    const TopkWs w = carve_topk_ws(ws, n, V, k);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    if (shape.lpr == 0) return GLOVE_E_BADARG;
    const int nbv = blocks_for(V, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV) hipLaunchKernelGGL((inv_norm_kernel<LPR, NV>), dim3(nbv), dim3(kBlock), 0, st, R, V, d4, w.inv_norm)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    hipLaunchKernelGGL(cosine_mfma_kernel<GatheredQueries>, dim3((V + kSimTile - 1) / kSimTile, (n + kSimTile - 1) / kSimTile),
                       dim3(kBlock), 0, st, R, V, d, GatheredQueries{query_ids}, n, w.inv_norm, w.sims);
    launch_topk_stages(w.sims, n, V, k, sims_out, idx_out, w.pingpong, st);
    return (int)hipGetLastError();
}

}  // extern "C"
