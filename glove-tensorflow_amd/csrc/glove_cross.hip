// Nearest neighbours across two embedding tables on gfx950, by cosine or by CSLS: the fourth object of
// libglove_eval_hip.so, include/glove_eval_cross_hip.h (the semantics and the limits are stated there).
//
//   glove_cross_topk_f32   for n rows of Q (by id) the k rows of T with the largest cosine, or the largest
//                          2 cos - q_pen - t_pen (CSLS, Conneau et al. 2018).
//   glove_topk_mean_f32    the mean of each top-k list: a CSLS penalty.
//
// Five pieces on one stream: the inverse norms of the gathered query rows and of T's rows, the n x Vt similarity GEMM
// (cosine_mfma_kernel's tile, its A operand gathered from a second table, the penalties in its one store) and the
// staged top-k selection; all but the GEMM kernel are those of glove_topk_kernels.h, unchanged.
#include "glove_common.h"
#include "glove_topk_kernels.h"
#include "../../include/glove_eval_cross_hip.h"

namespace glove {

// sims[q, v] = ((Q[qid[q]] . T[v]) q_inv[q]) t_inv[v], or with the penalties ((2 cos) - q_pen[q]) - t_pen[v].
// Workgroup = 128 queries x 128 rows of T, four waves of 2 x 2 MFMA blocks through sim_tile_gemm, like
// cosine_mfma_kernel: a dot product's bits are those of PREDICT's.
template <bool kCsls>
__global__ __launch_bounds__(kBlock) void cross_cosine_mfma_kernel(const float *__restrict__ Q, const int32_t *__restrict__ qid,
                                                                   int32_t n, const float *__restrict__ T, int32_t Vt, int32_t d,
                                                                   const float *__restrict__ q_inv_all,
                                                                   const float *__restrict__ t_inv,
                                                                   const float *__restrict__ q_pen,
                                                                   const float *__restrict__ t_pen,
                                                                   float *__restrict__ sims /* [n, Vt] */)
{
    __shared__ float Qs[kSimTile][kSimK + 1];
    __shared__ float Ts[kSimTile][kSimK + 1];
    __shared__ float q_inv[kSimTile];                      // inverse norms of this tile's queries, for the epilogue
    __shared__ float q_p[kCsls ? kSimTile : 1];            // ... and their penalties
    const int v0 = blockIdx.x * kSimTile, q0 = blockIdx.y * kSimTile;
    if (threadIdx.x < kSimTile) {
        const bool in = q0 + threadIdx.x < n;
        q_inv[threadIdx.x] = in ? q_inv_all[q0 + threadIdx.x] : 0.f;
        if constexpr (kCsls) q_p[threadIdx.x] = in ? q_pen[q0 + threadIdx.x] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;               // this wave's 64 x 64 quadrant of the tile
    const int r32 = lane & 31, kh = lane >> 5;
    f32x16 acc[2][2];
    // (the first barrier of sim_tile_gemm stands between the stores to q_inv / q_p above and the epilogue's reads)
    sim_tile_gemm(Qs, Ts, acc, Q, T, d, [&](int row) -> int32_t { return q0 + row < n ? qid[q0 + row] : -1; },
                  [&](int row) -> int32_t { return v0 + row < Vt ? v0 + row : -1; }, wm * 64, 32, wn * 64);
    // C/D map: column = row of T, row = query
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int v = v0 + wn * 64 + b * 32 + r32;
        const float iv = v < Vt ? t_inv[v] : 0.f;
        float tp = 0.f;
        if constexpr (kCsls) tp = v < Vt ? t_pen[v] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int ql = wm * 64 + a * 32 + sim_cd_row(reg, kh), q = q0 + ql;
                const float c = acc[a][b][reg] * q_inv[ql] * iv;
                // the penalties ride in the one store of (q, v): two subtractions, each rounded
                float s = c;
                if constexpr (kCsls) s = __fsub_rn(__fsub_rn(__fmul_rn(2.0f, c), q_p[ql]), tp);
                if (q < n && v < Vt) sims[(size_t)q * Vt + v] = s;
            }
        }
    }
}

// mean_out[q] = (sims[q, 0] + sims[q, 1] + ... ) / k in that order: one thread per row
__global__ __launch_bounds__(kBlock) void topk_mean_kernel(const float *__restrict__ sims, int32_t n, int32_t k,
                                                           float *__restrict__ mean_out)
{
    for (int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x; q < n; q += (int64_t)gridDim.x * kBlock) {
        const float *row = sims + (size_t)q * k;
        float s = 0.f;
        for (int j = 0; j < k; ++j) s = __fadd_rn(s, row[j]);
        mean_out[q] = __fdiv_rn(s, (float)k);
    }
}

// the workspace: q_inv[n] | t_inv[Vt] | sims[n Vt] | two ping-pong buffers of winners, each piece 256-B aligned
struct CrossWs {
    float *q_inv, *t_inv, *sims;
    void *pingpong;
    size_t bytes;
};

static CrossWs carve_cross_ws(void *ws, int32_t n, int32_t Vt, int32_t k)
{
    WsCarver c{(char *)ws};
    CrossWs s;
    s.q_inv = c.take<float>((size_t)n);
    s.t_inv = c.take<float>((size_t)Vt);
    s.sims = c.take<float>((size_t)n * Vt);
    s.pingpong = c.take<char>(topk_pingpong_bytes(n, Vt, k));
    s.bytes = c.off;
    return s;
}

// What both entry points refuse (every row of T is a candidate: k <= Vt)
static bool cross_sizes_ok(int32_t n, int32_t Vt, int32_t d, int32_t k)
{
    return n >= 0 && n <= 65535 * kSimTile && sim_table_ok(Vt, d) && topk_k_ok(k, Vt, 0);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_eval_cross_abi_version(void) { return GLOVE_EVAL_CROSS_ABI_VERSION; }

size_t glove_cross_topk_workspace_bytes(int32_t n, int32_t Vt, int32_t d, int32_t k)
{
    if (!cross_sizes_ok(n, Vt, d, k)) return 0;
    return carve_cross_ws(nullptr, n, Vt, k).bytes;
}

int glove_cross_topk_f32(const float *Q, int32_t Vq, const int32_t *qid, int32_t n, const float *T, int32_t Vt, int32_t d,
                         int32_t k, const float *q_pen, const float *t_pen, float *sims_out, int32_t *idx_out,
                         void *ws, size_t ws_bytes, void *stream)
{
    if (!cross_sizes_ok(n, Vt, d, k) || Vq <= 0) return GLOVE_E_BADARG;
    if ((q_pen == nullptr) != (t_pen == nullptr)) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!Q || !qid || !T || !sims_out || !idx_out || !ws) return GLOVE_E_BADARG;
    const CrossWs w = carve_cross_ws(ws, n, Vt, k);
    if (w.bytes > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int nbq = blocks_for(n, kBlock / shape.lpr), nbv = blocks_for(Vt, kBlock / shape.lpr);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV)                                                                                               \
    hipLaunchKernelGGL((gathered_inv_norm_kernel<LPR, NV>), dim3(nbq), dim3(kBlock), 0, st, Q, d4, qid, n, w.q_inv); \
    hipLaunchKernelGGL((inv_norm_kernel<LPR, NV>), dim3(nbv), dim3(kBlock), 0, st, T, Vt, d4, w.t_inv)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    const dim3 grid((Vt + kSimTile - 1) / kSimTile, (n + kSimTile - 1) / kSimTile);
    if (q_pen)
        hipLaunchKernelGGL(cross_cosine_mfma_kernel<true>, grid, dim3(kBlock), 0, st, Q, qid, n, T, Vt, d, w.q_inv, w.t_inv,
                           q_pen, t_pen, w.sims);
    else
        hipLaunchKernelGGL(cross_cosine_mfma_kernel<false>, grid, dim3(kBlock), 0, st, Q, qid, n, T, Vt, d, w.q_inv, w.t_inv,
                           q_pen, t_pen, w.sims);
    launch_topk_stages(w.sims, n, Vt, k, sims_out, idx_out, w.pingpong, st);
    return (int)hipGetLastError();
}

int glove_topk_mean_f32(const float *sims, int32_t n, int32_t k, float *mean_out, void *stream)
{
    if (n < 0 || k < 1) return GLOVE_E_BADARG;
    if (n == 0) return 0;
    if (!sims || !mean_out) return GLOVE_E_BADARG;
    hipLaunchKernelGGL(topk_mean_kernel, dim3(blocks_for(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, sims, n, k,
                       mean_out);
    return (int)hipGetLastError();
}

}  // extern "C"
