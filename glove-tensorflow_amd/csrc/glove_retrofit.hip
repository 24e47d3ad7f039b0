// Retrofitting a table to a semantic lexicon (Faruqui et al. 2015) on gfx950: the third object of libglove_factor_hip.so,
// include/glove_factor_graph_hip.h (the update, its order and the contract for in-place calls are stated there).
//
//   glove_retrofit_rows_f32  one launch: one lane group per LISTED row gathers the rows its positions name (the gather of
//                            glove_csr_spmm_f32: glove_lane_rows.h), adds alpha w times its own trained row and divides.
//                            Out of place over all rows it is a Jacobi sweep in one trip of the table; in place over the
//                            rows of one level of trainer.retrofit.level_schedule it is the sequential (Gauss-Seidel)
//                            sweep in vocabulary order, level by level.
//
// A row is one chain whatever its length (rows are not chunked): the bits must be those of a scalar loop over the row's
// positions, and a lexicon row of thousands of neighbours is rare.
#include "glove_common.h"
#include "glove_lane_rows.h"
#include "../../include/glove_factor_graph_hip.h"

#include <cmath>

namespace glove {

// w of the header's step 2: the float32 sum of the weights of positions [beg, end) in position order, the positions whose
// column lies outside [0, n) left out.  Every lane of the group computes the same sum from the same words.
template <bool UNIT>
__device__ inline float weight_sum(const int32_t *__restrict__ col_idx, const float *__restrict__ beta, int64_t beg,
                                   int64_t end, int32_t n)
{
    float w = 0.f;
#pragma unroll 4
    for (int64_t p = beg; p < end; ++p) {
        const float b = UNIT ? 1.f : beta[p];
        if ((uint32_t)col_idx[p] < (uint32_t)n) w = w + b;
    }
    return w;
}

// Steps 3 and 4 of the header for one float4: (t q_hat + s) / (t + w).  The product alpha w is formed by the caller; here
// nothing may be contracted: den is one addition, num one fmaf.
__device__ inline f4 retrofit_quotient(float t, float den, const f4 qh, const f4 s)
{
    f4 o;
    o.x = __builtin_fmaf(t, qh.x, s.x) / den;
    o.y = __builtin_fmaf(t, qh.y, s.y) / den;
    o.z = __builtin_fmaf(t, qh.z, s.z) / den;
    o.w = __builtin_fmaf(t, qh.w, s.w) / den;
    return o;
}

// Q_in and Q_out carry no __restrict__: they are one table in the in-place sweep.  A lane stores the float4s it loaded
// itself (a row that lists itself), after every load of its chain; the rows other groups store are read by nobody
// (the header's contract).
template <int LPR, int NV, bool UNIT>
__global__ __launch_bounds__(kBlock) void retrofit_rows_kernel(const int64_t *__restrict__ row_ptr,
                                                               const int32_t *__restrict__ col_idx,
                                                               const float *__restrict__ beta, int32_t n, int64_t nnz,
                                                               const int32_t *__restrict__ rows, int32_t n_list,
                                                               const f4 *__restrict__ Q_hat, const f4 *Q_in, f4 *Q_out,
                                                               int d4, float alpha)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR;
    const int64_t j = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    if (j >= n_list) return;
    const int32_t i = rows ? rows[j] : (int32_t)j;
    if ((uint32_t)i >= (uint32_t)n) return;                 // (a listed id outside [0, n): skipped)
    int64_t a = row_ptr[i], b = row_ptr[i + 1];
    if (a < 0 || b > nnz || b < a) a = b = 0;               // (a row_ptr that leaves [0, nnz]: an empty row)
    const float w = weight_sum<UNIT>(col_idx, beta, a, b, n);
    f4 acc[NV];
    if (w == 0.f) {                                    // no position, none in range, or weights that cancel: a copy
        load_dense<LPR, NV>(acc, Q_in + (size_t)i * d4, d4, lg);
        store_dense<LPR, NV>(acc, Q_out + (size_t)i * d4, d4, lg);
        return;
    }
    f4 qh[NV];
    load_dense<LPR, NV>(qh, Q_hat + (size_t)i * d4, d4, lg);
    chunk_sum<LPR, NV, UNIT>(acc, col_idx, beta, a, b, Q_in, d4, n, lg);
    float t, den;
    {
#pragma clang fp contract(off)
        t = alpha * w;
        den = t + w;
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = retrofit_quotient(t, den, qh[k], acc[k]);
    store_dense<LPR, NV>(acc, Q_out + (size_t)i * d4, d4, lg);
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_factor_graph_abi_version(void) { return GLOVE_FACTOR_GRAPH_ABI_VERSION; }

int glove_retrofit_rows_f32(const int64_t *row_ptr, const int32_t *col_idx, const float *beta, int32_t n, int64_t nnz,
                            const int32_t *rows, int32_t n_list, const float *Q_hat, const float *Q_in, float *Q_out,
                            int32_t d, float alpha, void *stream)
{
    if (n < 1 || nnz < 0 || nnz > INT32_MAX || n_list < 0 || n_list > n) return GLOVE_E_BADARG;
    if (d < 4 || d > 1024 || d % 4 != 0 || !std::isfinite(alpha) || alpha < 0.f) return GLOVE_E_BADARG;
    if (!rows && n_list != n) return GLOVE_E_BADARG;
    if (!row_ptr || !Q_hat || !Q_in || !Q_out || Q_out == Q_hat || (nnz > 0 && !col_idx)) return GLOVE_E_BADARG;
    if (n_list == 0) return 0;
    const int d4 = d / 4;
    const RowShape shape = pick_row_shape(d4);
    const int gpb = kBlock / shape.lpr;
    const unsigned nb = (unsigned)(((int64_t)n_list + gpb - 1) / gpb);
    hipStream_t st = (hipStream_t)stream;
#define LAUNCH(LPR, NV, UNIT)                                                                                           \
    hipLaunchKernelGGL((retrofit_rows_kernel<LPR, NV, UNIT>), dim3(nb), dim3(kBlock), 0, st, row_ptr, col_idx, beta, n, \
                       nnz, rows, n_list, (const f4 *)Q_hat, (const f4 *)Q_in, (f4 *)Q_out, d4, alpha)
#define CALL(LPR, NV)                                                                                                   \
    if (beta) LAUNCH(LPR, NV, false);                                                                                   \
    else LAUNCH(LPR, NV, true)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
#undef LAUNCH
    return (int)hipGetLastError();
}

}  // extern "C"
