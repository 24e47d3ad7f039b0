// What one lane group does with dense rows of d4 float4 and the positions of a CSR row: the inline helpers the kernels of
// glove_factor.hip (glove_csr_spmm_f32) and of glove_retrofit.hip (glove_retrofit_rows_f32) share.  No kernel lives here:
// every kernel is instantiated in exactly one object.
#pragma once
#include "glove_common.h"

namespace glove {

constexpr int kInFlight = 4;              // partner rows a lane group has in flight (MI355X: 4 per wave measured near the HBM rate)

template <int LPR, int NV>
__device__ inline void load_dense(f4 (&r)[NV], const f4 *__restrict__ row, int d4, int lg)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int q = lg + k * LPR;
        r[k] = q < d4 ? row[q] : f4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int LPR, int NV>
__device__ inline void store_dense(const f4 (&r)[NV], f4 *__restrict__ row, int d4, int lg)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int q = lg + k * LPR;
        if (q < d4) row[q] = r[k];
    }
}

template <int NV>
__device__ inline void fma_row(f4 (&acc)[NV], float v, const f4 (&r)[NV])
{
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        acc[k].x = __builtin_fmaf(v, r[k].x, acc[k].x);
        acc[k].y = __builtin_fmaf(v, r[k].y, acc[k].y);
        acc[k].z = __builtin_fmaf(v, r[k].z, acc[k].z);
        acc[k].w = __builtin_fmaf(v, r[k].w, acc[k].w);
    }
}

// acc = the chunk sum of positions [beg, end) in position order, by the LPR lanes of one group (lane lg of it): every
// lane reads the same (column, value) words — one request per group — and its own float4 of the partner row.  kInFlight
// partner rows are loaded before the first of them is used, the next trip's columns and values before that.  A column
// outside [0, n_cols) adds nothing (and is not loaded).  UNIT: every value is 1 and `val` is not read (it may be null).
template <int LPR, int NV, bool UNIT = false>
__device__ inline void chunk_sum(f4 (&acc)[NV], const int32_t *__restrict__ col_idx, const float *__restrict__ val,
                                 int64_t beg, int64_t end, const f4 *__restrict__ B, int d4, int32_t n_cols, int lg)
{
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = f4{0.f, 0.f, 0.f, 0.f};
    int64_t p = beg;
    int32_t c[kInFlight];
    float v[kInFlight];
    if (p + kInFlight <= end) {
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) { c[u] = col_idx[p + u]; v[u] = UNIT ? 1.f : val[p + u]; }
    }
    while (p + kInFlight <= end) {
        f4 r[kInFlight][NV];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const bool in = (uint32_t)c[u] < (uint32_t)n_cols;
            load_dense<LPR, NV>(r[u], B + (size_t)(in ? c[u] : 0) * d4, in ? d4 : 0, lg);
        }
        float vc[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) vc[u] = (uint32_t)c[u] < (uint32_t)n_cols ? v[u] : 0.f;
        p += kInFlight;
        if (p + kInFlight <= end) {
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) { c[u] = col_idx[p + u]; v[u] = UNIT ? 1.f : val[p + u]; }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) fma_row<NV>(acc, vc[u], r[u]);
    }
    for (; p < end; ++p) {
        const int32_t cc = col_idx[p];
        if ((uint32_t)cc >= (uint32_t)n_cols) continue;
        f4 r[NV];
        load_dense<LPR, NV>(r, B + (size_t)cc * d4, d4, lg);
        fma_row<NV>(acc, UNIT ? 1.f : val[p], r);
    }
}

}  // namespace glove
