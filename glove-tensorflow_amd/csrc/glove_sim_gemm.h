// The one tile loop of the similarity GEMMs: cosine_mfma_kernel (glove_topk_kernels.h: PREDICT and 3CosAdd),
// cosmul_mfma_kernel (glove_cosmul.hip) and kmeans_assign_kernel (glove_kmeans.hip).  The kernels keep their LDS arrays,
// their prologues and their epilogues; which table row a tile row is comes from a callable they pass in.
#pragma once
#include "glove_common.h"

namespace glove {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kSimK = 32;                                  // columns of a slab

// acc[j][b] = (A block j of this wave) x (B block b)^T over the d columns of the rows, on v_mfma_f32_32x32x2_f32 in exact
// f32: a k-ordered fmaf chain per accumulator (k = 0, 1, 2, ...), so a dot product's bits are those of a scalar loop and
// do not depend on the tile, the block or the kernel.
// The operands go through LDS in slabs of kSimK columns (row stride 33 floats: a tile column is read conflict-free):
// 8 threads x 16 B per row, zeros where the tile row is no row or the column is >= d (d is a multiple of 4).  The next
// slab's global loads are issued before the MFMAs of the current one and land in LDS after them; two barriers per slab,
// the last of them behind the last MFMA (the caller may rewrite what the callables read, and call again).
//   a_id / b_id     tile row (0 .. TA - 1 / TB - 1) -> the row of A / B [rows, d] it holds, or < 0 for none (a null
//                   pointer here instead cost 3CosMul's six gathers per slab 0.8 % of its time: DESIGN.md)
//   A block j       LDS rows a_base + j * a_step + (lane & 31);  B block b: b_base + b * 32 + (lane & 31)
// Operand maps: A[i = lane & 31][k = lane >> 5], B likewise; MFMA order A block outer, B block inner.
template <int TA, int TB, int MA, int NB, class PA, class PB>
__device__ inline void sim_tile_gemm(float (&As)[TA][kSimK + 1], float (&Bs)[TB][kSimK + 1], f32x16 (&acc)[MA][NB],
                                     const float *A, const float *B, int d, PA a_id, PB b_id, int a_base, int a_step, int b_base)
{
    constexpr int kQuads = kSimK / 4;                      // float4 per row and slab
    constexpr int kPerA = TA * kQuads / kBlock, kPerB = TB * kQuads / kBlock;   // float4 per thread, operand and slab
    static_assert(TA * kQuads % kBlock == 0 && TB * kQuads % kBlock == 0, "a slab is whole float4s per thread");
    const int r32 = threadIdx.x & 31, kh = (threadIdx.x >> 5) & 1;
#pragma unroll
    for (int j = 0; j < MA; ++j)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][b][i] = 0.f;
    f4 an[kPerA], bn[kPerB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int x = 0; x < kPerA; ++x) {
            const int i = threadIdx.x + x * kBlock, c = (i % kQuads) * 4;
            const int32_t id = a_id(i / kQuads);
            an[x] = f4{0.f, 0.f, 0.f, 0.f};
            if (k0 + c < d && id >= 0) an[x] = *reinterpret_cast<const f4 *>(A + (size_t)id * d + k0 + c);
        }
#pragma unroll
        for (int x = 0; x < kPerB; ++x) {
            const int i = threadIdx.x + x * kBlock, c = (i % kQuads) * 4;
            const int32_t id = b_id(i / kQuads);
            bn[x] = f4{0.f, 0.f, 0.f, 0.f};
            if (k0 + c < d && id >= 0) bn[x] = *reinterpret_cast<const f4 *>(B + (size_t)id * d + k0 + c);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += kSimK) {
#pragma unroll
        for (int x = 0; x < kPerA; ++x) {
            const int i = threadIdx.x + x * kBlock;
            float *s = &As[i / kQuads][(i % kQuads) * 4];
            s[0] = an[x].x; s[1] = an[x].y; s[2] = an[x].z; s[3] = an[x].w;
        }
#pragma unroll
        for (int x = 0; x < kPerB; ++x) {
            const int i = threadIdx.x + x * kBlock;
            float *s = &Bs[i / kQuads][(i % kQuads) * 4];
            s[0] = bn[x].x; s[1] = bn[x].y; s[2] = bn[x].z; s[3] = bn[x].w;
        }
        __syncthreads();
        if (k0 + kSimK < d) fetch(k0 + kSimK);
#pragma unroll 4
        for (int kk = 0; kk < kSimK; kk += 2) {
            float a[MA], b[NB];
#pragma unroll
            for (int j = 0; j < MA; ++j) a[j] = As[a_base + j * a_step + r32][kk + kh];
#pragma unroll
            for (int j = 0; j < NB; ++j) b[j] = Bs[b_base + j * 32 + r32][kk + kh];
#pragma unroll
            for (int j = 0; j < MA; ++j)
#pragma unroll
                for (int i = 0; i < NB; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[i], acc[j][i], 0, 0, 0);
        }
        __syncthreads();
    }
}

// C/D map of a 32 x 32 block: column (B row) = lane & 31, row (A row) of accumulator register `reg` on half-wave kh = lane >> 5
__device__ inline int sim_cd_row(int reg, int kh) { return (reg & 3) + 8 * (reg >> 2) + 4 * kh; }

}  // namespace glove
