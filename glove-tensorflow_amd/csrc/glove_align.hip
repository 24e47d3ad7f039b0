// The cross-covariance of gathered row pairs of two dense tables on gfx950: the fourth object of
// libglove_factor_hip.so, include/glove_factor_align_hip.h (the semantics, the limits and the summation order are
// stated there).
//
//   glove_cross_gram_f64   M = X~^T Y~ in float64 from float32 chunk chains on v_mfma_f32_32x32x2_f32, the rows of both
//                          operands gathered through id lists and scaled per row.  Two launches: (slice, pair of
//                          64-column blocks (bi, bj), all nb x nb of them) per workgroup, then the slices.
//
// The shape is gram_slice_kernel's (glove_pca.hip): the contraction runs over the pairs, so the MFMA's k index is the
// pair; lane (r, h) of a wave feeds column r of the A block (of X~) and column r of the B block (of Y~) of pair k + h,
// both read from a row-major LDS slab.  A workgroup holds a slab of kGramRows pairs of two 64-column blocks (32 KB) and
// its four waves own the four 32 x 32 tiles of the 64 x 64 block of M.  Which tiles share a workgroup does not enter the
// bits: every (i, j) is one chain per chunk.
#include "glove_sim_gemm.h"
#include "../../include/glove_factor_align_hip.h"

namespace glove {

constexpr int kGramChunk = GLOVE_GRAM_CHUNK;
constexpr int kGramSlice = GLOVE_GRAM_SLICE;
constexpr int kGramCols = 64;              // columns of a block: 2 x 2 tiles of 32 per workgroup
constexpr int kGramRows = 64;              // pairs of a slab
constexpr int kGramSlabsPerChunk = kGramChunk / kGramRows;
static_assert(kGramSlice % kGramChunk == 0 && kGramChunk % kGramRows == 0, "a slice is whole chunks, a chunk whole slabs");

__host__ __device__ inline int64_t gram_slices(int64_t n) { return (n + kGramSlice - 1) / kGramSlice; }

// ---- the slice partial of one pair of column blocks
__global__ __launch_bounds__(kBlock) void cross_gram_slice_kernel(const float *__restrict__ X, const float *__restrict__ Y,
                                                                  int d, const int32_t *__restrict__ xid,
                                                                  const int32_t *__restrict__ yid, int64_t n,
                                                                  const float *__restrict__ x_scale,
                                                                  const float *__restrict__ y_scale, int nb,
                                                                  double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float As[kGramRows][kGramCols];
    __shared__ __attribute__((aligned(16))) float Bs[kGramRows][kGramCols];
    const int pairs = nb * nb;
    const int64_t slice = blockIdx.x / pairs;
    const int bi = (blockIdx.x % pairs) / nb, bj = (blockIdx.x % pairs) % nb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1, r32 = lane & 31, kh = lane >> 5;
    // loads: 16 float4 per slab row and operand; this thread's quad of columns and its first pair of the slab
    constexpr int kQuads = kGramCols / 4, kPer = kGramRows * kQuads / kBlock, kStep = kBlock / kQuads;
    const int q = threadIdx.x % kQuads, r0 = threadIdx.x / kQuads;
    const int ca = bi * kGramCols + q * 4, cb = bj * kGramCols + q * 4;
    const int64_t p_beg = slice * kGramSlice, p_end = p_beg + kGramSlice < n ? p_beg + kGramSlice : n;
    // Three stages in flight: the ids of slab s + 2, the rows (and their scales) of slab s + 1, the MFMAs of slab s.  A row's
    // address needs its id, so the ids go one slab ahead of the rows; the rows are issued before this slab's MFMAs and used
    // after them.  The scale is multiplied in on the way into LDS, not behind the load, where the wave would wait for
    // the load on the spot (the comment on the mean in gram_slice_kernel has the measurement).
    int32_t ia[kPer], ib[kPer];
    f4 an[kPer], bn[kPer];
    float sa[kPer], sb[kPer];
    auto fetch_ids = [&](int64_t p0) {
#pragma unroll
        for (int x = 0; x < kPer; ++x) {
            const int64_t p = p0 + r0 + x * kStep;
            ia[x] = p < p_end ? xid[p] : -1;
            ib[x] = p < p_end ? yid[p] : -1;
        }
    };
    auto fetch_rows = [&]() {
#pragma unroll
        for (int x = 0; x < kPer; ++x) {
            an[x] = f4{0.f, 0.f, 0.f, 0.f};
            bn[x] = f4{0.f, 0.f, 0.f, 0.f};
            sa[x] = sb[x] = 0.f;
            if (ia[x] >= 0) {                                  // (a pair that is none: zeros)
                if (ca < d) an[x] = *reinterpret_cast<const f4 *>(X + (size_t)ia[x] * d + ca);
                if (cb < d) bn[x] = *reinterpret_cast<const f4 *>(Y + (size_t)ib[x] * d + cb);
                if (x_scale) sa[x] = x_scale[ia[x]];
                if (y_scale) sb[x] = y_scale[ib[x]];
            }
        }
    };
    f32x16 acc;
    double dacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; dacc[i] = 0.0; }
    fetch_ids(p_beg);
    fetch_rows();
    fetch_ids(p_beg + kGramRows);
    int slab = 0;
    for (int64_t p0 = p_beg; p0 < p_end; p0 += kGramRows, ++slab) {
#pragma unroll
        for (int x = 0; x < kPer; ++x) {                       // x~ = one float32 product, rounded; the row itself without a scale
            *reinterpret_cast<f4 *>(&As[r0 + x * kStep][q * 4]) = x_scale ? an[x] * sa[x] : an[x];
            *reinterpret_cast<f4 *>(&Bs[r0 + x * kStep][q * 4]) = y_scale ? bn[x] * sb[x] : bn[x];
        }
        __syncthreads();
        const bool last = p0 + kGramRows >= p_end;
        if (!last) {
            fetch_rows();
            fetch_ids(p0 + 2 * kGramRows);
        }
#pragma unroll 8
        for (int kk = 0; kk < kGramRows; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + kh][wi * 32 + r32], Bs[kk + kh][wj * 32 + r32], acc, 0, 0, 0);
        __syncthreads();
        if (last || slab % kGramSlabsPerChunk == kGramSlabsPerChunk - 1) {      // the chunk's chain ends: float64 from here
#pragma unroll
            for (int i = 0; i < 16; ++i) { dacc[i] += (double)acc[i]; acc[i] = 0.f; }
        }
    }
    double *out = part + (size_t)slice * d * d;
    const int j = bj * kGramCols + wj * 32 + r32;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = bi * kGramCols + wi * 32 + sim_cd_row(reg, kh);
        if (i < d && j < d) out[(size_t)i * d + j] = dacc[reg];
    }
}

// M[i][j] = the slice partials of (i, j) in slice order
__global__ __launch_bounds__(kBlock) void cross_gram_combine_kernel(const double *__restrict__ part, int64_t slices, int d,
                                                                    double *__restrict__ M)
{
    const int dd = d * d;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < dd; idx += gridDim.x * kBlock) {
        double s = 0.0;
        for (int64_t sl = 0; sl < slices; ++sl) s += part[(size_t)sl * dd + idx];
        M[idx] = s;
    }
}

static bool align_sizes_ok(int64_t n, int32_t d) { return n >= 1 && n <= INT32_MAX && d >= 4 && d <= 1024 && d % 4 == 0; }

static size_t cross_gram_ws_bytes(int64_t n, int32_t d)
{
    const size_t bytes = align_up((size_t)gram_slices(n) * (size_t)d * (size_t)d * sizeof(double), 256);
    return bytes < 256 ? 256 : bytes;
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_factor_align_abi_version(void) { return GLOVE_FACTOR_ALIGN_ABI_VERSION; }

size_t glove_cross_gram_workspace_bytes(int64_t n, int32_t d)
{
    if (!align_sizes_ok(n, d)) return 0;
    return cross_gram_ws_bytes(n, d);
}

int glove_cross_gram_f64(const float *X, int32_t Vx, const float *Y, int32_t Vy, int32_t d, const int32_t *xid,
                         const int32_t *yid, int64_t n, const float *x_scale, const float *y_scale, double *M_out, void *ws,
                         size_t ws_bytes, void *stream)
{
    if (!align_sizes_ok(n, d) || Vx < 1 || Vy < 1 || !X || !Y || !xid || !yid || !M_out || !ws) return GLOVE_E_BADARG;
    if (cross_gram_ws_bytes(n, d) > ws_bytes) return GLOVE_E_WORKSPACE;
    const int64_t slices = gram_slices(n);
    const int nb = (d + kGramCols - 1) / kGramCols;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cross_gram_slice_kernel, dim3((unsigned)(slices * nb * nb)), dim3(kBlock), 0, st, X, Y, (int)d, xid, yid,
                       n, x_scale, y_scale, nb, (double *)ws);
    hipLaunchKernelGGL(cross_gram_combine_kernel, dim3(blocks_for((int64_t)d * d, kBlock)), dim3(kBlock), 0, st,
                       (const double *)ws, slices, (int)d, M_out);
    return (int)hipGetLastError();
}

}  // extern "C"
