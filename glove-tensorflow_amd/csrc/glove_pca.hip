// Contractions over the ROWS of a dense [n, d] table on gfx950: the second object of libglove_factor_hip.so,
// include/glove_factor_dense_hip.h (the semantics, the limits and the summation orders are stated there).
//
//   glove_col_sums_f64        column sums in float64.  Two launches: (slice, 32 columns) per workgroup, then the slices.
//   glove_gram_f64            X~^T X~ in float64 from float32 chunk chains on v_mfma_f32_32x32x2_f32.  Two launches:
//                             (slice, pair of 64-column blocks bi <= bj) per workgroup, then the slices and the mirror.
//   glove_rows_transform_f32  X T^T - shift on the tile loop of the similarity GEMMs (glove_sim_gemm.h).
//
// The Gram matrix contracts over rows, so the MFMA's k index is the table row: lane (r, h) of a wave feeds column r of
// the A block and column r of the B block of table row k + h, both read from a row-major LDS slab (a half-wave reads 32
// consecutive floats).  A workgroup holds a slab of kGramRows rows of two 64-column blocks (32 KB) and
// its four waves own the four 32 x 32 tiles of the 64 x 64 block of G; on a diagonal block the tile below the diagonal
// is not computed.  Which tiles share a workgroup does not enter the bits: every (i, j) is one chain per chunk.
#include "glove_sim_gemm.h"
#include "../../include/glove_factor_dense_hip.h"

namespace glove {

constexpr int kGramChunk = GLOVE_GRAM_CHUNK;
constexpr int kGramSlice = GLOVE_GRAM_SLICE;
constexpr int kGramCols = 64;              // columns of a block: 2 x 2 tiles of 32 per workgroup
constexpr int kGramRows = 64;              // rows of a slab
constexpr int kGramSlabsPerChunk = kGramChunk / kGramRows;
static_assert(kGramSlice % kGramChunk == 0 && kGramChunk % kGramRows == 0, "a slice is whole chunks, a chunk whole slabs");
constexpr int kSumCols = 32;               // columns of a column-sum workgroup: one 128-B line per row
constexpr int kSumLanes = kBlock / (kSumCols / 4);      // row lanes: 32
constexpr int kXfRows = 128, kXfCols = 64; // the transform's tile: 128 table rows x 64 rows of T

__host__ __device__ inline int64_t gram_slices(int64_t n) { return (n + kGramSlice - 1) / kGramSlice; }

// ---- column sums
__global__ __launch_bounds__(kBlock) void colsum_slice_kernel(const float *__restrict__ X, int64_t n, int d, int groups,
                                                              double *__restrict__ part)
{
    __shared__ double red[kSumLanes][kSumCols + 1];
    const int64_t slice = blockIdx.x / groups;
    const int c0 = (blockIdx.x % groups) * kSumCols;
    const int q = threadIdx.x % (kSumCols / 4), r = threadIdx.x / (kSumCols / 4);
    const int col = c0 + q * 4;
    const int64_t v_beg = slice * kGramSlice, v_end = v_beg + kGramSlice < n ? v_beg + kGramSlice : n;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (col < d) {
        constexpr int U = 8;               // rows in flight per thread
        const float *p = X + col;
        int64_t v = v_beg + r;
        for (; v + (int64_t)(U - 1) * kSumLanes < v_end; v += (int64_t)U * kSumLanes) {
            f4 x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = *reinterpret_cast<const f4 *>(p + (size_t)(v + (int64_t)u * kSumLanes) * d);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[0] += (double)x[u].x; s[1] += (double)x[u].y; s[2] += (double)x[u].z; s[3] += (double)x[u].w;
            }
        }
        for (; v < v_end; v += kSumLanes) {
            const f4 x = *reinterpret_cast<const f4 *>(p + (size_t)v * d);
            s[0] += (double)x.x; s[1] += (double)x.y; s[2] += (double)x.z; s[3] += (double)x.w;
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) red[r][q * 4 + c] = s[c];
    __syncthreads();
    if (threadIdx.x < kSumCols && c0 + threadIdx.x < d) {
        double t = 0.0;
        for (int lane = 0; lane < kSumLanes; ++lane) t += red[lane][threadIdx.x];
        part[(size_t)slice * d + c0 + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(kBlock) void colsum_combine_kernel(const double *__restrict__ part, int64_t slices, int d,
                                                                double *__restrict__ sums)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= d) return;
    double s = 0.0;
    for (int64_t sl = 0; sl < slices; ++sl) s += part[(size_t)sl * d + k];
    sums[k] = s;
}

// ---- the Gram matrix: the slice partial of one pair of column blocks
__global__ __launch_bounds__(kBlock) void gram_slice_kernel(const float *__restrict__ X, int64_t n, int d,
                                                            const float *__restrict__ mean, int nb, int pairs,
                                                            double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float As[kGramRows][kGramCols];
    __shared__ __attribute__((aligned(16))) float Bs[kGramRows][kGramCols];
    const int64_t slice = blockIdx.x / pairs;
    int p = blockIdx.x % pairs, bi = 0;
    while (p >= nb - bi) { p -= nb - bi; ++bi; }           // pairs in the order (0, 0), (0, 1), ..., (1, 1), ...
    const int bj = bi + p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = wave >> 1, wj = wave & 1, r32 = lane & 31, kh = lane >> 5;
    const bool active = !(bi == bj && wi > wj);            // the tile below the diagonal is its mirror's copy
    // loads: 16 float4 per slab row and operand; this thread's quad of columns and its first row
    constexpr int kQuads = kGramCols / 4, kPer = kGramRows * kQuads / kBlock, kStep = kBlock / kQuads;
    const int q = threadIdx.x % kQuads, r0 = threadIdx.x / kQuads;
    const int ca = bi * kGramCols + q * 4, cb = bj * kGramCols + q * 4;
    f4 ma = {0.f, 0.f, 0.f, 0.f}, mb = {0.f, 0.f, 0.f, 0.f};
    if (mean) {
        if (ca < d) ma = *reinterpret_cast<const f4 *>(mean + ca);
        if (cb < d) mb = *reinterpret_cast<const f4 *>(mean + cb);
    }
    const int64_t v_beg = slice * kGramSlice, v_end = v_beg + kGramSlice < n ? v_beg + kGramSlice : n;
    // The next slab's loads are issued before this slab's MFMAs and used after them.  The mean is subtracted on the way
    // into LDS, not behind the load: a subtraction there made the wave wait for the load on the spot (1.30 ms instead of
    // 0.73 at V = 400 k, d = 320; a second register set, two slabs ahead, measured 0.75: DESIGN.md §3k).  A diagonal pair
    // reads its one block once and takes both operands from As.
    const bool diag = bi == bj;
    f4 an[kPer], bn[kPer];
    auto fetch = [&](int64_t v0) {
#pragma unroll
        for (int x = 0; x < kPer; ++x) {
            const int64_t v = v0 + r0 + x * kStep;
            an[x] = f4{0.f, 0.f, 0.f, 0.f};
            bn[x] = f4{0.f, 0.f, 0.f, 0.f};
            if (v < v_end) {
                if (ca < d) an[x] = *reinterpret_cast<const f4 *>(X + (size_t)v * d + ca);
                if (cb < d && !diag) bn[x] = *reinterpret_cast<const f4 *>(X + (size_t)v * d + cb);
            }
        }
    };
    const float (*Bop)[kGramCols] = diag ? As : Bs;
    f32x16 acc;
    double dacc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; dacc[i] = 0.0; }
    fetch(v_beg);
    int slab = 0;
    for (int64_t v0 = v_beg; v0 < v_end; v0 += kGramRows, ++slab) {
#pragma unroll
        for (int x = 0; x < kPer; ++x) {
            const bool row = v0 + r0 + x * kStep < v_end;      // (x~ of a row that is none: 0, not -mean; ma, mb are 0 beyond d)
            *reinterpret_cast<f4 *>(&As[r0 + x * kStep][q * 4]) = row ? an[x] - ma : f4{0.f, 0.f, 0.f, 0.f};
            if (!diag) *reinterpret_cast<f4 *>(&Bs[r0 + x * kStep][q * 4]) = row ? bn[x] - mb : f4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const bool last = v0 + kGramRows >= v_end;
        if (!last) fetch(v0 + kGramRows);
        if (active) {
#pragma unroll 8
            for (int kk = 0; kk < kGramRows; kk += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + kh][wi * 32 + r32], Bop[kk + kh][wj * 32 + r32], acc, 0, 0, 0);
        }
        __syncthreads();
        if (last || slab % kGramSlabsPerChunk == kGramSlabsPerChunk - 1) {      // the chunk's chain ends: float64 from here
#pragma unroll
            for (int i = 0; i < 16; ++i) { dacc[i] += (double)acc[i]; acc[i] = 0.f; }
        }
    }
    if (!active) return;
    double *out = part + (size_t)slice * d * d;
    const int j = bj * kGramCols + wj * 32 + r32;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int i = bi * kGramCols + wi * 32 + sim_cd_row(reg, kh);
        if (i < d && j < d) out[(size_t)i * d + j] = dacc[reg];
    }
}

// G[i][j] = the slice partials of (min, max) in slice order: the upper triangle and its copy
__global__ __launch_bounds__(kBlock) void gram_combine_kernel(const double *__restrict__ part, int64_t slices, int d,
                                                              double *__restrict__ G)
{
    const int dd = d * d;
    for (int idx = blockIdx.x * kBlock + threadIdx.x; idx < dd; idx += gridDim.x * kBlock) {
        const int i = idx / d, j = idx % d;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        double s = 0.0;
        for (int64_t sl = 0; sl < slices; ++sl) s += part[(size_t)sl * dd + (size_t)lo * d + hi];
        G[idx] = s;
    }
}

// ---- Y = X T^T - shift: workgroup = 128 table rows x 64 rows of T, a wave owns 32 table rows and both blocks of T rows
__global__ __launch_bounds__(kBlock) void rows_transform_kernel(const float *__restrict__ X, int64_t n, int d,
                                                                const float *__restrict__ T, int m, int jtiles,
                                                                const float *__restrict__ shift, float *__restrict__ Y)
{
    __shared__ float Xs[kXfRows][kSimK + 1];
    __shared__ float Ts[kXfCols][kSimK + 1];
    const int64_t v0 = (int64_t)(blockIdx.x / jtiles) * kXfRows;
    const int j0 = (blockIdx.x % jtiles) * kXfCols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r32 = lane & 31, kh = lane >> 5;
    f32x16 acc[1][2];
    sim_tile_gemm(Xs, Ts, acc, X, T, d, [&](int row) -> int32_t { return v0 + row < n ? (int32_t)(v0 + row) : -1; },
                  [&](int row) -> int32_t { return j0 + row < m ? j0 + row : -1; }, wave * 32, 0, 0);
    // C/D map: column = row of T, row = table row
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int j = j0 + b * 32 + r32;
        if (j >= m) continue;
        const float sh = shift ? shift[j] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t v = v0 + wave * 32 + sim_cd_row(reg, kh);
            if (v < n) Y[(size_t)v * m + j] = shift ? acc[0][b][reg] - sh : acc[0][b][reg];
        }
    }
}

static bool dense_sizes_ok(int64_t n, int32_t d) { return n >= 1 && n <= INT32_MAX && d >= 4 && d <= 1024 && d % 4 == 0; }

static size_t gram_ws_bytes(int64_t n, int32_t d)
{
    const size_t bytes = align_up((size_t)gram_slices(n) * (size_t)d * (size_t)d * sizeof(double), 256);
    return bytes < 256 ? 256 : bytes;
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_factor_dense_abi_version(void) { return GLOVE_FACTOR_DENSE_ABI_VERSION; }

size_t glove_gram_workspace_bytes(int64_t n, int32_t d)
{
    if (!dense_sizes_ok(n, d)) return 0;
    return gram_ws_bytes(n, d);
}

int glove_col_sums_f64(const float *X, int64_t n, int32_t d, double *sums_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!dense_sizes_ok(n, d) || !X || !sums_out || !ws) return GLOVE_E_BADARG;
    if (gram_ws_bytes(n, d) > ws_bytes) return GLOVE_E_WORKSPACE;
    const int64_t slices = gram_slices(n);
    const int groups = (d + kSumCols - 1) / kSumCols;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_slice_kernel, dim3((unsigned)(slices * groups)), dim3(kBlock), 0, st, X, n, (int)d, groups,
                       (double *)ws);
    hipLaunchKernelGGL(colsum_combine_kernel, dim3((unsigned)((d + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       (const double *)ws, slices, (int)d, sums_out);
    return (int)hipGetLastError();
}

int glove_gram_f64(const float *X, int64_t n, int32_t d, const float *mean, double *G_out, void *ws, size_t ws_bytes,
                   void *stream)
{
    if (!dense_sizes_ok(n, d) || !X || !G_out || !ws) return GLOVE_E_BADARG;
    if (gram_ws_bytes(n, d) > ws_bytes) return GLOVE_E_WORKSPACE;
    const int64_t slices = gram_slices(n);
    const int nb = (d + kGramCols - 1) / kGramCols, pairs = nb * (nb + 1) / 2;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gram_slice_kernel, dim3((unsigned)(slices * pairs)), dim3(kBlock), 0, st, X, n, (int)d, mean, nb, pairs,
                       (double *)ws);
    hipLaunchKernelGGL(gram_combine_kernel, dim3(blocks_for((int64_t)d * d, kBlock)), dim3(kBlock), 0, st, (const double *)ws,
                       slices, (int)d, G_out);
    return (int)hipGetLastError();
}

int glove_rows_transform_f32(const float *X, int64_t n, int32_t d, const float *T, int32_t m, const float *shift,
                             float *Y_out, void *stream)
{
    if (!dense_sizes_ok(n, d) || !dense_sizes_ok(1, m) || !X || !T || !Y_out || Y_out == X) return GLOVE_E_BADARG;
    const int64_t vtiles = (n + kXfRows - 1) / kXfRows;
    const int jtiles = (m + kXfCols - 1) / kXfCols;
    hipLaunchKernelGGL(rows_transform_kernel, dim3((unsigned)(vtiles * jtiles)), dim3(kBlock), 0, (hipStream_t)stream, X, n,
                       (int)d, T, (int)m, jtiles, shift, Y_out);
    return (int)hipGetLastError();
}

}  // extern "C"
