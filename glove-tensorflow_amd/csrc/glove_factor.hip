// What a count-based baseline (truncated SVD of a reweighted co-occurrence matrix) needs on gfx950: the one object of
// libglove_factor_hip.so, include/glove_factor_hip.h (the semantics, the limits and the summation orders are stated there).
//
//   glove_csr_spmm_f32       CSR x dense [n_cols, l]: one partner row of l floats gathered per nonzero, the access pattern
//                            of the step's gather passes.  Two launches: the chunks of the rows longer than one chunk,
//                            then every row (a short row summed on the spot, a long one from its chunk sums).
//   glove_csr_row_sums_f64   the marginals in float64, the same two launches with a wave in place of a lane group.
//   glove_coo_reweight_f32   sqrt / log1p / shifted smoothed PPMI, entry by entry in float64.
//
// Nothing here sizes a grid from the device: the chunks of long rows are found through SLOTS.  Cut the positions
// [0, nnz) into tiles of kChunk.  A row of more than kChunk nonzeros that begins inside a tile ends beyond it, so at
// most one long row begins in a tile, and of the later chunks of one long row (kChunk apart) at most one begins in a
// tile: slot 2 t holds the chunk 0 that begins in tile t, slot 2 t + 1 the later chunk that does.  A lane group takes a
// slot, finds the row by bisecting row_ptr (wave-uniform loads, about 20 of them against up to kChunk gathered rows) and
// leaves when the slot is empty — most are.
#include "glove_common.h"
#include "glove_lane_rows.h"
#include "../../include/glove_factor_hip.h"

namespace glove {

constexpr int kChunk = GLOVE_FACTOR_CHUNK;

// the last r in [0, n_rows) with row_ptr[r] <= x (row_ptr[0] == 0 <= x): the row that holds position x when x < nnz
__device__ inline int32_t last_row_at(const int64_t *__restrict__ row_ptr, int32_t n_rows, int64_t x)
{
    int32_t lo = 0, hi = n_rows;
    while (hi - lo > 1) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// The chunk of slot `slot`: positions [beg, end) of a row of more than kChunk nonzeros; false for an empty slot.  A
// row_ptr that leaves [0, nnz] names no chunk (nothing is read outside the arrays whatever the caller handed over).
__device__ inline bool find_chunk(const int64_t *__restrict__ row_ptr, int32_t n_rows, int64_t nnz, int64_t slot,
                                  int64_t &beg, int64_t &end)
{
    const int64_t t0 = (slot >> 1) * kChunk;
    if (t0 >= nnz) return false;
    if (slot & 1) {                       // chunk c >= 1 beginning in the tile: its row holds the positions t0 - 1 and t0
        if (t0 == 0) return false;
        const int32_t r = last_row_at(row_ptr, n_rows, t0);
        const int64_t a = row_ptr[r], b = row_ptr[r + 1];
        if (a < 0 || b > nnz || a >= t0 || b - a <= kChunk) return false;
        beg = a + (t0 - a + kChunk - 1) / kChunk * kChunk;
        if (beg >= b) return false;
        end = beg + kChunk < b ? beg + kChunk : b;
    } else {                              // chunk 0: a long row beginning in the tile is the last row that begins there
        const int32_t r = last_row_at(row_ptr, n_rows, t0 + kChunk - 1);
        const int64_t a = row_ptr[r], b = row_ptr[r + 1];
        if (a < t0 || b > nnz || b - a <= kChunk) return false;
        beg = a;
        end = a + kChunk;
    }
    return true;
}

// slot of chunk c of the long row that begins at position a
__device__ inline int64_t chunk_slot(int64_t a, int64_t c) { return 2 * (a / kChunk + c) + (c > 0); }

// launch 1: the chunk sums of the rows longer than one chunk, one lane group per slot
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void spmm_chunk_kernel(const int64_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col_idx,
                                                            const float *__restrict__ val, int32_t n_rows,
                                                            int32_t n_cols, int64_t nnz, const f4 *__restrict__ B,
                                                            int d4, int64_t n_slots, f4 *__restrict__ part)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR;
    const int64_t slot = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    if (slot >= n_slots) return;
    int64_t beg, end;
    if (!find_chunk(row_ptr, n_rows, nnz, slot, beg, end)) return;
    f4 acc[NV];
    chunk_sum<LPR, NV>(acc, col_idx, val, beg, end, B, d4, n_cols, lg);
    store_dense<LPR, NV>(acc, part + (size_t)slot * d4, d4, lg);
}

// launch 2: every row, one lane group each — a row of one chunk summed here (zeros when it has no nonzeros), a longer
// one from its chunk sums in chunk order
template <int LPR, int NV>
__global__ __launch_bounds__(kBlock) void spmm_rows_kernel(const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col_idx,
                                                           const float *__restrict__ val, int32_t n_rows,
                                                           int32_t n_cols, int64_t nnz, const f4 *__restrict__ B,
                                                           int d4, const f4 *__restrict__ part, f4 *__restrict__ Y)
{
    constexpr int GPB = kBlock / LPR;
    const int lg = threadIdx.x % LPR;
    const int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / LPR;
    if (i >= n_rows) return;
    int64_t a = row_ptr[i], b = row_ptr[i + 1];
    if (a < 0 || b > nnz || b < a) a = b = 0;               // (a row_ptr that leaves [0, nnz]: an empty row)
    f4 acc[NV];
    if (b - a <= kChunk) {
        chunk_sum<LPR, NV>(acc, col_idx, val, a, b, B, d4, n_cols, lg);
    } else {
        const int64_t n_chunks = (b - a + kChunk - 1) / kChunk;
        load_dense<LPR, NV>(acc, part + (size_t)chunk_slot(a, 0) * d4, d4, lg);
#pragma unroll 4
        for (int64_t c = 1; c < n_chunks; ++c) {
            f4 r[NV];
            load_dense<LPR, NV>(r, part + (size_t)chunk_slot(a, c) * d4, d4, lg);
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[k] += r[k];
        }
    }
    store_dense<LPR, NV>(acc, Y + (size_t)i * d4, d4, lg);
}

// ---- row sums in float64: lane j takes x[first + j], x[first + j + 64], ... in order; then the butterfly of the header
__device__ inline double wave_butterfly_f64(double s)
{
#pragma unroll
    for (int dlt = 32; dlt > 0; dlt >>= 1) s += __shfl_xor(s, dlt, 64);
    return s;
}

__device__ inline double wave_chunk_sum_f64(const float *__restrict__ val, int64_t beg, int64_t end, int lane)
{
    double s = 0.0;
    for (int64_t p = beg + lane; p < end; p += 64) s += (double)val[p];
    return wave_butterfly_f64(s);
}

__global__ __launch_bounds__(kBlock) void rowsum_chunk_kernel(const int64_t *__restrict__ row_ptr,
                                                              const float *__restrict__ val, int32_t n_rows, int64_t nnz,
                                                              int64_t n_slots, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (slot >= n_slots) return;
    int64_t beg, end;
    if (!find_chunk(row_ptr, n_rows, nnz, slot, beg, end)) return;
    const double s = wave_chunk_sum_f64(val, beg, end, lane);
    if (lane == 0) part[slot] = s;
}

__global__ __launch_bounds__(kBlock) void rowsum_rows_kernel(const int64_t *__restrict__ row_ptr,
                                                             const float *__restrict__ val, int32_t n_rows, int64_t nnz,
                                                             const double *__restrict__ part, double *__restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (i >= n_rows) return;
    int64_t a = row_ptr[i], b = row_ptr[i + 1];
    if (a < 0 || b > nnz || b < a) a = b = 0;
    double s;
    if (b - a <= kChunk) {
        s = wave_chunk_sum_f64(val, a, b, lane);
    } else {
        const int64_t n_chunks = (b - a + kChunk - 1) / kChunk;
        s = 0.0;
        for (int64_t c = lane; c < n_chunks; c += 64) s += part[chunk_slot(a, c)];
        s = wave_butterfly_f64(s);
    }
    if (lane == 0) sums[i] = s;
}

__global__ __launch_bounds__(kBlock) void reweight_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
                                                          const float *val_in, int64_t nnz, int32_t kind,
                                                          const double *__restrict__ row_sums,
                                                          const double *__restrict__ col_weights, double total,
                                                          double log_shift, float *val_out)
{
    for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * kBlock) {
        const double x = (double)val_in[p];
        double y = 0.0;
        if (x > 0.0) {
            if (kind == GLOVE_REWEIGHT_NONE) y = x;
            else if (kind == GLOVE_REWEIGHT_SQRT) y = sqrt(x);
            else if (kind == GLOVE_REWEIGHT_LOG1P) y = log1p(x);
            else {
                const double pmi = log(x * total / (row_sums[row[p]] * col_weights[col[p]])) - log_shift;
                y = pmi > 0.0 ? pmi : 0.0;                 // (a NaN — a marginal that is not positive — gives 0)
            }
        }
        val_out[p] = (float)y;
    }
}

static bool csr_sizes_ok(int32_t n_rows, int64_t nnz, int32_t l)
{
    if (n_rows < 1 || nnz < 0 || nnz > INT32_MAX) return false;
    return l == 0 || (l >= 4 && l <= 1024 && l % 4 == 0);
}

static int64_t csr_slots(int64_t nnz) { return 2 * ((nnz + kChunk - 1) / kChunk); }

static size_t csr_ws_bytes(int64_t nnz, int32_t l)
{
    const size_t bytes = align_up((size_t)csr_slots(nnz) * (l ? (size_t)l * sizeof(float) : sizeof(double)), 256);
    return bytes < 256 ? 256 : bytes;
}

}  // namespace glove

using namespace glove;

extern "C" {

int glove_factor_abi_version(void) { return GLOVE_FACTOR_ABI_VERSION; }

size_t glove_csr_spmm_workspace_bytes(int32_t n_rows, int64_t nnz, int32_t l)
{
    if (!csr_sizes_ok(n_rows, nnz, l)) return 0;
    return csr_ws_bytes(nnz, l);
}

int glove_csr_spmm_f32(const int64_t *row_ptr, const int32_t *col_idx, const float *val, int32_t n_rows, int32_t n_cols,
                       int64_t nnz, const float *B, int32_t l, float *Y_out, void *ws, size_t ws_bytes, void *stream)
{
    if (!csr_sizes_ok(n_rows, nnz, l) || l == 0 || n_cols < 1) return GLOVE_E_BADARG;
    if (!row_ptr || !B || !Y_out || !ws || Y_out == B || (nnz > 0 && (!col_idx || !val))) return GLOVE_E_BADARG;
    if (csr_ws_bytes(nnz, l) > ws_bytes) return GLOVE_E_WORKSPACE;
    const int d4 = l / 4;
    const RowShape shape = pick_row_shape(d4);
    const int gpb = kBlock / shape.lpr;
    const int64_t n_slots = csr_slots(nnz);
    const unsigned nb_chunks = (unsigned)((n_slots + gpb - 1) / gpb), nb_rows = (unsigned)(((int64_t)n_rows + gpb - 1) / gpb);
    hipStream_t st = (hipStream_t)stream;
#define CALL(LPR, NV)                                                                                                   \
    if (nnz > kChunk)                                                                                                   \
        hipLaunchKernelGGL((spmm_chunk_kernel<LPR, NV>), dim3(nb_chunks), dim3(kBlock), 0, st, row_ptr, col_idx, val,  \
                           n_rows, n_cols, nnz, (const f4 *)B, d4, n_slots, (f4 *)ws);                                  \
    hipLaunchKernelGGL((spmm_rows_kernel<LPR, NV>), dim3(nb_rows), dim3(kBlock), 0, st, row_ptr, col_idx, val, n_rows, \
                       n_cols, nnz, (const f4 *)B, d4, (const f4 *)ws, (f4 *)Y_out)
    GLOVE_DISPATCH_ROW_SHAPE(shape, CALL);
#undef CALL
    return (int)hipGetLastError();
}

int glove_csr_row_sums_f64(const int64_t *row_ptr, const float *val, int32_t n_rows, int64_t nnz, double *sums_out,
                           void *ws, size_t ws_bytes, void *stream)
{
    if (!csr_sizes_ok(n_rows, nnz, 0)) return GLOVE_E_BADARG;
    if (!row_ptr || !sums_out || !ws || (nnz > 0 && !val)) return GLOVE_E_BADARG;
    if (csr_ws_bytes(nnz, 0) > ws_bytes) return GLOVE_E_WORKSPACE;
    constexpr int wpb = kBlock / 64;
    const int64_t n_slots = csr_slots(nnz);
    hipStream_t st = (hipStream_t)stream;
    if (nnz > kChunk)
        hipLaunchKernelGGL(rowsum_chunk_kernel, dim3((unsigned)((n_slots + wpb - 1) / wpb)), dim3(kBlock), 0, st, row_ptr, val,
                           n_rows, nnz, n_slots, (double *)ws);
    hipLaunchKernelGGL(rowsum_rows_kernel, dim3((unsigned)(((int64_t)n_rows + wpb - 1) / wpb)), dim3(kBlock), 0, st, row_ptr,
                       val, n_rows, nnz, (const double *)ws, sums_out);
    return (int)hipGetLastError();
}

int glove_coo_reweight_f32(const int32_t *row, const int32_t *col, const float *val_in, int64_t nnz, int32_t kind,
                           const double *row_sums, const double *col_weights, double total, double log_shift,
                           float *val_out, void *stream)
{
    if (nnz < 0 || nnz > INT32_MAX || kind < GLOVE_REWEIGHT_NONE || kind > GLOVE_REWEIGHT_PPMI) return GLOVE_E_BADARG;
    if (nnz == 0) return 0;
    if (!val_in || !val_out) return GLOVE_E_BADARG;
    if (kind == GLOVE_REWEIGHT_PPMI && (!row || !col || !row_sums || !col_weights)) return GLOVE_E_BADARG;
    hipLaunchKernelGGL(reweight_kernel, dim3(blocks_for(nnz, kBlock * 4)), dim3(kBlock), 0, (hipStream_t)stream, row, col,
                       val_in, nnz, kind, row_sums, col_weights, total, log_shift, val_out);
    return (int)hipGetLastError();
}

}  // extern "C"
