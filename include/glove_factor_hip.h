/*
 * glove_factor_hip.h — C ABI of libglove_factor_hip.so: what a count-based baseline (truncated SVD of the PPMI, log or
 * square-root co-occurrence matrix: the GloVe paper's SVD / SVD-S / SVD-L rows; Levy, Goldberg & Dagan 2015) needs on
 * the MI355X (gfx950).  A library of its own: training, evaluation and data preparation never load it, and
 * glove_hip.h stays as it is.  The entry points below are versioned by GLOVE_FACTOR_ABI_VERSION.
 *
 * Conventions (as glove_eval_cluster_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known bounds (n_rows, n_cols, nnz, l), never from counts the device
 *     computed;
 *   - fp32 arithmetic (float64 where a call says so), int32 ids (0 <= id < bound; checking them is the caller's job:
 *     the kernels do not look), dense row stride l % 4 == 0 with zero padding columns, rows 16-B aligned.
 *
 * The sparse matrix is CSR: row_ptr int64[n_rows + 1] with row_ptr[0] == 0, row_ptr[n_rows] == nnz and no descent;
 * the positions of row i are row_ptr[i] .. row_ptr[i + 1] - 1 in ascending order, col_idx int32[nnz], val float[nnz].
 * The columns of a row need not be sorted and one column may appear more than once.
 *
 * Limits of every CSR call: 1 <= n_rows <= 2^31 - 1; 1 <= n_cols <= 2^31 - 1; 0 <= nnz <= 2^31 - 1;
 * l % 4 == 0 and 4 <= l <= 1024.
 *
 * Chunks.  A row of more than GLOVE_FACTOR_CHUNK nonzeros is cut into chunks of GLOVE_FACTOR_CHUNK consecutive
 * positions counted from the row's first one (the last chunk shorter); a shorter row is one chunk.  One lane group
 * (spmm) or one wave (row sums) sums one chunk, so its work is bounded by the chunk length whatever the row's length —
 * the rows of a count-sorted vocabulary are Zipf-skewed, the first ones hold a nonzero in almost every column.
 */
#ifndef GLOVE_FACTOR_HIP_H
#define GLOVE_FACTOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_FACTOR_ABI_VERSION 1

#define GLOVE_FACTOR_CHUNK 512      /* nonzeros of a chunk: part of the bits of every sum below */

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / l % 4 != 0 / unknown kind */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

/* glove_coo_reweight_f32's `kind` */
#define GLOVE_REWEIGHT_NONE  0
#define GLOVE_REWEIGHT_SQRT  1
#define GLOVE_REWEIGHT_LOG1P 2
#define GLOVE_REWEIGHT_PPMI  3

int glove_factor_abi_version(void);

/* The workspace of glove_csr_spmm_f32 (l >= 4) and of glove_csr_row_sums_f64 (l == 0, where n_rows and nnz alone
 * count): a pure host function, 0 for sizes the calls would refuse.  It holds the chunk sums of the rows of more than
 * GLOVE_FACTOR_CHUNK nonzeros: 2 ceil(nnz / GLOVE_FACTOR_CHUNK) slots of l floats (row sums: of one double), rounded up
 * to 256 B and never less than 256 B.  Chunk c of a row whose first position is a lies in slot
 * 2 (a / GLOVE_FACTOR_CHUNK + c) + (c > 0), integer division: no two chunks share a slot, and no count has to come back
 * from the device to size it. */
size_t glove_csr_spmm_workspace_bytes(int32_t n_rows, int64_t nnz, int32_t l);

/* Y[i] = sum over the positions p of row i of val[p] B[col_idx[p]], B [n_cols, l] and Y_out [n_rows, l] dense rows of
 * stride l.  A row without nonzeros is written as zeros by the kernel itself (Y_out needs no clearing); a column that
 * appears twice in a row is added twice.  A^T Q is this call on the transposed CSR.  Y_out must not alias B.
 *
 * No float atomics; the bits of Y[i] are a function of row i's positions, val and B alone — not of the grid, of the
 * other rows or of n_rows.  The summation order, every column on its own:
 *   - a chunk's sum starts from 0 and takes its positions one by one in ascending order, s = fma(val[p], B[col][k], s);
 *   - a row of one chunk is that chunk's sum;
 *   - a longer row is the sum of its chunk sums in chunk order, starting from chunk 0's and adding the others one by
 *     one (plain additions), by a second launch.
 * One lane group (16, 32 or 64 lanes by l, one float4 to four per lane) sums one chunk with four partner rows in
 * flight; the groups of a wave hold different short rows.
 * nnz == 0 writes n_rows rows of zeros. */
int glove_csr_spmm_f32(const int64_t *row_ptr, const int32_t *col_idx, const float *val, int32_t n_rows, int32_t n_cols,
                       int64_t nnz, const float *B /* [n_cols, l] */, int32_t l, float *Y_out /* [n_rows, l] */,
                       void *ws, size_t ws_bytes, void *stream);

/* sums_out[i] = the sum of val over row i's positions in float64 (0.0 for a row without nonzeros): the marginals; the
 * column marginals are this call on the transposed CSR.  Bitwise repeatable, in this order:
 *   - lane j of the 64 of a wave adds the chunk's positions j, j + 64, j + 128, ... (counted from the chunk's first) in
 *     ascending order, starting from 0.0;
 *   - the 64 lane sums are combined by a butterfly: x += x of lane ^ 32, then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
 *   - a row of one chunk is that chunk's sum; the chunk sums of a longer row are summed the same way (lane j takes
 *     chunks j, j + 64, ...) by a second launch.
 * ws: glove_csr_spmm_workspace_bytes(n_rows, nnz, 0). */
int glove_csr_row_sums_f64(const int64_t *row_ptr, const float *val, int32_t n_rows, int64_t nnz,
                           double *sums_out /* [n_rows] */, void *ws, size_t ws_bytes, void *stream);

/* The entrywise transform of a COO table, val_out[p] = f(x = val_in[p]) computed in float64 and rounded to f32 once:
 *   GLOVE_REWEIGHT_NONE   x
 *   GLOVE_REWEIGHT_SQRT   sqrt(x)
 *   GLOVE_REWEIGHT_LOG1P  log1p(x)
 *   GLOVE_REWEIGHT_PPMI   max(0, log(x * total / (row_sums[row[p]] * col_weights[col[p]])) - log_shift)
 * and 0 wherever x <= 0 (or x is a NaN).  For context-distribution smoothing (Levy et al. 2015) the caller passes
 * col_weights[j] = c_j^alpha and total = sum_j c_j^alpha; alpha = 1 is plain PMI; log_shift = log(k) is the shifted
 * PPMI of k negative samples.  row, col, row_sums and col_weights are read for GLOVE_REWEIGHT_PPMI only (and may be
 * null otherwise).  val_out may alias val_in.  0 <= nnz <= 2^31 - 1; nnz == 0 returns 0 without a launch. */
int glove_coo_reweight_f32(const int32_t *row, const int32_t *col, const float *val_in, int64_t nnz, int32_t kind,
                           const double *row_sums, const double *col_weights, double total, double log_shift,
                           float *val_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_FACTOR_HIP_H */
