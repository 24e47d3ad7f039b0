/*
 * glove_factor_graph_hip.h — the third header of libglove_factor_hip.so: one relaxation sweep over the rows of a dense
 * [n, d] table along the edges of a sparse n x n graph, on the MI355X (gfx950).  What retrofitting word vectors to a
 * semantic lexicon needs (Faruqui et al., NAACL 2015: trainer.retrofit).  glove_factor_hip.h and
 * glove_factor_dense_hip.h stay as they are; the entry points below are versioned by GLOVE_FACTOR_GRAPH_ABI_VERSION.
 *
 * Conventions (as glove_factor_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: the grid is sized from n_list, a host-known size;
 *   - no float atomics, no fences: every sum below has a stated order and is bitwise repeatable.
 *
 * The graph is CSR as in glove_factor_hip.h: row_ptr int64[n + 1] with row_ptr[0] == 0, row_ptr[n] == nnz and no
 * descent; the positions of row i are row_ptr[i] .. row_ptr[i + 1] - 1 in ascending order; col_idx int32[nnz] need not
 * be sorted inside a row and one column may appear more than once (it is then added more than once).  The graph is
 * square: rows and columns are ids of the same table.  beta float[nnz] holds one weight per position; a null beta
 * stands for a weight of 1 everywhere.
 *
 * A dense table is [n, d] float32 with row stride d, d % 4 == 0, 4 <= d <= 1024, zero padding columns (what
 * trainer.hip_api.row_width produces), rows 16-B aligned.
 */
#ifndef GLOVE_FACTOR_GRAPH_HIP_H
#define GLOVE_FACTOR_GRAPH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_FACTOR_GRAPH_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 / aliasing */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_factor_graph_abi_version(void);

/* The retrofitting update of the listed rows: row i of Q_out becomes the weighted mean of its own row of Q_hat (the
 * vectors as they were trained, weight alpha times the row's weight sum) and of the rows of Q_in its positions name
 * (weight beta).  rows int32[n_list] lists the ids to update; a null rows stands for 0 .. n - 1 and requires
 * n_list == n.  A row that is not listed is not touched.
 *
 * Limits: 1 <= n <= 2^31 - 1; 0 <= nnz <= 2^31 - 1; 0 <= n_list <= n (n_list == 0 returns 0 without a launch);
 * d % 4 == 0 and 4 <= d <= 1024; alpha finite and >= 0.  Q_out must not be Q_hat.  Q_out == Q_in IS allowed: that is
 * the in-place (Gauss-Seidel) sweep, under the contract below.
 *
 * The update of a listed row i with positions a .. b - 1, every column k on its own, in this order (it is the bits):
 *   1. s = 0; for p = a .. b - 1 ascending, s = fmaf(beta[p], Q_in[col_idx[p]][k], s)   (beta[p] = 1 for a null beta);
 *   2. w = 0; over the same positions, w = w + beta[p] in float32;
 *   3. t = alpha * w (one float32 multiply, not fused with what follows), num = fmaf(t, Q_hat[i][k], s), den = t + w;
 *   4. Q_out[i][k] = num / den, the correctly rounded IEEE float32 quotient.
 * With alpha = 1 and a null beta this is Faruqui's (n_i q^_i + sum_j q_j) / (2 n_i).
 *   - A listed row without positions, or with w == 0, is COPIED from Q_in: an out-of-place call over all rows leaves no
 *     row of Q_out unwritten.
 *   - No id causes an access out of bounds: a listed id outside [0, n) is skipped; a column outside [0, n) adds nothing
 *     to s and nothing to w (and is not loaded); a row whose row_ptr leaves [0, nnz] or descends counts as empty.
 *   - Padding columns (zero in Q_hat and Q_in) give exact zeros.
 * The bits of Q_out[i] are a function of row i's positions, beta, alpha, Q_hat[i] and the rows of Q_in it names — not
 * of the grid, of the list or of n_list.
 *
 * Contract for in-place calls (Q_out == Q_in); the kernel does not look.  No listed row may be a column of
 * ANOTHER listed row: a row that is written in a call is read by no other row of that call.  A row that
 * lists ITSELF is fine: a lane group has read its own row's float4s before it stores them.  The level schedule of
 * trainer.retrofit.level_schedule cuts the rows into lists that keep this contract and whose calls, one after the
 * other, give the bits of a scalar loop over the ids 0, 1, 2, ...
 *
 * One lane group (16, 32 or 64 lanes by d, one float4 to four per lane: the shapes of glove_csr_spmm_f32) updates one
 * listed row with four partner rows in flight; the groups of a wave hold different rows.  Rows are NOT chunked: a row
 * is one chain whatever its length, so a row of thousands of positions serialises one lane group. */
int glove_retrofit_rows_f32(const int64_t *row_ptr, const int32_t *col_idx, const float *beta /* [nnz] or null: all 1 */,
                            int32_t n, int64_t nnz,
                            const int32_t *rows /* [n_list] or null: rows 0 .. n-1, n_list == n */, int32_t n_list,
                            const float *Q_hat /* [n, d] */, const float *Q_in /* [n, d] */, float *Q_out /* [n, d] */,
                            int32_t d, float alpha, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_FACTOR_GRAPH_HIP_H */
