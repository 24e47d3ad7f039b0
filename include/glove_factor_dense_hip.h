/*
 * glove_factor_dense_hip.h — the second header of libglove_factor_hip.so: contractions over the ROWS of a dense [n, d]
 * table on the MI355X (gfx950) — column sums, the d x d Gram / covariance matrix and the product with a small [m, d]
 * matrix.  What post-processing a finished embedding table needs (all-but-the-top, Mu & Viswanath 2018; PCA reduction,
 * Raunak et al. 2019: trainer.postprocess).  glove_factor_hip.h stays as it is; the entry points below are versioned by
 * GLOVE_FACTOR_DENSE_ABI_VERSION.
 *
 * Conventions (as glove_factor_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known sizes (n, d, m);
 *   - no float atomics: every sum below has a stated order and is bitwise repeatable.
 *
 * A dense table is [n, d] float32 with row stride d, d % 4 == 0, 4 <= d <= 1024, zero padding columns (what
 * trainer.hip_api.row_width produces), rows 16-B aligned; 1 <= n <= 2^31 - 1.
 *
 * Chunks and slices.  The rows are cut into chunks of GLOVE_GRAM_CHUNK consecutive rows counted from row 0 (the last
 * one shorter) and into slices of GLOVE_GRAM_SLICE rows = 16 chunks.  Both constants are part of the bits.
 */
#ifndef GLOVE_FACTOR_DENSE_HIP_H
#define GLOVE_FACTOR_DENSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_FACTOR_DENSE_ABI_VERSION 1

#define GLOVE_GRAM_CHUNK 1024       /* rows of a chunk: one float32 fmaf chain */
#define GLOVE_GRAM_SLICE 16384      /* rows of a slice: 16 chunk partials added in float64 */

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 / aliasing */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_factor_dense_abi_version(void);

/* The workspace of glove_col_sums_f64 and of glove_gram_f64: a pure host function, 0 for sizes the calls would refuse.
 * ceil(n / GLOVE_GRAM_SLICE) slots of d * d doubles (the Gram call's slice partials; the column sums keep d doubles per
 * slice at its start), rounded up to 256 B and never less than 256 B. */
size_t glove_gram_workspace_bytes(int64_t n, int32_t d);

/* sums_out[k] = the sum of column k over the n rows, in float64.  Bitwise repeatable, in this order:
 *   - row lane r (0 .. 31) of a slice adds the slice's rows r, r + 32, r + 64, ... in ascending order, starting from 0.0;
 *   - a slice's sum adds its 32 lane sums in lane order, starting from 0.0;
 *   - sums_out[k] adds the slice sums in slice order, starting from 0.0, by a second launch. */
int glove_col_sums_f64(const float *X /* [n, d] */, int64_t n, int32_t d, double *sums_out /* [d] */,
                       void *ws, size_t ws_bytes, void *stream);

/* G[i][j] = sum over the rows v of x~[v, i] x~[v, j], x~[v, i] = the float32 difference X[v, i] - mean[i] (x~ = X when
 * mean is null); mean float32 [d].  G_out [d, d] float64, row stride d.  The summation order, every (i, j) on its own:
 *   - a chunk's partial is a float32 chain s = fmaf(x~[v, i], x~[v, j], s) over the chunk's rows in ascending order,
 *     starting from 0 (on gfx950: v_mfma_f32_32x32x2_f32, the same chain bit for bit);
 *   - a slice's partial starts at 0.0 and adds its chunk partials in chunk order, in float64;
 *   - G[i][j] starts at 0.0 and adds the slice partials in slice order, in float64, by a second launch.
 * So the bits of G are a function of X, mean, n and d alone: not of the grid, not of how tiles are grouped into
 * workgroups.  Only i <= j is computed; G[j][i] is its copy, and fmaf(a, b, c) == fmaf(b, a, c), so G is exactly
 * symmetric.  Padding columns (zero in X and in mean) give exact zeros. */
int glove_gram_f64(const float *X /* [n, d] */, int64_t n, int32_t d, const float *mean /* [d] or null */,
                   double *G_out /* [d, d] */, void *ws, size_t ws_bytes, void *stream);

/* Y[v, j] = dot(X[v], T[j]) - shift[j] (no subtraction when shift is null): T [m, d] float32 with row stride d,
 * shift float32 [m], Y_out [n, m] float32 with row stride m; m % 4 == 0, 4 <= m <= 1024.  Y_out must not alias X.
 * The dot product is a float32 chain s = fmaf(X[v, k], T[j, k], s) over k = 0, 1, ..., d - 1 starting from 0 (the tile
 * loop of the similarity GEMMs, v_mfma_f32_32x32x2_f32); the shift is subtracted once, after the last column. */
int glove_rows_transform_f32(const float *X /* [n, d] */, int64_t n, int32_t d, const float *T /* [m, d] */, int32_t m,
                             const float *shift /* [m] or null */, float *Y_out /* [n, m] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_FACTOR_DENSE_HIP_H */
