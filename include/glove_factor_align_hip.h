/*
 * glove_factor_align_hip.h — the fourth header of libglove_factor_hip.so: the d x d cross-covariance of gathered row
 * pairs of two dense tables on the MI355X (gfx950).  What fitting an orthogonal map between two embedding spaces on
 * anchor pairs needs (orthogonal Procrustes: trainer.align).  The three older headers stay as they are; the entry points
 * below are versioned by GLOVE_FACTOR_ALIGN_ABI_VERSION.
 *
 * Conventions (as glove_factor_dense_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known sizes (n, d);
 *   - no float atomics: every sum below has a stated order and is bitwise repeatable.
 *
 * Tables are dense [V, d] float32 with row stride d, d % 4 == 0, 4 <= d <= 1024, zero padding columns, rows 16-B aligned.
 * The chunks and slices are those of glove_factor_dense_hip.h, counted over the PAIRS: GLOVE_GRAM_CHUNK consecutive pairs
 * from pair 0 on, GLOVE_GRAM_SLICE pairs = 16 chunks.  Both constants are part of the bits here too.
 */
#ifndef GLOVE_FACTOR_ALIGN_HIP_H
#define GLOVE_FACTOR_ALIGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "glove_factor_dense_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_FACTOR_ALIGN_ABI_VERSION 1

int glove_factor_align_abi_version(void);

/* The workspace of glove_cross_gram_f64: a pure host function, 0 for sizes the call would refuse.
 * ceil(n / GLOVE_GRAM_SLICE) slots of d * d doubles (the slice partials), rounded up to 256 B and never less than 256 B. */
size_t glove_cross_gram_workspace_bytes(int64_t n, int32_t d);

/* M[i][j] = sum over the pairs p of x~[p, i] y~[p, j], with
 *     x~[p, i] = X[xid[p], i] x_scale[xid[p]]   one float32 product, rounded (X[xid[p], i] itself when x_scale is null),
 *     y~[p, j] = Y[yid[p], j] y_scale[yid[p]]   likewise.
 * X [Vx, d] and Y [Vy, d] float32 with the same row stride d; xid, yid [n] int32 ids into them, which may repeat and come
 * in any order (checking them is the caller's job); x_scale [Vx], y_scale [Vy] float32 or null, each on its own.
 * M_out [d, d] float64, row stride d.  The summation order is glove_gram_f64's with the pair index in place of the row,
 * every (i, j) on its own:
 *   - a chunk's partial is a float32 chain s = fmaf(x~[p, i], y~[p, j], s) over the chunk's pairs in ascending order,
 *     starting from 0 (on gfx950: v_mfma_f32_32x32x2_f32, the same chain bit for bit);
 *   - a slice's partial starts at 0.0 and adds its chunk partials in chunk order, in float64;
 *   - M[i][j] starts at 0.0 and adds the slice partials in slice order, in float64, by a second launch.
 * So the bits of M are a function of the operands alone, not of the grid.  Every (i, j) is computed: M is not symmetric.
 * With Y == X, identity ids and null scales M is glove_gram_f64(X, null) bit for bit.  Padding columns give exact zeros.
 *   1 <= n <= 2^31 - 1;  4 <= d <= 1024, d % 4 == 0;  Vx, Vy >= 1. */
int glove_cross_gram_f64(const float *X, int32_t Vx, const float *Y, int32_t Vy, int32_t d, const int32_t *xid,
                         const int32_t *yid, int64_t n, const float *x_scale /* [Vx] or null */,
                         const float *y_scale /* [Vy] or null */, double *M_out /* [d, d] */, void *ws, size_t ws_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_FACTOR_ALIGN_HIP_H */
