/*
 * glove_eval_cross_hip.h — fourth header of libglove_eval_hip.so: nearest neighbours ACROSS two embedding tables on the
 * MI355X (gfx950), by cosine or by CSLS (cross-domain similarity local scaling: Conneau et al. 2018, MUSE), and the mean
 * of a top-k list, which is what a CSLS penalty is.  What trainer.align drives.  The three older headers stay as they
 * are and keep their own versions; the entry points below are versioned by GLOVE_EVAL_CROSS_ABI_VERSION.
 *
 * Conventions (as glove_eval_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph;
 *   - fp32 arithmetic, int32 ids (checking them is the caller's job), row stride d % 4 == 0 up to 1024 with zero padding
 *     columns, rows 16-B aligned.
 */
#ifndef GLOVE_EVAL_CROSS_HIP_H
#define GLOVE_EVAL_CROSS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_EVAL_CROSS_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 / one penalty array without the other */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_eval_cross_abi_version(void);

/* The k rows of T closest to each of n rows of Q.  Q [Vq, d] and T [Vt, d] are two tables of the same row stride d;
 * query q is row qid[q] of Q (0 <= qid[q] < Vq).  With
 *     q_inv[q] = 1 / sqrt(max(|Q[qid[q]]|^2, 1e-12)),  t_inv[v] = 1 / sqrt(max(|T[v]|^2, 1e-12))
 * (the l2_normalize clamp of the PREDICT path),
 *     cos(q, v) = ((Q[qid[q]] . T[v]) q_inv[q]) t_inv[v]:
 * the dot product is a float32 chain s = fmaf(Q[.., c], T[v, c], s) over c = 0, 1, ..., d - 1 starting from 0 (the tile
 * loop of the similarity GEMMs, v_mfma_f32_32x32x2_f32), the two float32 products are taken in that order and there is
 * no clamp to +-1: PREDICT's epilogue, so with Q == T the scores are glove_topk_cosine_f32's bit for bit.
 *   q_pen, t_pen both null:   score(q, v) = cos(q, v)                                    (nearest neighbours)
 *   q_pen [n], t_pen [Vt]:    score(q, v) = ((2.0f cos(q, v)) - q_pen[q]) - t_pen[v]     (CSLS)
 * two float32 subtractions in that order, nothing contracted; q_pen[q] is the mean cosine of query q to its nearest
 * rows of T, t_pen[v] that of T[v] to its nearest rows of the query side (glove_topk_mean_f32 of the two top-k lists).
 * One of them null and the other not is GLOVE_E_BADARG.
 * sims_out / idx_out [n, k] hold the k best per query in descending score, ties to the lower id first (tf.math.top_k,
 * the staged selection of the PREDICT path).
 *   1 <= k <= min(Vt, 1024);  0 <= n <= 65535 * 128;  n == 0 returns 0 without a launch, after the size checks.
 * The scores are an n x Vt matrix in the workspace: callers with many queries walk them in batches.
 * ws: glove_cross_topk_workspace_bytes(n, Vt, d, k) bytes (a pure host function; 0 for sizes the call would refuse),
 * laid out as  q_inv[n] | t_inv[Vt] | scores[n Vt] | the two ping-pong buffers of the top-k stages,  each piece rounded
 * up to 256 B. */
size_t glove_cross_topk_workspace_bytes(int32_t n, int32_t Vt, int32_t d, int32_t k);
int glove_cross_topk_f32(const float *Q, int32_t Vq, const int32_t *qid, int32_t n, const float *T, int32_t Vt, int32_t d,
                         int32_t k, const float *q_pen, const float *t_pen, float *sims_out, int32_t *idx_out,
                         void *ws, size_t ws_bytes, void *stream);

/* mean_out[q] = the mean of row q of sims [n, k]: a float32 sum s = s + sims[q, j] over j = 0, 1, ..., k - 1 starting
 * from 0, then one IEEE division by (float)k.  One thread per row, no workspace.  n >= 0 (n == 0 returns 0 without a
 * launch), k >= 1. */
int glove_topk_mean_f32(const float *sims /* [n, k] */, int32_t n, int32_t k, float *mean_out /* [n] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_EVAL_CROSS_HIP_H */
