/*
 * glove_eval_sim_hip.h — second header of libglove_eval_hip.so: 3CosMul word analogies and the cosine of word pairs
 * (word-similarity datasets) on the MI355X (gfx950).  glove_eval_hip.h (3CosAdd) stays as it is and keeps its own
 * version; the entry points below are versioned by GLOVE_EVAL_SIM_ABI_VERSION.  The semantics are those of Levy &
 * Goldberg's 3CosMul (gensim most_similar_cosmul) and of gensim's evaluate_word_pairs.
 *
 * Conventions (as glove_eval_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph;
 *   - fp32 arithmetic, int32 ids (0 <= id < V, checking them is the caller's job), row stride d % 4 == 0 up to 1024
 *     with zero padding columns, rows 16-B aligned.
 */
#ifndef GLOVE_EVAL_SIM_HIP_H
#define GLOVE_EVAL_SIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_EVAL_SIM_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 / eps out of range */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_eval_sim_abi_version(void);

/* The cosine both entry points use.  With inv_norm[x] = 1 / sqrt(max(|W[x]|^2, 1e-12)) (the l2_normalize clamp of the
 * PREDICT path),
 *     cos(x, v) = clamp((W[x] . W[v]) inv_norm[x] inv_norm[v], -1, 1);
 * the clamp is there because a float32 cosine can overshoot +-1 by an ulp.
 *
 * Word analogies a : b :: c : ?, 3CosMul.  With s(x, v) = (1 + cos(x, v)) / 2 every vocabulary row has the score
 *     score(v) = s(b, v) s(c, v) / (s(a, v) + eps);
 * the candidates are all v in [0, V) except a, b and c (which may repeat among themselves).  sims_out / idx_out [n,k]
 * hold the k best per question in descending score, ties to the lower id first (tf.math.top_k).
 *   W    [V,d]
 *   abc  [n,3] int32 ids in [0, V)
 *   1 <= k <= min(V - 3, 1024): at least k candidates remain, so an excluded id never reaches the output
 *   0 <= n <= 65535 * 128; n == 0 returns 0 without a launch (the sizes and eps are checked first)
 *   eps  finite and in (0, 1] (the paper's 1e-3, gensim's 1e-6): with the clamp no denominator is below eps
 * The three cosines of a (question, v) pair are combined in the epilogue of the similarity GEMM (matrix cores, exact
 * f32): the scores are one n x V matrix in the workspace, no 3n x V matrix exists.  Callers with many questions walk
 * them in batches; a question's scores do not depend on the batch it is in.
 * ws: glove_cosmul_workspace_bytes(n, V, d, k) bytes, a pure host function (0 for sizes the call would refuse).  Layout:
 *     inv_norm[V] | scores[n V] | 2 x (values, ids) of n ceil(V / 4096) k winners of the staged top-k
 * floats / int32, each of the six pieces rounded up to 256 B. */
size_t glove_cosmul_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t k);
int glove_cosmul_topk_f32(const float *W, int32_t V, int32_t d, const int32_t *abc, int32_t n, int32_t k, float eps,
                          float *sims_out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream);

/* cos_out[i] = cos(pairs[i,0], pairs[i,1]) as defined above (word-similarity datasets).  One lane group per pair in a
 * fixed summation order: bitwise repeatable whatever the grid.  n >= 0; n == 0 returns 0 without a launch.  No workspace. */
int glove_pair_cosine_f32(const float *W, int32_t V, int32_t d, const int32_t *pairs /* [n,2] */, int32_t n,
                          float *cos_out /* [n] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_EVAL_SIM_HIP_H */
