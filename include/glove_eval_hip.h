/*
 * glove_eval_hip.h — C ABI of libglove_eval_hip.so: intrinsic evaluation of finished GloVe embeddings on the
 * MI355X (gfx950).  A library of its own beside glove_hip.h, which is the ABI of the training hot path: scoring
 * embeddings is not on that path.  The reference (yxtay/glove-tensorflow) has no such step; the semantics are those of
 * the word-analogy test of GloVe's eval/python/evaluate.py and of gensim's most_similar (3CosAdd).
 *
 * Conventions (as glove_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph;
 *   - fp32 arithmetic, int32 ids (0 <= id < V), row stride d % 4 == 0 with zero padding columns, rows 16-B aligned.
 */
#ifndef GLOVE_EVAL_HIP_H
#define GLOVE_EVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_EVAL_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_eval_abi_version(void);

/* Word analogies a : b :: c : ?, 3CosAdd.  With w^_v = W[v] / sqrt(max(|W[v]|^2, 1e-12)) (the l2_normalize clamp of
 * the PREDICT path), question q = (a, b, c) has the query  x = w^_b - w^_a + w^_c  and every vocabulary row the score
 *     score(v) = x . w^_v / sqrt(max(|x|^2, 1e-12));
 * the candidates are all v in [0, V) except a, b and c (which may repeat among themselves).  sims_out / idx_out [n,k]
 * hold the k best per question in descending score, ties to the lower id first (tf.math.top_k, the PREDICT path).
 *   W    [V,d], d = row stride in floats (a multiple of 4 up to 1024; padding columns zero)
 *   abc  [n,3] int32 ids in [0, V): checking them is the caller's job
 *   1 <= k <= min(V - 3, 1024): at least k candidates remain, so an excluded id never reaches the output
 *   0 <= n <= 65535 * 128; n == 0 returns 0 without a launch
 * The scores are an n x V matrix in the workspace (the similarity GEMM runs on the matrix cores in exact f32, the
 * top-k is the staged selection of glove_topk_cosine_f32): callers with many questions walk them in batches.
 * ws: glove_analogy_workspace_bytes(n, V, d, k) bytes (a pure host function; 0 for sizes the call would refuse). */
size_t glove_analogy_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t k);
int glove_analogy_topk_f32(const float *W, int32_t V, int32_t d, const int32_t *abc, int32_t n, int32_t k,
                           float *sims_out, int32_t *idx_out, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_EVAL_HIP_H */
