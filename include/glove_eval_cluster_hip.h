/*
 * glove_eval_cluster_hip.h — third header of libglove_eval_hip.so: spherical k-means over the rows of an embedding table
 * on the MI355X (gfx950) — word classes (word2vec's -classes) and concept categorization (AP, BLESS, Battig,
 * ESSLLI-2008: cluster the words of a gold-labelled set, score the clusters' purity).  glove_eval_hip.h and
 * glove_eval_sim_hip.h stay as they are and keep their own versions; the entry points below are versioned by
 * GLOVE_EVAL_CLUSTER_ABI_VERSION.
 *
 * Conventions (as glove_eval_hip.h):
 *   - return 0 on success, otherwise the hipError_t value (never throws, never aborts);
 *     GLOVE_E_* codes (< 0) report argument errors detected on the host before any launch;
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing, clears nothing with
 *     memset nodes, keeps no global state and never synchronizes;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns, so it can be captured
 *     into a hipGraph: grids are sized from host-known bounds, never from counts the device computed;
 *   - fp32 arithmetic, int32 ids (0 <= id < V, checking them is the caller's job), row stride d % 4 == 0 up to 1024
 *     with zero padding columns, rows 16-B aligned.
 *
 * Semantics.  With inv(v) = 1 / sqrt(max(|W[v]|^2, 1e-12)) (the l2_normalize clamp of the PREDICT path) the points are
 *     x_i = W[ids[i]] inv(ids[i]),   i in [0, n)   (ids may repeat),
 * the centroids C [K,d] dense rows of the same stride d as W, cinv(c) their inverse norms under the same clamp.
 *
 * Limits of every call: d % 4 == 0 and 4 <= d <= 1024; V >= 1; 0 <= n <= 65535 * 128; 1 <= K <= 4096.
 */
#ifndef GLOVE_EVAL_CLUSTER_HIP_H
#define GLOVE_EVAL_CLUSTER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLOVE_EVAL_CLUSTER_ABI_VERSION 1

#ifndef GLOVE_E_BADARG
#define GLOVE_E_BADARG   (-1)   /* null pointer / size out of range / d % 4 != 0 / C_out aliases C_in */
#define GLOVE_E_WORKSPACE (-2)  /* workspace too small */
#endif

int glove_eval_cluster_abi_version(void);

/* The one workspace of both calls below: a pure host function, 0 for sizes the calls would refuse.  Layout, int32 /
 * float, each of the seven pieces rounded up to 256 B (T = ceil(n / 2048) tiles, R1 = n / 64 + K, R2 = R1 / 64 + K,
 * integer divisions):
 *     pinv[n] | cinv[K] | hist[T K] | starts[5 (K + 1)] | sorted[n] | sums_a[R1 d] | sums_b[R2 d]
 * assign uses the first two pieces, update the other five; V does not enter the size (the inverse norms are those of
 * the n points, not of the table). */
size_t glove_kmeans_workspace_bytes(int32_t n, int32_t V, int32_t d, int32_t K);

/* Assign.  s(i, c) = (W[ids[i]] . C[c]) inv(ids[i]) cinv(c);  assign_out[i] = argmax_c s(i, c), the scores compared
 * unclamped, ties to the lower c (the order of tf.math.top_k);  cos_out[i] = the winning score clamped to [-1, 1].
 * A zero row scores 0 against every centroid and lands in cluster 0; a zero centroid scores 0 against every point.
 * The similarity GEMM runs on the matrix cores in exact f32 (v_mfma_f32_32x32x2_f32, a k-ordered fma chain); a
 * workgroup owns 128 points, walks the centroid tiles itself and keeps each point's best (score, c) in registers: no
 * n x K matrix goes through memory.  A point's result does not depend on its place in the call or on n.
 * n == 0 returns 0 without a launch (the sizes are checked first). */
int glove_kmeans_assign_f32(const float *W, int32_t V, int32_t d, const int32_t *ids, int32_t n, const float *C, int32_t K,
                            int32_t *assign_out /* [n] */, float *cos_out /* [n] */, void *ws, size_t ws_bytes, void *stream);

/* Update.  sum_c = sum of x_i over { i : assign[i] == c };  C_out[c] = sum_c / sqrt(max(|sum_c|^2, 1e-12));  a cluster
 * without members keeps its row of C_in, copied bit for bit;  counts_out[c] = the cluster's size.  C_out must not
 * alias C_in.  A point whose assign lies outside [0, K) belongs to no cluster.
 *
 * The bits of C_out[c] are a function of W, ids, assign and C_in alone — not of the grid, the call or the other
 * clusters.  No float atomics: the point indices are sorted by cluster with a stable counting sort (a histogram per
 * tile of 2048 points with integer atomics, whose result is order-free; a scan; the rank of a point inside its tile by
 * counting the earlier equal keys), then summed in this fixed order:
 *   - a cluster's members in ascending i;
 *   - split into chunks of 64 consecutive members (the last one shorter); a chunk's sum starts from its first member and
 *     adds the others one by one, in order, every column on its own;
 *   - the chunk sums of a cluster, in chunk order, are again split into chunks of 64 and summed the same way, level
 *     after level until one row is left (a level that finds one row hands it on unchanged, so the number of levels
 *     a call runs — ceil(log64 n), at least one — does not show in the bits);
 *   - |sum_c|^2 is summed as the inverse norm of a table row is.
 * One lane group sums one chunk: its work is bounded by the chunk length whatever the cluster's size.
 * n == 0 returns 0 without a launch and leaves C_out and counts_out untouched (the sizes are checked first). */
int glove_kmeans_update_f32(const float *W, int32_t V, int32_t d, const int32_t *ids, int32_t n, const int32_t *assign,
                            const float *C_in, int32_t K, float *C_out /* [K,d] */, int32_t *counts_out /* [K] */,
                            void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GLOVE_EVAL_CLUSTER_HIP_H */
