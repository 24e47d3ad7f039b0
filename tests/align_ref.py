"""TEST-ONLY NumPy restatement of the three definitions trainer.align stands on (include/glove_factor_align_hip.h,
include/glove_eval_cross_hip.h), as plain functions for the kernel tests and as a backend of align_tables /
translation_precision; and the cases the tests share.  Never imported by the product.

The float64 mode is the reference: sums and products in float64, but what the headers define in float32 is float32 here
too: the scaled row x~ = X[id] * scale[id] is one float32 product, a CSLS penalty is a float32 sum in position order
divided once in float32, and the penalties enter the score as those float32 numbers.  The float32 mode keeps the tables
and the results of the products in float32 (NumPy's own float32 matrix products): the rounding level a float32
implementation has whatever its summation order, what the driver test measures the device against."""
import numpy as np
import torch

import pca_ref

EPS = 1e-12                     # tf.math.l2_normalize's clamp, as in the PREDICT path


# ---- 1. the cross-covariance of gathered row pairs
def scaled_rows(X, ids, scale=None):
    """x~ [n, d] IN THE TABLE'S TYPE: the gathered rows times their scales, one product each."""
    X = np.asarray(X)
    ids = np.asarray(ids, np.int64)
    return X[ids] if scale is None else X[ids] * np.asarray(scale, X.dtype)[ids, None]


def cross_gram(X, xid, Y, yid, x_scale=None, y_scale=None):
    """M = X~^T Y~, every product and sum in float64."""
    return scaled_rows(X, xid, x_scale).astype(np.float64).T @ scaled_rows(Y, yid, y_scale).astype(np.float64)


def cross_gram_magnitude(X, xid, Y, yid, x_scale=None, y_scale=None):
    """sum over the pairs of |x~_i y~_j|: what the rounding bound of a chain scales with."""
    return np.abs(scaled_rows(X, xid, x_scale).astype(np.float64)).T @ np.abs(scaled_rows(Y, yid, y_scale).astype(np.float64))


# ---- 2. cosines across two tables, CSLS, top-k
def inv_norms(W, dtype=np.float64):
    W = np.asarray(W, dtype)
    return 1.0 / np.sqrt(np.maximum((W * W).sum(1), dtype(EPS)))


def scores(Q, qid, T, q_pen=None, t_pen=None, dtype=np.float64):
    """[n, Vt]: cos(Q[qid[q]], T[v]), or 2 cos - q_pen[q] - t_pen[v] (the penalties as given, float32 numbers)."""
    Q, T = np.asarray(Q, dtype), np.asarray(T, dtype)
    qid = np.asarray(qid, np.int64)
    if (q_pen is None) != (t_pen is None):
        raise ValueError("both penalty arrays or neither")
    c = ((Q[qid] @ T.T) * inv_norms(Q[qid], dtype)[:, None]) * inv_norms(T, dtype)[None, :]
    if q_pen is None:
        return c
    return (dtype(2.0) * c - np.asarray(q_pen, dtype)[:, None]) - np.asarray(t_pen, dtype)[None, :]


def topk(Q, qid, T, k, q_pen=None, t_pen=None, extra=0, dtype=np.float64):
    """(scores [n, k + extra], idx [n, k + extra]): descending, ties to the lower id (a stable sort of the negated scores).
    `extra`: further ranks behind the k-th, for the gap of the last rank to the next one."""
    s = scores(Q, qid, T, q_pen, t_pen, dtype)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k + extra]
    return np.take_along_axis(s, order, 1), order.astype(np.int32)


def topk_mean(sims):
    """float32: s = s + sims[:, j] for j = 0, 1, ... from 0, then one division by float32(k)."""
    sims = np.asarray(sims, np.float32)
    s = np.zeros(sims.shape[0], np.float32)
    for j in range(sims.shape[1]):
        s = (s + sims[:, j]).astype(np.float32)
    return (s / np.float32(sims.shape[1])).astype(np.float32)


def csls_penalty(A, ids, B, knn=10):
    """The float32 mean of the knn best float64 cosines of each A[ids] row against B, rounded to float32 first."""
    return topk_mean(topk(A, ids, B, knn)[0].astype(np.float32))


# ---- 3. the fit and the scoring, spelled out without the driver
def procrustes_map(X, xid, Y, yid, unit=True):
    """W float64 = V U^T of M = U S V^T, M the float64 cross-covariance of the (unit-length) anchor rows."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    a, b = X[np.asarray(xid, np.int64)], Y[np.asarray(yid, np.int64)]
    if unit:
        a, b = a * inv_norms(a)[:, None], b * inv_norms(b)[:, None]
    U, _, Vt = np.linalg.svd(a.T @ b)
    return Vt.T @ U.T


def precision_at(A, T, pairs, top_k=(1, 5, 10), method="nn", knn=10, penalty_rows=None):
    """MUSE's word-translation precision in float64: {k: share of the distinct source ids with a gold target in the top k}."""
    A, T = np.asarray(A, np.float64), np.asarray(T, np.float64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    queries = sorted(set(pairs[:, 0].tolist()))
    gold = {s: {t for s2, t in pairs.tolist() if s2 == s} for s in queries}
    q_pen = t_pen = None
    if method == "csls":
        q_pen = csls_penalty(A, queries, T, knn)
        t_pen = csls_penalty(T, np.arange(len(T)), A[:penalty_rows], knn)
    idx = topk(A, queries, T, max(top_k), q_pen, t_pen)[1]
    return {k: sum(any(v in gold[s] for v in row[:k]) for row, s in zip(idx.tolist(), queries)) / len(queries) for k in top_k}


# ---- the backend
class NumpyBackend(pca_ref.NumpyBackend):
    """align_tables' and translation_precision's backend on the CPU: torch tensors in and out, NumPy inside
    (rows_transform is pca_ref's)."""

    def cross_gram(self, X, xid, Y, yid, x_scale=None, y_scale=None, ws=None):
        sc = lambda s: None if s is None else s.numpy()
        if self._np is np.float64:
            return torch.from_numpy(cross_gram(X.numpy(), xid.numpy(), Y.numpy(), yid.numpy(), sc(x_scale), sc(y_scale)))
        a, b = scaled_rows(X.numpy(), xid.numpy(), sc(x_scale)), scaled_rows(Y.numpy(), yid.numpy(), sc(y_scale))
        return torch.from_numpy((a.T @ b).astype(np.float64))                  # a float32 product

    def cross_topk(self, Q, qid, T, k, q_pen=None, t_pen=None, batch=1024):
        pen = lambda p: None if p is None else p.numpy()
        s, i = topk(Q.numpy(), qid.numpy(), T.numpy(), k, pen(q_pen), pen(t_pen), dtype=self._np)
        return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i)

    def topk_mean(self, sims):
        return torch.from_numpy(topk_mean(sims.numpy()))


# ---- the cases the tests share
def planted_rotation(seed=0, V=500, d=20, noise=0.0):
    """(X [V, d], Y = X Q^T + noise N(0, 1) [V, d], Q orthogonal [d, d]) in float64: Y's rows are X's rotated by Q."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((V, d))
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    Y = X @ Q.T
    if noise:
        Y = Y + noise * rng.standard_normal((V, d))
    return X, Y, Q


def hub_case(seed=0, n=40, d=64):
    """(A [n, d], T [n + 1, d], pairs): the queries are a cluster (a unit centre plus 0.5 N(0, I / d)), query i's planted
    partner is target i = the query plus 0.7 N(0, I / d) (cosine about 0.85), and target n is a hub, the queries' mean
    (cosine about 0.89 to every query): nearest neighbours answer the hub, whose target-side penalty (about 0.9 against
    a partner's 0.75) CSLS takes off again."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(d)
    centre /= np.linalg.norm(centre)
    A = centre + 0.5 * rng.standard_normal((n, d)) / np.sqrt(d)
    partners = A + 0.7 * rng.standard_normal((n, d)) / np.sqrt(d)
    T = np.concatenate([partners, A.mean(axis=0)[None, :]])
    pairs = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)
    return A, T, pairs
