"""NumPy restatement of include/glove_cooc_stream_hip.h: a chunk's keys, the merge of two key tables, and the
(row, col, count, value) table of a key table — np.unique and integer sums; the value loop in float64, k ascending from
0.0, as the header states it.  NumpyBackend wraps the three as the backend trainer.cooccur.CoocAccumulator drives (the
product backend is GloveHip)."""
import numpy as np


def chunk_keys(tokens, n_own, V, context):
    """(keys int64 ascending, counts int64): both orientations of every pair (p, p + k), p < n_own, k in 1 .. context,
    p + k < len(tokens), tokens[p] != tokens[p + k]; key = (a V + b) context + (k - 1)."""
    tok = np.asarray(tokens, np.int64)
    n_total = len(tok)
    keys = []
    for k in range(1, context + 1):
        m = min(n_own, n_total - k)
        if m <= 0:
            break
        a, b = tok[:m], tok[k:k + m]
        keep = a != b
        a, b = a[keep], b[keep]
        keys += [(a * V + b) * context + (k - 1), (b * V + a) * context + (k - 1)]
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    uk, cnt = np.unique(keys, return_counts=True)
    return uk.astype(np.int64), cnt.astype(np.int64)


def merge(keys_a, counts_a, keys_b, counts_b):
    """The ascending union of two strictly ascending tables; counts of shared keys summed in int64."""
    keys = np.concatenate([np.asarray(keys_a, np.int64), np.asarray(keys_b, np.int64)])
    counts = np.concatenate([np.asarray(counts_a, np.int64), np.asarray(counts_b, np.int64)])
    uk, inv = np.unique(keys, return_inverse=True)
    out = np.zeros(len(uk), np.int64)
    np.add.at(out, inv, counts)
    return uk, out


def finalize(keys, counts, V, context, min_count=0):
    """(row int32, col int32, count int64, value float64) in (row, col) order, count >= min_count only;
    value = sum_k (double)n_k / (double)k, k ascending, starting from 0.0."""
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int64)
    ab = keys // context
    k = keys % context + 1
    uab, inv = np.unique(ab, return_inverse=True)
    cnt = np.zeros(len(uab), np.int64)
    np.add.at(cnt, inv, counts)
    val = np.zeros(len(uab), np.float64)
    for dist in range(1, context + 1):          # keys ascend, so within one (a, b) the distances do: add them in that order
        sel = k == dist
        term = np.zeros(len(uab), np.float64)
        term[inv[sel]] = counts[sel].astype(np.float64) / np.float64(dist)
        present = np.zeros(len(uab), bool)
        present[inv[sel]] = True
        val = np.where(present, val + term, val)
    keep = cnt >= min_count
    return (uab[keep] // V).astype(np.int32), (uab[keep] % V).astype(np.int32), cnt[keep], val[keep]


class NumpyBackend:
    """The three operations of a CoocAccumulator backend on numpy arrays (no `device`: tokens stay where they are)."""

    def cooc_chunk_keys(self, tokens, n_own, V, context):
        return chunk_keys(tokens, n_own, V, context)

    def cooc_merge(self, keys_a, counts_a, keys_b, counts_b, keys_out=None, counts_out=None):
        keys, counts = merge(keys_a, counts_a, keys_b, counts_b)
        if keys_out is None:
            return keys, counts
        assert len(keys) <= len(keys_out) == len(counts_out), "the accumulator sized its buffer for both inputs"
        assert not np.shares_memory(keys_out, keys_a) and not np.shares_memory(keys_out, keys_b)
        keys_out[:len(keys)] = keys
        counts_out[:len(keys)] = counts
        return keys_out[:len(keys)], counts_out[:len(keys)]

    def cooc_finalize(self, keys, counts, V, context, min_count=0):
        return finalize(keys, counts, V, context, min_count)
