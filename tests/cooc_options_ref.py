"""NumPy restatement of include/glove_cooc_options_hip.h and of the preprocessing options of trainer.cooccur: the keep
rule's hash in uint64 arithmetic, the token filter, the subsampling thresholds, the three window weightings — from a key
table, and by brute force from a token list — and NumpyBackend, the backend of tests/cooc_stream_ref.py with
`token_filter` and a `cooc_finalize` that takes `weighting` (the product backend is GloveHip)."""
import numpy as np

import cooc_stream_ref

GOLDEN_GAMMA, MUL_A, MUL_B = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
KEEP_ALWAYS = 0xFFFFFFFF
WEIGHTINGS = ("harmonic", "uniform", "dynamic")


def hash_u(seed, p):
    """u(seed, p) of the header for an array of positions: uint32, all arithmetic mod 2^64."""
    with np.errstate(over="ignore"):
        x = np.asarray(p).astype(np.uint64) + np.uint64(((int(seed) + 1) * GOLDEN_GAMMA) & 0xFFFFFFFFFFFFFFFF)
        x ^= x >> np.uint64(30)
        x *= np.uint64(MUL_A)
        x ^= x >> np.uint64(27)
        x *= np.uint64(MUL_B)
        x ^= x >> np.uint64(31)
    return (x >> np.uint64(32)).astype(np.uint32)


def keep_mask(ids, pos0, thresholds, seed):
    """The keep decision of every token of a block whose first token has the global position pos0."""
    ids = np.asarray(ids, np.int64)
    thr = np.asarray(thresholds, np.uint32)[ids]
    p = np.uint64(pos0) + np.arange(len(ids), dtype=np.uint64)
    return (thr == np.uint32(KEEP_ALWAYS)) | (hash_u(seed, p) < thr)


def token_filter(ids, pos0, thresholds, seed):
    """The survivors, in stream order."""
    ids = np.asarray(ids, np.int32)
    return ids[keep_mask(ids, pos0, thresholds, seed)]


def thresholds(counts, T, delete_unknown=False):
    """uint32 [V] from the ids' stream counts: 0xFFFFFFFF where q = sqrt(T / f) >= 1 (and everywhere for T = 0),
    otherwise floor(q 2^32), f = count / total in float64; thresholds[0] = 0 with delete_unknown."""
    counts = np.asarray(counts, np.int64)
    total = float(counts.sum())
    out = []
    for c in counts.tolist():
        q = 1.0 if (T == 0 or c == 0) else float(np.sqrt(np.float64(T) / (np.float64(c) / np.float64(total))))
        out.append(KEEP_ALWAYS if q >= 1.0 else min(int(np.floor(np.float64(q) * 4294967296.0)), KEEP_ALWAYS))
    out = np.asarray(out, np.uint32)
    if delete_unknown:
        out[0] = 0
    return out


def keep_probability(thresholds_):
    """q of every id, as the table realises it."""
    t = np.asarray(thresholds_, np.uint32).astype(np.float64)
    return np.where(t == KEEP_ALWAYS, 1.0, t / 4294967296.0)


def _values(n_by_distance, context, weighting):
    """value of every pair from its int64 counts per distance, n_by_distance [pairs, context] (column k - 1)."""
    n = np.asarray(n_by_distance, np.int64)
    if weighting == "uniform":
        return n.sum(axis=1).astype(np.float64)
    if weighting == "dynamic":
        w = np.arange(context, 0, -1, dtype=np.int64)               # context - k + 1 for k = 1 .. context
        return (n * w).sum(axis=1).astype(np.float64) / np.float64(context)
    assert weighting == "harmonic", weighting
    val = np.zeros(len(n), np.float64)
    for k in range(1, context + 1):                                 # k ascending from 0.0; absent distances add nothing
        present = n[:, k - 1] > 0
        val = np.where(present, val + n[:, k - 1].astype(np.float64) / np.float64(k), val)
    return val


def finalize_weighted(keys, counts, V, context, min_count=0, weighting="harmonic"):
    """(row int32, col int32, count int64, value float64) of a key table in (row, col) order, count >= min_count only."""
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int64)
    uab, inv = np.unique(keys // context, return_inverse=True)
    n = np.zeros((len(uab), context), np.int64)
    np.add.at(n, (inv, keys % context), counts)
    cnt = n.sum(axis=1)
    keep = cnt >= min_count
    return ((uab[keep] // V).astype(np.int32), (uab[keep] % V).astype(np.int32), cnt[keep], _values(n, context, weighting)[keep])


def brute_force_table(tokens, V, context, min_count=0, weighting="harmonic"):
    """The same table straight from a token list: every position pair (p, p + k), k = 1 .. context, of distinct tokens
    counts once for (a, b) and once for (b, a) at distance k.  No keys, no chunks."""
    tok = [int(t) for t in tokens]
    n = {}
    for p, a in enumerate(tok):
        for k in range(1, context + 1):
            if p + k >= len(tok):
                break
            b = tok[p + k]
            if a == b:
                continue
            for pair in ((a, b), (b, a)):
                n.setdefault(pair, [0] * context)[k - 1] += 1
    pairs = sorted(n)
    table = np.asarray([n[pair] for pair in pairs], np.int64).reshape(len(pairs), context)
    cnt = table.sum(axis=1)
    keep = cnt >= min_count
    row = np.asarray([a for a, _ in pairs], np.int32)[keep]
    col = np.asarray([b for _, b in pairs], np.int32)[keep]
    return row, col, cnt[keep], _values(table, context, weighting)[keep]


class NumpyBackend(cooc_stream_ref.NumpyBackend):
    """tests/cooc_stream_ref.py's backend with the two operations the preprocessing options add."""

    def token_filter(self, ids, pos0, thresholds_, seed):
        return token_filter(ids, pos0, thresholds_, seed)

    def cooc_finalize(self, keys, counts, V, context, min_count=0, weighting="harmonic"):
        if weighting == "harmonic":
            return cooc_stream_ref.finalize(keys, counts, V, context, min_count)
        return finalize_weighted(keys, counts, V, context, min_count, weighting)
