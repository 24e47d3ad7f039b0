"""Float64 NumPy restatement of spherical k-means as include/glove_eval_cluster_hip.h defines it — assign (with each
point's margin, best minus second best), update, the driver of GloveHip.kmeans — and of the bookkeeping of
trainer.categorize / trainer.classes: the gold-file format, the lookup, purity, score_file and classes_file.  Written
from the definitions, not from the trainer's code."""
import os
from types import SimpleNamespace

import numpy as np

UNK = "<UNK>"


def inv_norms(M):
    M = np.asarray(M, np.float64)
    return 1.0 / np.sqrt(np.maximum((M * M).sum(axis=1), 1e-12))


def unit_points(W, ids):
    X = np.asarray(W, np.float64)[np.asarray(ids, np.int64)]
    return X * inv_norms(X)[:, None]


def scores(W, ids, C):
    """s(i, c) = (W[ids[i]] . C[c]) inv(ids[i]) cinv(c), unclamped, [n, K]."""
    X = np.asarray(W, np.float64)[np.asarray(ids, np.int64)]
    C = np.asarray(C, np.float64)
    return (X @ C.T) * inv_norms(X)[:, None] * inv_norms(C)[None, :]


def assign(W, ids, C):
    """(assign [n] int32, cos [n] clamped, margin [n]: the best score minus the second best, inf with one centroid).
    np.argmax takes the first of equal scores: ties to the lower c."""
    S = scores(W, ids, C)
    a = S.argmax(axis=1) if len(S) else np.zeros(0, np.int64)
    best = S[np.arange(len(S)), a]
    if S.shape[1] > 1:
        rest = S.copy()
        rest[np.arange(len(S)), a] = -np.inf
        margin = best - rest.max(axis=1)
    else:
        margin = np.full(len(S), np.inf)
    return a.astype(np.int32), np.clip(best, -1.0, 1.0), margin


def update(W, ids, a, C):
    """(C' [K,d] float64, counts [K]): the clusters' summed unit rows over their clamped norms; an empty cluster keeps
    its row of C."""
    C = np.asarray(C, np.float64)
    X = unit_points(W, ids)
    a = np.asarray(a, np.int64)
    out = C.copy()
    counts = np.bincount(a, minlength=len(C)).astype(np.int64)
    sums = np.zeros_like(C)
    np.add.at(sums, a, X)
    for c in np.flatnonzero(counts):
        out[c] = sums[c] / np.sqrt(max(float(sums[c] @ sums[c]), 1e-12))
    return out, counts


def initial_rows(n, K, seed, r):
    return np.sort(np.random.default_rng([seed, r]).choice(n, K, replace=False))


def run(W, ids, C, iterations=100):
    """One run from the centroids C: (assign, cos, centroids that produced them, assign passes, converged, the minimum
    margin over the passes, the objective after every pass)."""
    previous, t, low, objectives = None, 0, np.inf, []
    while True:
        t += 1
        a, cos, margin = assign(W, ids, C)
        low = min(low, margin.min()) if len(margin) else low
        objectives.append(float(cos.sum()))
        converged = previous is not None and np.array_equal(a, previous)
        if converged or t == iterations:
            return SimpleNamespace(assign=a, cos=cos, centroids=C, iterations=t, converged=converged, min_margin=low,
                                   objective=objectives[-1], trace=objectives)
        C, _ = update(W, ids, a, C)
        previous = a


def kmeans(W, ids, K, seed=0, restarts=1, iterations=100, init=None):
    """The driver: the winning run (largest objective, ties to the lower restart) with `objectives` and `assignments` of
    all restarts."""
    runs = []
    for r in range(1 if init is not None else restarts):
        C = np.asarray(init, np.float64) if init is not None else unit_points(W, np.asarray(ids)[initial_rows(len(ids), K, seed, r)])
        runs.append(run(W, ids, C, iterations))
    best = max(range(len(runs)), key=lambda r: (runs[r].objective, -r))
    res = runs[best]
    res.objectives = [x.objective for x in runs]
    res.assignments = [x.assign for x in runs]
    return res


def purity(a, gold):
    """(1 / n) sum over the clusters of max over the categories of |cluster & category|."""
    a = list(np.asarray(a).tolist())
    assert len(a) == len(gold)
    if not a:
        return None
    total = 0
    for cluster in set(a):
        members = [g for x, g in zip(a, gold) if x == cluster]
        total += max(members.count(g) for g in set(members))
    return total / len(a)


def parse(path, lowercase=True, delimiter=None, word_column=1, category_column=2):
    """[(word, category), ...]: blank lines and # lines left out."""
    out = []
    for line in open(path, encoding="utf8").read().split("\n"):
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        f = [x.strip() for x in line.rstrip("\r").split(delimiter)] if delimiter else line.split()
        w = f[word_column - 1]
        out.append((w.lower() if lowercase else w, f[category_column - 1]))
    return out


def lookup(pairs, vocab, restrict=None):
    """(ids, gold, skipped, duplicates)."""
    ids, gold, skipped, duplicates = [], [], 0, 0
    usable = vocab if restrict is None else vocab[:restrict]
    for w, g in pairs:
        if w == UNK or w not in usable:
            skipped += 1
        elif usable.index(w) in ids:
            duplicates += 1
        else:
            ids.append(usable.index(w))
            gold.append(g)
    return ids, gold, skipped, duplicates


def score_file(path, vocab, W, restrict=None, lowercase=True, delimiter=None, word_column=1, category_column=2, clusters=None,
               restarts=10, iterations=100, seed=0, embeddings="row", global_step=0):
    """The record of Estimator.evaluate_categorization on the table W (already the chosen embeddings)."""
    pairs = parse(path, lowercase, delimiter, word_column, category_column)
    ids, gold, skipped, duplicates = lookup(pairs, vocab, restrict)
    W = np.asarray(W)[:restrict] if restrict is not None else np.asarray(W)
    K = len(set(gold)) if clusters is None else clusters
    res = kmeans(W, np.asarray(ids, np.int32), K, seed, restarts, iterations)
    purities = [purity(a, gold) for a in res.assignments]
    return {"global_step": global_step, "embeddings": embeddings, "categories_file": os.path.basename(str(path)),
            "words_total": len(pairs), "words_seen": len(ids), "skipped": skipped, "duplicates": duplicates,
            "categories": len(set(gold)), "clusters": K, "restarts": restarts, "seed": seed, "iterations": res.iterations,
            "converged": bool(res.converged), "objective": res.objective, "purity": purity(res.assign, gold),
            "purity_mean": float(np.mean(purities)), "purity_min": min(purities), "purity_max": max(purities),
            "sizes": np.bincount(res.assign, minlength=K).tolist()}


def classes_file(vocab, W, K, restrict=None, iterations=10, restarts=1, seed=0, embeddings="row", global_step=0):
    """(the lines of classes.txt, the record of Estimator.word_classes) on the table W."""
    W = np.asarray(W)[:restrict] if restrict is not None else np.asarray(W)
    ids = [i for i, w in enumerate(vocab[:len(W)]) if w != UNK]
    res = kmeans(W, np.asarray(ids, np.int32), K, seed, restarts, iterations)
    sizes = np.bincount(res.assign, minlength=K)
    lines = ["%s %d" % (vocab[i], c) for i, c in zip(ids, res.assign.tolist())]
    rec = {"global_step": global_step, "embeddings": embeddings, "words": len(ids), "classes": K, "iterations": res.iterations,
           "converged": bool(res.converged), "objective": res.objective, "empty": int((sizes == 0).sum()),
           "largest": int(sizes.max()), "smallest": int(sizes.min())}
    return lines, rec


def planted(centres=24, per=90, d=64, noise=0.35, seed=77):
    """(W [centres * per, d] float32, gold [n], init [centres, d] float32: one member per centre): unit centres plus
    noise / sqrt(d) per coordinate, shuffled."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((centres, d))
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    gold = np.repeat(np.arange(centres), per)
    W = mu[gold] + noise / np.sqrt(d) * rng.standard_normal((centres * per, d))
    order = rng.permutation(len(gold))
    W, gold = W[order].astype(np.float32), gold[order]
    first = np.array([np.flatnonzero(gold == c)[0] for c in range(centres)])
    return W, gold, W[first].copy()
