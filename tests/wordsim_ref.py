"""TEST-ONLY restatement of the word-similarity evaluation (trainer.wordsim, Estimator.evaluate_word_pairs) in float64
NumPy and plain Python loops: what tests/test_wordsim.py and tests/test_gpu_wordsim.py compare the product with.  Never
imported by it."""
import math
import os

import numpy as np

import cosmul_ref


def parse(path, lowercase=True, delimiter=None, score_column=3):
    """[(word1, word2, score), ...]; '#' and blank lines skipped, a first line without a number in the score column too."""
    rows, first = [], True
    for lineno, line in enumerate(open(path, encoding="utf8"), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        cols = [c.strip() for c in line.split(delimiter)] if delimiter else line.split()
        try:
            score = float(cols[score_column - 1])
            if not math.isfinite(score):
                raise ValueError
        except (IndexError, ValueError):
            if first:
                first = False
                continue
            raise ValueError("line %d" % lineno)
        first = False
        w1, w2 = cols[0], cols[1]
        rows.append((w1.lower(), w2.lower(), score) if lowercase else (w1, w2, score))
    return rows


def ranks(x):
    """Average ranks, one value at a time: 1 + (values below) + (ties besides itself) / 2."""
    return [1 + sum(b < a for b in x) + (sum(b == a for b in x) - 1) / 2 for a in x]


def pearson(x, y):
    n = len(x)
    if n < 2:
        return None
    mx, my = math.fsum(x) / n, math.fsum(y) / n
    sxy = math.fsum((a - mx) * (b - my) for a, b in zip(x, y))
    sxx, syy = math.fsum((a - mx) ** 2 for a in x), math.fsum((b - my) ** 2 for b in y)
    if sxx == 0 or syy == 0:
        return None
    return sxy / math.sqrt(sxx * syy)


def spearman(x, y):
    return pearson(ranks(list(x)), ranks(list(y)))


def score_file(path, vocab, W, restrict=None, lowercase=True, delimiter=None, score_column=3, embeddings="row",
               global_step=0):
    """The record of wordsim.json from a pairs file, the vocabulary (tokens in id order) and the table W."""
    W = np.asarray(W, np.float64)
    if restrict is not None:
        W, vocab = W[:restrict], vocab[:restrict]
    ids = {}
    for i, t in enumerate(vocab):
        if t != "<UNK>" and t not in ids:
            ids[t] = i
    rows = parse(path, lowercase, delimiter, score_column)
    kept = [(ids[a], ids[b], s) for a, b, s in rows if a in ids and b in ids]
    cos = cosmul_ref.pair_cosine(W, [k[:2] for k in kept]).tolist() if kept else []
    human = [k[2] for k in kept]
    return {"global_step": global_step, "embeddings": embeddings, "pairs_file": os.path.basename(str(path)),
            "pairs_total": len(rows), "pairs_seen": len(kept), "skipped": len(rows) - len(kept),
            "spearman": spearman(cos, human), "pearson": pearson(cos, human)}
