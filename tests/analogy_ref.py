"""TEST-ONLY restatement of the word-analogy evaluation (include/glove_eval_hip.h, trainer.analogy) in float64 NumPy and
plain Python: what tests/test_analogy.py and tests/test_gpu_analogy.py compare the product with.  Never imported by it."""
import numpy as np

EPS = 1e-12                     # tf.math.l2_normalize's clamp, as in the PREDICT path


def scores(W, abc, dtype=np.float64):
    """[n, V] 3CosAdd scores with the three ids of every question at -inf."""
    W = np.asarray(W, dtype)
    abc = np.asarray(abc, np.int64).reshape(-1, 3)
    unit = W / np.sqrt(np.maximum((W * W).sum(1, keepdims=True), dtype(EPS)))
    q = unit[abc[:, 1]] - unit[abc[:, 0]] + unit[abc[:, 2]]
    s = (q @ unit.T) / np.sqrt(np.maximum((q * q).sum(1, keepdims=True), dtype(EPS)))
    rows = np.arange(len(abc))
    for j in range(3):
        s[rows, abc[:, j]] = -np.inf
    return s


def topk(W, abc, k, extra=0, dtype=np.float64):
    """(sims [n, k + extra], idx [n, k + extra]): descending score, ties to the lower id (a stable sort of the negated
    scores).  `extra`: further ranks behind the k-th, for the gap of the last rank to the next one."""
    s = scores(W, abc, dtype)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k + extra]
    return np.take_along_axis(s, order, 1), order.astype(np.int32)


def separated(sims_ext, k, gap=1e-5):
    """[n, k] bool: ranks whose reference score is at least `gap` away from both neighbours in the ranking (sims_ext:
    topk(..., extra >= 1) where the vocabulary has that many candidates, so that rank k - 1 has a neighbour behind it)."""
    s = np.asarray(sims_ext, np.float64)
    with np.errstate(invalid="ignore"):
        d = s[:, :-1] - s[:, 1:]                    # d[:, r]: rank r to rank r + 1
    ok = np.ones((s.shape[0], k), bool)
    ok[:, 1:] &= d[:, :k - 1] >= gap
    m = min(k, d.shape[1])
    ok[:, :m] &= d[:, :m] >= gap
    return ok


# ---- the question file and the counts, as trainer.analogy keeps them
def parse(path, lowercase=True):
    sections = []
    for lineno, line in enumerate(open(path, encoding="utf8"), 1):
        line = line.strip()
        if not line:
            continue
        if line.startswith(":"):
            sections.append([line[1:].strip(), []])
            continue
        words = line.split()
        if len(words) != 4:
            raise ValueError("line %d" % lineno)
        if not sections:
            sections.append(["", []])
        sections[-1][1].append([w.lower() for w in words] if lowercase else words)
    return sections


def score_file(path, vocab, W, top_k=1, restrict=None, lowercase=True, embeddings="row", global_step=0):
    """The record of analogy.json from a question file, the vocabulary (tokens in id order) and the table W."""
    W = np.asarray(W, np.float64)
    if restrict is not None:
        W, vocab = W[:restrict], vocab[:restrict]
    ids = {}
    for i, t in enumerate(vocab):
        if t != "<UNK>" and t not in ids:
            ids[t] = i
    out = []
    for name, questions in parse(path, lowercase):
        correct = total = skipped = 0
        for words in questions:
            if any(w not in ids for w in words):
                skipped += 1
                continue
            a, b, c, want = (ids[w] for w in words)
            total += 1
            correct += int(want in topk(W, [[a, b, c]], top_k)[1][0])
        out.append({"name": name, "correct": correct, "total": total, "skipped": skipped,
                    "accuracy": correct / total if total else None})

    def merged(rows):
        c, t, s = (sum(r[key] for r in rows) for key in ("correct", "total", "skipped"))
        return {"correct": c, "total": t, "skipped": s, "accuracy": c / t if t else None}
    total = merged(out)
    return {"global_step": global_step, "embeddings": embeddings, "top_k": top_k, "sections": out,
            "semantic": merged([r for r in out if not r["name"].startswith("gram")]),
            "syntactic": merged([r for r in out if r["name"].startswith("gram")]), "total": total,
            "questions_seen": total["total"], "questions_total": total["total"] + total["skipped"]}
