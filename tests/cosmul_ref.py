"""TEST-ONLY restatement of 3CosMul word analogies and of the pair cosine (include/glove_eval_sim_hip.h) in float64 NumPy
and plain Python: what tests/test_cosmul.py and tests/test_gpu_cosmul.py compare the product with.  Never imported by it."""
import numpy as np

import analogy_ref

EPS_NORM = 1e-12                # tf.math.l2_normalize's clamp, as in the PREDICT path


def unit_rows(W, dtype=np.float64):
    W = np.asarray(W, dtype)
    return W * (dtype(1) / np.sqrt(np.maximum((W * W).sum(1, keepdims=True), dtype(EPS_NORM))))


def scores(W, abc, eps, dtype=np.float64):
    """[n, V] 3CosMul scores s(b, v) s(c, v) / (s(a, v) + eps), s = (1 + cos) / 2 with cos clamped to [-1, 1], and the
    three ids of every question at -inf."""
    unit = unit_rows(W, dtype)
    abc = np.asarray(abc, np.int64).reshape(-1, 3)
    sa, sb, sc = ((dtype(1) + np.clip(unit[abc[:, j]] @ unit.T, -1, 1)) * dtype(0.5) for j in range(3))
    s = sb * sc / (sa + dtype(eps))
    rows = np.arange(len(abc))
    for j in range(3):
        s[rows, abc[:, j]] = -np.inf
    return s


def topk(W, abc, k, eps, extra=0, dtype=np.float64):
    """(scores [n, k + extra], idx [n, k + extra]): descending score, ties to the lower id (a stable sort of the
    negated scores).  `extra`: further ranks behind the k-th, for the gap of the last rank to the next one."""
    s = scores(W, abc, eps, dtype)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k + extra]
    return np.take_along_axis(s, order, 1), order.astype(np.int32)


def separated(sims_ext, k, gap=1e-5):
    """[n, k] bool: ranks whose reference score s is at least gap * max(1, |s|) away from both neighbours in the ranking
    (3CosMul scores reach 1 / eps: the gap is relative above 1).  sims_ext: topk(..., extra >= 1) where the vocabulary
    has that many candidates."""
    s = np.asarray(sims_ext, np.float64)
    with np.errstate(invalid="ignore"):
        d = s[:, :-1] - s[:, 1:]                    # d[:, r]: rank r to rank r + 1
    need = gap * np.maximum(1.0, np.abs(s[:, :k]))
    ok = np.ones((s.shape[0], k), bool)
    ok[:, 1:] &= d[:, :k - 1] >= need[:, 1:]
    m = min(k, d.shape[1])
    ok[:, :m] &= d[:, :m] >= need[:, :m]
    return ok


def pair_cosine(W, pairs, dtype=np.float64):
    unit = unit_rows(W, dtype)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.clip((unit[pairs[:, 0]] * unit[pairs[:, 1]]).sum(1), -1, 1)


def score_file(path, vocab, W, eps=1e-3, top_k=1, restrict=None, lowercase=True, embeddings="row", global_step=0):
    """The record of analogy_3cosmul.json from a question file, the vocabulary (tokens in id order) and the table W."""
    W = np.asarray(W, np.float64)
    if restrict is not None:
        W, vocab = W[:restrict], vocab[:restrict]
    ids = {}
    for i, t in enumerate(vocab):
        if t != "<UNK>" and t not in ids:
            ids[t] = i
    out = []
    for name, questions in analogy_ref.parse(path, lowercase):
        correct = total = skipped = 0
        for words in questions:
            if any(w not in ids for w in words):
                skipped += 1
                continue
            a, b, c, want = (ids[w] for w in words)
            total += 1
            correct += int(want in topk(W, [[a, b, c]], top_k, eps)[1][0])
        out.append({"name": name, "correct": correct, "total": total, "skipped": skipped,
                    "accuracy": correct / total if total else None})

    def merged(rows):
        c, t, s = (sum(r[key] for r in rows) for key in ("correct", "total", "skipped"))
        return {"correct": c, "total": t, "skipped": s, "accuracy": c / t if t else None}
    total = merged(out)
    return {"global_step": global_step, "embeddings": embeddings, "top_k": top_k, "method": "3cosmul", "epsilon": eps,
            "sections": out, "semantic": merged([r for r in out if not r["name"].startswith("gram")]),
            "syntactic": merged([r for r in out if r["name"].startswith("gram")]), "total": total,
            "questions_seen": total["total"], "questions_total": total["total"] + total["skipped"]}
