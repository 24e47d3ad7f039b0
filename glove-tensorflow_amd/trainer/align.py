"""`python -m trainer.align fit --source-dir S --target-dir T --output-dir A (--dictionary FILE | --shared-vocab
[--anchors N]) [--embeddings row|col|sum] [--normalize unit|none] [--refine R] [--refine-vocab N] [--knn K]
[--optimizer NAME]`
`python -m trainer.align eval --source-dir A --target-dir T --dictionary FILE [--method nn|csls] [--knn K]
[--restrict-vocab N] [--top-k 1 5 10]`

Puts two embedding tables side by side: runs of trainer.estimator that differ in optimizer, sharding, shuffling or seed,
trainer.svd baselines, trainer.postprocess / trainer.retrofit outputs, imported vectors of another language.  The
reference does not have this.

fit: an orthogonal map W from the source space to the target space, fitted on anchor pairs (orthogonal Procrustes,
Schoenemann 1966; Smith et al. 2017, Conneau et al. 2018 for word vectors): with M = sum over the anchors of x~ y~^T
(the d x d cross-covariance: on the GPU, include/glove_factor_align_hip.h) and M = U S V^T (numpy.linalg.svd on the host
in float64), W = V U^T minimises sum |W x~ - y~|^2 over the orthogonal matrices; it is the polar factor of M^T, so no
sign rule is needed.  --normalize unit takes x~, y~ as the unit-length rows (the scales are the clamped inverse norms of
the PREDICT path), none as the rows themselves.  W is rounded once to float32 and applied to the UNSCALED source rows
(include/glove_factor_dense_hip.h: rows_transform).  --refine R repeats the fit R times on the dictionary MUSE's
build_dictionary induces: the pairs among the first --refine-vocab rows of both sides that are each other's nearest
neighbour by CSLS (cross-domain similarity local scaling, 2 cos - r_T(x) - r_S(y) with r the mean cosine to the --knn
nearest rows of the other side: include/glove_eval_cross_hip.h), sorted by source id; every refit is on the original
source rows.  Centring the anchors (Artetxe et al.) and unsupervised initialisation are not done.

Writes a job directory at step 0 the way trainer.postprocess does: the source vocabulary, R = the mapped vectors, so
trainer.analogy, trainer.wordsim, trainer.categorize and `trainer.vectors export` open A unchanged; and align.json
(settings, both inputs and their steps, anchors used and skipped, the top singular values, the orthogonality defect
max |W W^T - I| of the float32 W, the mean anchor cosine before and after, the dictionary size per refinement round,
seconds per phase).  --output-dir is used as given: no date suffix.

eval: MUSE's word-translation scoring of A's row table against T's: each distinct source word of the dictionary is
queried once, by nearest neighbours or by CSLS, and is a hit at k if any of its gold targets is among the k best.
--restrict-vocab N takes the first N target rows as candidates and, for CSLS, the first N source rows as the set the
target-side penalty is computed against.  Writes A/eval/bli.json.

`align_tables` and `translation_precision` are backend-neutral like trainer.postprocess.postprocess_table: `backend`
has four operations (GloveHip is the product one; the tests bring a NumPy one), on torch tensors that live on
`backend.device` (the CPU without one):
    cross_gram(X [Vx, d], xid [n], Y [Vy, d], yid [n], x_scale [Vx] or None, y_scale [Vy] or None) -> f64 [d, d]
    rows_transform(X [n, d], T [m, d]) -> [n, m] = X T^T
    cross_topk(Q [Vq, d], qid [n], T [Vt, d], k, q_pen [n] or None, t_pen [Vt] or None) -> (scores [n, k], idx [n, k])
    topk_mean(sims [n, k]) -> [n]
Tables have `backend.dtype` (float32 without one) and the row stride of trainer.hip_api.row_width, zero padding columns;
ids are int32.
"""
from __future__ import annotations

import argparse
import json
import logging
import time
from pathlib import Path

import numpy as np
import torch

from trainer import config
from trainer.postprocess import EMBEDDINGS, _Phases

logger = logging.getLogger(__name__)

NORMALIZE = ("unit", "none")
METHODS = ("nn", "csls")
TOP_SINGULAR_VALUES = 32        # how many align.json records
NORM_EPS = 1e-12                # tf.math.l2_normalize's clamp, as in the PREDICT path


# ---- the anchors
def vocab_ids(vocab) -> dict:
    """token -> id, the first of equal tokens; <UNK> is no word."""
    ids = {}
    for i, t in enumerate(vocab):
        if t != "<UNK>" and t not in ids:
            ids[t] = i
    return ids


def read_dictionary(path, source_vocab, target_vocab, target_limit=None):
    """A bilingual dictionary in MUSE's format, lines `source target` separated by whitespace -> (pairs int32 [m, 2] of
    (source id, target id) in file order, each pair once; counts: lines, pairs, skipped (a word outside its vocabulary,
    or a target beyond the first `target_limit` rows), duplicates)."""
    src, tgt = vocab_ids(source_vocab), vocab_ids(target_vocab)
    pairs, seen = [], set()
    lines = skipped = duplicates = 0
    with open(path, encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            words = line.split()
            if not words:
                continue
            if len(words) != 2:
                raise ValueError("%s, line %d: expected `source target`, got %d tokens" % (path, lineno, len(words)))
            lines += 1
            s, t = src.get(words[0]), tgt.get(words[1])
            if s is None or t is None or (target_limit is not None and t >= target_limit):
                skipped += 1
            elif (s, t) in seen:
                duplicates += 1
            else:
                seen.add((s, t))
                pairs.append((s, t))
    return (np.asarray(pairs, np.int32).reshape(-1, 2),
            {"lines": lines, "pairs": len(pairs), "skipped": skipped, "duplicates": duplicates})


def shared_vocab_pairs(source_vocab, target_vocab, anchors=None):
    """The words both vocabularies hold, in source-vocabulary order (the first `anchors` of them) -> (pairs, counts)."""
    tgt = vocab_ids(target_vocab)
    pairs = [(s, tgt[t]) for t, s in vocab_ids(source_vocab).items() if t in tgt]
    shared = len(pairs)
    if anchors is not None:
        pairs = pairs[:anchors]
    return np.asarray(pairs, np.int32).reshape(-1, 2), {"shared": shared, "pairs": len(pairs), "skipped": 0, "duplicates": 0}


# ---- the fit
def check_settings(normalize: str, refine: int, refine_vocab: int, knn: int, anchors=None):
    """ValueError for what no pair of tables can give."""
    if normalize not in NORMALIZE:
        raise ValueError("--normalize must be one of %s, got %r" % (", ".join(NORMALIZE), normalize))
    if refine < 0:
        raise ValueError("--refine must not be negative, got %d" % refine)
    if refine_vocab < 1:
        raise ValueError("--refine-vocab must be positive, got %d" % refine_vocab)
    if knn < 1 or knn > 1024:
        raise ValueError("--knn must lie in [1, 1024], got %d" % knn)
    if anchors is not None and anchors < 1:
        raise ValueError("--anchors must be positive, got %d" % anchors)


def _backend(backend):
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    return backend, torch.device(getattr(backend, "device", "cpu")), getattr(backend, "dtype", torch.float32)


def _padded(W, d: int, dev, dt) -> torch.Tensor:
    """The table in the kernels' row stride, zero padding columns."""
    W = W if torch.is_tensor(W) else torch.from_numpy(np.ascontiguousarray(W))
    X = torch.zeros(W.shape[0], d, dtype=dt, device=dev)
    X[:, :W.shape[1]] = W.to(device=dev, dtype=dt)
    return X


def clamped_inv_norms(X: torch.Tensor) -> torch.Tensor:
    """1 / sqrt(max(|row|^2, 1e-12)) per row, in the table's type."""
    return 1.0 / torch.sqrt(torch.clamp((X * X).sum(dim=1), min=NORM_EPS))


def _ids(a, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def procrustes(M: np.ndarray):
    """(W = V U^T float64, singular values descending) of M = U S V^T: the orthogonal W that maximises tr(W M)."""
    U, S, Vt = np.linalg.svd(np.asarray(M, np.float64))
    return Vt.T @ U.T, S


def csls_penalty(backend, A, ids, B, knn: int) -> torch.Tensor:
    """The mean cosine of each row A[ids] to its knn nearest rows of B."""
    return backend.topk_mean(backend.cross_topk(A, ids, B, knn)[0])


def mutual_neighbours(backend, A, T, knn: int) -> np.ndarray:
    """MUSE's build_dictionary on the rows of A and T: the pairs (s, t) that are each other's best by CSLS, sorted by s."""
    dev = A.device
    s_ids, t_ids = _ids(np.arange(A.shape[0]), dev), _ids(np.arange(T.shape[0]), dev)
    s_pen, t_pen = csls_penalty(backend, A, s_ids, T, knn), csls_penalty(backend, T, t_ids, A, knn)
    fwd = backend.cross_topk(A, s_ids, T, 1, s_pen, t_pen)[1][:, 0].cpu().numpy().astype(np.int64)
    bwd = backend.cross_topk(T, t_ids, A, 1, t_pen, s_pen)[1][:, 0].cpu().numpy().astype(np.int64)
    s = np.arange(A.shape[0])
    keep = bwd[fwd] == s
    return np.stack([s[keep], fwd[keep]], axis=1).astype(np.int32)


def align_tables(source, target, pairs, normalize: str = "unit", refine: int = 0, refine_vocab: int = 15000, knn: int = 10,
                 backend=None) -> dict:
    """The orthogonal map of the table `source` [Vs, d_model] onto `target` [Vt, d_model] (numpy arrays or tensors) fitted
    on the anchors pairs [n, 2] = (source id, target id), and `refine` rounds of refitting on the CSLS mutual neighbours
    among the first `refine_vocab` rows of both sides.
    Returns Y [Vs, d_model] = the source rows mapped (W applied to the unscaled rows), W [d_model, d_model] rounded to the
    table's type, singular_values (of the last fit's M, descending), orthogonality_defect max |W W^T - I|,
    anchor_cosine_before / anchor_cosine_after (means over the given anchors), dictionary_sizes (per refinement round)
    and seconds per phase."""
    backend, dev, dt = _backend(backend)
    from trainer.hip_api import row_width
    np_dt = np.float64 if dt == torch.float64 else np.float32
    check_settings(normalize, refine, refine_vocab, knn)
    if source.ndim != 2 or target.ndim != 2 or source.shape[0] < 1 or target.shape[0] < 1:
        raise ValueError("expected two tables [V, d], got %s and %s" % (tuple(source.shape), tuple(target.shape)))
    if source.shape[1] != target.shape[1]:
        raise ValueError("the tables differ in embedding size: %d and %d" % (source.shape[1], target.shape[1]))
    pairs = np.asarray(pairs).reshape(-1, 2)
    if len(pairs) < 1:
        raise ValueError("fewer than one anchor pair")
    (Vs, d_model), Vt = source.shape, target.shape[0]
    if pairs.min() < 0 or pairs[:, 0].max() >= Vs or pairs[:, 1].max() >= Vt:
        raise ValueError("an anchor id lies outside its table")
    Ns, Nt = min(refine_vocab, Vs), min(refine_vocab, Vt)
    if refine and knn > min(Ns, Nt):
        raise ValueError("--knn %d exceeds the %d rows the refinement looks at" % (knn, min(Ns, Nt)))
    phases = _Phases(dev)
    d = row_width(max(Vs, Vt), d_model)
    X, Y = _padded(source, d, dev, dt), _padded(target, d, dev, dt)
    x_inv, y_inv = clamped_inv_norms(X), clamped_inv_norms(Y)
    x_scale, y_scale = (x_inv, y_inv) if normalize == "unit" else (None, None)
    phases.done("upload")

    def anchor_cosine(A, ids) -> float:
        a, b = ids[:, 0].long(), ids[:, 1].long()
        a_inv = x_inv[a] if A is X else clamped_inv_norms(A[a])
        return float(((A[a].double() * Y[b].double()).sum(dim=1) * a_inv.double() * y_inv[b].double()).mean())

    def fit(ids: torch.Tensor):
        M = backend.cross_gram(X, ids[:, 0].contiguous(), Y, ids[:, 1].contiguous(), x_scale, y_scale)
        phases.done("cross_gram")
        W64, S = procrustes(M.cpu().numpy().astype(np.float64)[:d_model, :d_model])
        T = np.zeros((d, d), np_dt)
        T[:d_model, :d_model] = W64.astype(np_dt)                   # rounded once, to the table's type
        phases.done("svd")
        A = backend.rows_transform(X, torch.from_numpy(T).to(dev))
        phases.done("rows_transform")
        return T[:d_model, :d_model], S, A

    anchors = _ids(pairs, dev)
    before = anchor_cosine(X, anchors)
    W, S, A = fit(anchors)
    sizes = []
    for _ in range(refine):
        induced = mutual_neighbours(backend, A[:Ns].contiguous(), Y[:Nt].contiguous(), knn)
        phases.done("build_dictionary")
        sizes.append(int(len(induced)))
        if len(induced) < 1:
            raise ValueError("the refinement found no mutual nearest neighbours")
        W, S, A = fit(_ids(induced, dev))
    after = anchor_cosine(A, anchors)
    W64 = W.astype(np.float64)
    out = A[:, :d_model].cpu().numpy()
    phases.done("download")
    return {"Y": np.ascontiguousarray(out), "W": W, "singular_values": S,
            "orthogonality_defect": float(np.abs(W64 @ W64.T - np.eye(d_model)).max()),
            "anchor_cosine_before": before, "anchor_cosine_after": after, "dictionary_sizes": sizes,
            "seconds": phases.seconds}


# ---- word translation
def translation_precision(source, target, pairs, method: str = "csls", knn: int = 10, top_k=(1, 5, 10), backend=None,
                          batch: int = 1024, penalty_rows=None) -> dict:
    """MUSE's word-translation scoring: every distinct source id of pairs [m, 2] = (source id, target id) is queried once
    against all rows of `target` [Vt, d_model], by cosine ("nn") or by CSLS ("csls": the target-side penalty against the
    first `penalty_rows` rows of `source`, all of them by default); a query is a hit at k if any of its gold targets is
    among its k best.
    -> precision {k: share of the queries}, queries, pairs."""
    backend, dev, dt = _backend(backend)
    from trainer.hip_api import row_width
    if method not in METHODS:
        raise ValueError("--method must be one of %s, got %r" % (", ".join(METHODS), method))
    top_k = sorted({int(k) for k in top_k})
    pairs = np.asarray(pairs).reshape(-1, 2)
    if len(pairs) < 1:
        raise ValueError("no dictionary pair has both words in the vocabularies")
    if source.shape[1] != target.shape[1]:
        raise ValueError("the tables differ in embedding size: %d and %d" % (source.shape[1], target.shape[1]))
    (Vs, d_model), Vt = source.shape, target.shape[0]
    if not top_k or top_k[0] < 1 or top_k[-1] > min(Vt, 1024):
        raise ValueError("--top-k must lie in [1, min(candidates, 1024) = %d], got %s" % (min(Vt, 1024), top_k))
    Np = Vs if penalty_rows is None else min(int(penalty_rows), Vs)
    if method == "csls" and (knn < 1 or knn > min(Np, Vt, 1024)):
        raise ValueError("--knn must lie in [1, %d], got %d" % (min(Np, Vt, 1024), knn))
    phases = _Phases(dev)
    d = row_width(max(Vs, Vt), d_model)
    A, T = _padded(source, d, dev, dt), _padded(target, d, dev, dt)
    queries = np.unique(pairs[:, 0])                                # ascending source id
    gold = {int(s): set() for s in queries}
    for s, t in pairs.tolist():
        gold[s].add(t)
    q_ids = _ids(queries, dev)
    phases.done("upload")
    q_pen = t_pen = None
    if method == "csls":
        q_pen = backend.topk_mean(backend.cross_topk(A, q_ids, T, knn, batch=batch)[0])
        t_pen = backend.topk_mean(backend.cross_topk(T, _ids(np.arange(Vt), dev), A[:Np].contiguous(), knn, batch=batch)[0])
        phases.done("penalties")
    idx = backend.cross_topk(A, q_ids, T, top_k[-1], q_pen, t_pen, batch=batch)[1].cpu().numpy()
    phases.done("cross_topk")
    hits = {k: 0 for k in top_k}
    for row, s in zip(idx.tolist(), queries.tolist()):
        for k in top_k:
            hits[k] += int(any(v in gold[s] for v in row[:k]))
    return {"precision": {k: hits[k] / len(queries) for k in top_k}, "queries": int(len(queries)), "pairs": int(len(pairs)),
            "seconds": phases.seconds}


# ---- the command line
def load_job_table(job_dir, embeddings: str):
    """(table float32 [V, d], vocabulary, global step, the job directory as its params.json names it)."""
    from trainer.data_utils import read_vocab
    from trainer.train_utils import CheckpointManager
    params = json.loads(Path(job_dir, "params.json").read_text())
    latest = CheckpointManager(params["job_dir"]).latest()
    if latest is None:
        raise ValueError("%s holds no checkpoint" % params["job_dir"])
    tables = torch.load(latest, map_location="cpu", weights_only=False)["tables"]
    W = {"row": lambda: tables["R"], "col": lambda: tables["C"], "sum": lambda: tables["R"] + tables["C"]}[embeddings]()
    vocab = read_vocab(params["vocab_txt"])
    if len(vocab) != W.shape[0]:
        raise ValueError("%d vocabulary lines for a table of %d rows" % (len(vocab), W.shape[0]))
    return W.float(), vocab, int(tables["global_step"]), str(params["job_dir"])


def build_cli() -> argparse.ArgumentParser:
    cli = argparse.ArgumentParser(description="align two embedding spaces (orthogonal Procrustes) and score word translation across them",
                                  formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = cli.add_subparsers(dest="command", required=True)
    fit = sub.add_parser("fit", formatter_class=argparse.ArgumentDefaultsHelpFormatter, help="two job directories -> the source mapped into the target's space")
    fit.add_argument("--source-dir", required=True, help="job directory whose vectors are mapped")
    fit.add_argument("--target-dir", required=True, help="job directory whose space they are mapped into")
    fit.add_argument("--output-dir", required=True, help="where params.json, vocab.txt, model.ckpt-0 and align.json go (used as given)")
    how = fit.add_mutually_exclusive_group(required=True)
    how.add_argument("--dictionary", help="anchor pairs: lines `source target` (MUSE's format)")
    how.add_argument("--shared-vocab", action="store_true", help="anchor pairs: the words both vocabularies hold, in source order")
    fit.add_argument("--anchors", type=int, default=None, help="with --shared-vocab: keep the first N shared words only")
    fit.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum, of both directories")
    fit.add_argument("--normalize", choices=NORMALIZE, default="unit", help="fit on unit-length anchor rows, or on the rows as they are")
    fit.add_argument("--refine", type=int, default=0, help="rounds of refitting on the CSLS mutual nearest neighbours")
    fit.add_argument("--refine-vocab", type=int, default=15000, help="rows of both sides a refinement round looks at")
    fit.add_argument("--knn", type=int, default=10, help="neighbours a CSLS penalty averages over")
    fit.add_argument("--optimizer", default=config.OPTIMIZER, help="optimizer whose initial slots the checkpoint holds")
    ev = sub.add_parser("eval", formatter_class=argparse.ArgumentDefaultsHelpFormatter, help="word-translation precision of an aligned directory")
    ev.add_argument("--source-dir", required=True, help="job directory `fit` wrote (its row table is queried)")
    ev.add_argument("--target-dir", required=True, help="job directory of the target space")
    ev.add_argument("--dictionary", required=True, help="test pairs: lines `source target`")
    ev.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="which table of the target directory")
    ev.add_argument("--method", choices=METHODS, default="csls", help="nearest neighbours by cosine, or by CSLS")
    ev.add_argument("--knn", type=int, default=10, help="neighbours a CSLS penalty averages over")
    ev.add_argument("--restrict-vocab", type=int, default=None, help="candidates: the first N target rows (CSLS: and the first N source rows behind the target-side penalty)")
    ev.add_argument("--top-k", type=int, nargs="+", default=[1, 5, 10], help="a query is a hit if a gold target is among this many best")
    ev.add_argument("--batch-size", type=int, default=1024, help="queries per GPU call (their scores are a [batch, candidates] matrix)")
    return cli


def fit_main(args, backend=None) -> dict:
    from trainer.postprocess import write_step0_job_dir
    from trainer.train_utils import get_optimizer
    optimizer = get_optimizer(args.optimizer)["class_name"]
    # everything that can be refused is refused before any directory is made
    check_settings(args.normalize, args.refine, args.refine_vocab, args.knn, args.anchors)
    if args.anchors is not None and not args.shared_vocab:
        raise ValueError("--anchors goes with --shared-vocab")
    out_dir = Path(args.output_dir).resolve()
    for name in ("source_dir", "target_dir"):
        if out_dir == Path(getattr(args, name)).resolve():
            raise ValueError("--output-dir must differ from --%s (%s): an input is not overwritten" % (name.replace("_", "-"), out_dir))
    t0 = time.perf_counter()
    S, s_vocab, s_step, s_dir = load_job_table(args.source_dir, args.embeddings)
    T, t_vocab, t_step, t_dir = load_job_table(args.target_dir, args.embeddings)
    if S.shape[1] != T.shape[1]:
        raise ValueError("the directories differ in embedding size: %d and %d" % (S.shape[1], T.shape[1]))
    seconds = {"load": time.perf_counter() - t0}
    t0 = time.perf_counter()
    if args.shared_vocab:
        pairs, counts = shared_vocab_pairs(s_vocab, t_vocab, args.anchors)
    else:
        pairs, counts = read_dictionary(args.dictionary, s_vocab, t_vocab)
    seconds["anchors"] = time.perf_counter() - t0
    if len(pairs) < 1:
        raise ValueError("fewer than one anchor pair: %s" % counts)
    out = align_tables(S, T, pairs, normalize=args.normalize, refine=args.refine, refine_vocab=args.refine_vocab, knn=args.knn,
                       backend=backend)
    seconds.update(out["seconds"])
    t0 = time.perf_counter()
    V, width = out["Y"].shape
    record = {"source_job_dir": s_dir, "source_step": s_step, "target_job_dir": t_dir, "target_step": t_step,
              "embeddings": args.embeddings, "dictionary": None if args.shared_vocab else str(args.dictionary),
              "shared_vocab": bool(args.shared_vocab), "anchors": args.anchors, "normalize": args.normalize, "refine": args.refine,
              "refine_vocab": args.refine_vocab, "knn": args.knn, "optimizer": optimizer, "vocab_size": V, "embedding_size": width,
              "anchors_used": int(len(pairs)), "anchors_skipped": int(counts["skipped"]), "anchor_counts": counts,
              "top_singular_values": [float(x) for x in out["singular_values"][:TOP_SINGULAR_VALUES]],
              "orthogonality_defect": out["orthogonality_defect"], "anchor_cosine_before": out["anchor_cosine_before"],
              "anchor_cosine_after": out["anchor_cosine_after"], "dictionary_sizes": out["dictionary_sizes"]}
    params = write_step0_job_dir(args.output_dir, s_vocab, out["Y"], args.optimizer, {"align": record})
    seconds["write_job_dir"] = time.perf_counter() - t0
    Path(params["job_dir"], "align.json").write_text(json.dumps(dict(record, seconds=seconds), indent=2))
    logger.info("%d x %d (%s of %s, step %d) onto %s: %d anchors (%d skipped), %d refinements, anchor cosine %.4f -> %.4f -> %s",
                V, width, args.embeddings, s_dir, s_step, t_dir, len(pairs), counts["skipped"], args.refine,
                out["anchor_cosine_before"], out["anchor_cosine_after"], params["job_dir"])
    return out


def eval_main(args, backend=None) -> dict:
    if args.restrict_vocab is not None and args.restrict_vocab < 1:
        raise ValueError("--restrict-vocab must be positive, got %d" % args.restrict_vocab)
    t0 = time.perf_counter()
    A, s_vocab, s_step, s_dir = load_job_table(args.source_dir, "row")
    T, t_vocab, t_step, t_dir = load_job_table(args.target_dir, args.embeddings)
    seconds = {"load": time.perf_counter() - t0}
    pairs, counts = read_dictionary(args.dictionary, s_vocab, t_vocab, target_limit=args.restrict_vocab)
    if args.restrict_vocab is not None:
        T = T[:args.restrict_vocab]
    out = translation_precision(A, T, pairs, method=args.method, knn=args.knn, top_k=args.top_k, backend=backend,
                                batch=args.batch_size, penalty_rows=args.restrict_vocab)
    seconds.update(out["seconds"])
    record = {"source_job_dir": s_dir, "source_step": s_step, "target_job_dir": t_dir, "target_step": t_step,
              "embeddings": args.embeddings, "dictionary": str(args.dictionary), "method": args.method, "knn": args.knn,
              "restrict_vocab": args.restrict_vocab, "top_k": sorted(set(args.top_k)),
              "precision": {str(k): v for k, v in out["precision"].items()}, "queries": out["queries"], "pairs": out["pairs"],
              "pairs_skipped": counts["skipped"], "pairs_duplicate": counts["duplicates"], "seconds": seconds}
    eval_dir = Path(s_dir, "eval")
    eval_dir.mkdir(parents=True, exist_ok=True)
    (eval_dir / "bli.json").write_text(json.dumps(record, indent=2))
    logger.info("%s against %s by %s: %d queries, %s", s_dir, t_dir, args.method, out["queries"],
                ", ".join("P@%d %.4f" % kv for kv in out["precision"].items()))
    return dict(out, record=record)


def main(argv=None, backend=None) -> dict:
    args = build_cli().parse_args(argv)
    return (fit_main if args.command == "fit" else eval_main)(args, backend)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    try:
        main()
    except KeyboardInterrupt:
        pass
