"""`python -m trainer.retrofit --job-dir J --lexicon L --output-dir P [--embeddings row|col|sum] [--iterations 10]
[--alpha 1.0] [--schedule sequential|jacobi] [--restrict-vocab N] [--no-lowercase] [--optimizer NAME]`

Retrofitting a finished embedding table to a semantic lexicon (Faruqui et al., NAACL 2015): every word that the lexicon
gives neighbours is pulled towards them while it stays near its trained vector,
    q_i <- (alpha w_i q^_i + sum_j beta_ij q_j) / (alpha w_i + w_i),    w_i = sum_j beta_ij,
for a number of sweeps; with alpha = 1 and beta = 1 this is the paper's (n_i q^_i + sum_j q_j) / (2 n_i).  The reference
does not have this.  The sweeps run on the GPU (include/glove_factor_graph_hip.h).

Two schedules.  `sequential` is the paper's in-place (Gauss-Seidel) sweep, here in VOCABULARY ORDER — bit for bit what a
scalar loop over the ids 0, 1, 2, ... computes, whatever the hardware does in parallel.  (The original tool sweeps in the
order of a Python set of strings, which changes with the interpreter's hash seed.)  A level schedule makes it parallel:
rows that neither read nor are read by one another form a level, one launch updates a level in place, and the levels run
in order.  `jacobi` updates every row from the previous sweep's table, one launch per sweep between two buffers.

Writes a job directory at step 0 exactly as trainer.postprocess does: params.json, the vocabulary (cut to N with
--restrict-vocab), `model.ckpt-0` (R = the retrofitted vectors, C = 0, zero biases, the optimizer's slots at their
initial values) and retrofit.json (settings, the lexicon's counts, the schedule's figures, how far the vectors moved,
seconds per phase).  trainer.analogy, trainer.wordsim, trainer.categorize, trainer.classes and `trainer.vectors export`
open P unchanged.  Training from P is not supported: C and the biases are zero, not a model's.

`retrofit_table` is backend-neutral like trainer.postprocess.postprocess_table: `backend` has one operation (GloveHip is
the product one; the tests bring a NumPy one), on torch tensors that live on `backend.device` (the CPU without one):
    retrofit_rows(row_ptr i64 [n + 1], col_idx i32 [nnz], beta [nnz] or None, rows i32 [n_list] or None, Q_hat, Q_in,
                  Q_out [n, d], alpha) -> Q_out: the update above of the listed rows (None: all), a listed row without
                  neighbours copied from Q_in; Q_out may be Q_in.
Tables have `backend.dtype` (float32 without one) and the row stride of trainer.hip_api.row_width, zero padding columns.
"""
from __future__ import annotations

import argparse
import json
import logging
import math
import time
from pathlib import Path

import numpy as np
import torch

from trainer import config
from trainer.postprocess import EMBEDDINGS, _Phases

logger = logging.getLogger(__name__)

SCHEDULES = ("sequential", "jacobi")


def read_lexicon(path, vocab, lowercase: bool = True):
    """The lexicon file as a CSR graph over the vocabulary's ids.  A line is `word neighbour neighbour ...`, separated by
    whitespace: the first token is the key, the others are its neighbours (Faruqui's lexicon files: PPDB, WordNet,
    FrameNet).  With `lowercase` the file's tokens are lowercased before they are looked up.
      - a key outside the vocabulary drops its line; a neighbour outside it is dropped; both are counted;
      - several lines for one key are merged, in file order;
      - a neighbour a key already has is dropped (the first occurrence stays) and counted;
      - a key that lists itself keeps that neighbour;
      - the order of a row's neighbours is the file's: it is the summation order.
    Not done: Faruqui's `---num---` / `---punc---` normalisation of tokens, symmetrising the relation (a file that lists
    b under a but not a under b gives one edge), relation weights from the file (every edge has weight 1; `beta` stays
    available to callers of retrofit_table).
    -> (row_ptr int64 [V + 1], col_idx int32 [nnz], counts: lines, keys_in_vocab (distinct), keys_out_of_vocab (lines),
    neighbours_kept, neighbours_out_of_vocab, duplicate_neighbours, rows (keys that kept a neighbour at least))."""
    ids = {}
    for i, w in enumerate(vocab):
        ids.setdefault(w, i)
    V = len(vocab)
    neighbours = {}
    counts = dict(lines=0, keys_in_vocab=0, keys_out_of_vocab=0, neighbours_kept=0, neighbours_out_of_vocab=0,
                  duplicate_neighbours=0, rows=0)
    with open(path, encoding="utf8") as f:
        for line in f:
            tokens = line.split()
            if not tokens:
                continue
            if lowercase:
                tokens = [t.lower() for t in tokens]
            counts["lines"] += 1
            key = ids.get(tokens[0])
            if key is None:
                counts["keys_out_of_vocab"] += 1
                continue
            row = neighbours.setdefault(key, {})
            for t in tokens[1:]:
                j = ids.get(t)
                if j is None:
                    counts["neighbours_out_of_vocab"] += 1
                elif j in row:
                    counts["duplicate_neighbours"] += 1
                else:
                    row[j] = None                           # (a dict keeps insertion order)
    lens = np.zeros(V, np.int64)
    for key, row in neighbours.items():
        lens[key] = len(row)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col_idx = np.zeros(int(row_ptr[-1]), np.int32)
    for key, row in neighbours.items():
        col_idx[row_ptr[key]:row_ptr[key + 1]] = list(row)
    counts["keys_in_vocab"] = len(neighbours)
    counts["neighbours_kept"] = int(row_ptr[-1])
    counts["rows"] = int((lens > 0).sum())
    return row_ptr, col_idx, counts


def level_schedule(row_ptr, col_idx, n: int):
    """The rows with a position at least (U), cut into levels for the in-place sweep in id order: for i < j, both in U,
    with i a column of j or j a column of i, level(j) > level(i); level(i) = 1 + the largest level of such k < i, or 0
    without one — the longest path, so the number of levels (launches per sweep) is the least possible.  Rows outside U
    get no level: nothing updates them, they are constants.  Columns outside [0, n) count for nothing.  Computed on the host.
    -> (rows_by_level int32 [|U|]: level by level, ascending ids inside a level; level_offsets int64 [levels + 1])."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col_idx = np.asarray(col_idx, np.int64)
    n = int(n)
    if row_ptr.shape != (n + 1,) or row_ptr[0] != 0 or row_ptr[-1] != len(col_idx) or (np.diff(row_ptr) < 0).any():
        raise ValueError("row_ptr must hold n + 1 = %d ascending positions from 0 to nnz = %d" % (n + 1, len(col_idx)))
    lens = np.diff(row_ptr)
    in_u = lens > 0
    r = np.repeat(np.arange(n, dtype=np.int64), lens)
    ok = (col_idx >= 0) & (col_idx < n) & (col_idx != r)
    ok[ok] = in_u[col_idx[ok]]
    lo, hi = np.minimum(r[ok], col_idx[ok]), np.maximum(r[ok], col_idx[ok])
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    first = np.searchsorted(hi, np.arange(n + 1))           # the edges whose higher end is j: first[j] .. first[j + 1] - 1
    level = np.full(n, -1, np.int64)
    level[in_u] = 0
    for j in np.flatnonzero(np.diff(first) > 0).tolist():   # (ascending: every lower end has its level by now)
        level[j] = 1 + level[lo[first[j]:first[j + 1]]].max()
    rows = np.flatnonzero(in_u)
    rows = rows[np.argsort(level[rows], kind="stable")]     # (stable: ascending ids inside a level)
    n_levels = int(level.max()) + 1 if len(rows) else 0
    offsets = np.searchsorted(level[rows], np.arange(n_levels + 1)).astype(np.int64)
    return rows.astype(np.int32), offsets


def check_settings(iterations: int, alpha: float, schedule: str = "sequential"):
    """ValueError for what no sweep can take."""
    if iterations < 1:
        raise ValueError("--iterations must be at least 1, got %d" % iterations)
    if not (math.isfinite(alpha) and alpha >= 0):
        raise ValueError("--alpha must be finite and not negative, got %r" % alpha)
    if schedule not in SCHEDULES:
        raise ValueError("--schedule must be one of %s, got %r" % (", ".join(SCHEDULES), schedule))


def retrofit_table(W, row_ptr, col_idx, iterations: int = 10, alpha: float = 1.0, beta=None, schedule: str = "sequential",
                   backend=None) -> dict:
    """`iterations` sweeps of the update over the table W [n, d_model] (a numpy array or a tensor) along the CSR graph
    (row_ptr [n + 1], col_idx [nnz], beta [nnz] or None: all 1), Q^ = W throughout and Q = W at the start.
    `sequential`: per sweep one in-place call per level of level_schedule, in order — the sweep of a scalar loop over the
    ids 0, 1, 2, ..., bit for bit.  `jacobi`: per sweep one call over all rows from one buffer into the other.  The
    graph and the row lists are uploaded once.
    Returns Y [n, d_model], levels (launches per sequential sweep), largest_level (rows), longest_row (positions),
    rows_updated, shift_mean and shift_max (of |q_i - q^_i|_2 over the updated rows, from the table's type in float64)
    and seconds per phase."""
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    from trainer.hip_api import row_width
    iterations, alpha = int(iterations), float(alpha)
    check_settings(iterations, alpha, schedule)
    dev = torch.device(getattr(backend, "device", "cpu"))
    dt = getattr(backend, "dtype", torch.float32)
    W = W if torch.is_tensor(W) else torch.from_numpy(np.array(W))
    if W.dim() != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError("expected a table [n, d], got %s" % (tuple(W.shape),))
    n, d_model = int(W.shape[0]), int(W.shape[1])
    row_ptr = np.array(row_ptr, np.int64)                   # (copies: the caller's arrays may be read-only)
    col_idx = np.array(col_idx, np.int32)
    if beta is not None:
        beta = np.array(beta, np.float64 if dt == torch.float64 else np.float32)
        if beta.shape != col_idx.shape:
            raise ValueError("beta must hold one weight per position: %s for %s" % (beta.shape, col_idx.shape))
    phases = _Phases(dev)
    rows_by_level, offsets = level_schedule(row_ptr, col_idx, n)
    if len(rows_by_level) == 0:
        raise ValueError("the graph gives no row a neighbour: nothing to retrofit")
    level_sizes = np.diff(offsets)
    phases.done("schedule")
    d = row_width(n, d_model)
    Q_hat = torch.zeros(n, d, dtype=dt, device=dev)
    Q_hat[:, :d_model] = W.to(device=dev, dtype=dt)
    rp, ci = torch.from_numpy(row_ptr).to(dev), torch.from_numpy(col_idx).to(dev)
    bt = None if beta is None else torch.from_numpy(beta).to(dev)
    listed = torch.from_numpy(rows_by_level).to(dev)
    Q = Q_hat.clone()
    phases.done("upload")
    if schedule == "sequential":
        lists = [listed[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
        for _ in range(iterations):
            for rows in lists:
                backend.retrofit_rows(rp, ci, bt, rows, Q_hat, Q, Q, alpha)
    else:
        other = torch.empty_like(Q)
        for _ in range(iterations):
            backend.retrofit_rows(rp, ci, bt, None, Q_hat, Q, other, alpha)
            Q, other = other, Q
    phases.done("sweeps")
    moved = (Q[listed.long()].double() - Q_hat[listed.long()].double()).norm(dim=1)
    shift_mean, shift_max = float(moved.mean()), float(moved.max())
    Y = Q[:, :d_model].cpu().numpy()
    phases.done("download")
    return {"Y": np.ascontiguousarray(Y), "levels": int(len(level_sizes)), "largest_level": int(level_sizes.max()),
            "longest_row": int(np.diff(row_ptr).max()), "rows_updated": int(len(rows_by_level)), "shift_mean": shift_mean,
            "shift_max": shift_max, "seconds": phases.seconds}


def build_cli() -> argparse.ArgumentParser:
    cli = argparse.ArgumentParser(description="retrofit a job directory's embeddings to a semantic lexicon (Faruqui et al. 2015)",
                                  formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory to read (trainer.estimator's, trainer.svd's, an imported one)")
    cli.add_argument("--lexicon", required=True, help="lexicon file: `word neighbour neighbour ...` per line")
    cli.add_argument("--output-dir", required=True, help="where params.json, vocab.txt, model.ckpt-0 and retrofit.json go (used as given)")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--iterations", type=int, default=10, help="sweeps over the lexicon's words")
    cli.add_argument("--alpha", type=float, default=1.0, help="weight of a word's trained vector, times its neighbours' weight sum")
    cli.add_argument("--schedule", choices=SCHEDULES, default="sequential",
                     help="in place in vocabulary order (the paper's sweep, reproducible), or every word from the previous sweep")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only")
    cli.add_argument("--no-lowercase", action="store_true", help="take the lexicon's words as written instead of lowercasing them")
    cli.add_argument("--optimizer", default=config.OPTIMIZER, help="optimizer whose initial slots the checkpoint holds")
    return cli


def main(argv=None, backend=None) -> dict:
    from trainer.data_utils import read_vocab
    from trainer.postprocess import write_step0_job_dir
    from trainer.train_utils import CheckpointManager, get_optimizer
    args = build_cli().parse_args(argv)
    optimizer = get_optimizer(args.optimizer)["class_name"]
    # everything that can be refused is refused before any directory is made
    check_settings(args.iterations, args.alpha, args.schedule)
    if Path(args.output_dir).resolve() == Path(args.job_dir).resolve():
        raise ValueError("--output-dir must differ from --job-dir (%s): the source is not overwritten" % args.job_dir)
    if args.restrict_vocab is not None and args.restrict_vocab < 1:
        raise ValueError("--restrict-vocab must be positive, got %d" % args.restrict_vocab)
    source = json.loads(Path(args.job_dir, "params.json").read_text())
    latest = CheckpointManager(source["job_dir"]).latest()
    if latest is None:
        raise ValueError("%s holds no checkpoint" % source["job_dir"])
    t0 = time.perf_counter()
    tables = torch.load(latest, map_location="cpu", weights_only=False)["tables"]
    W = {"row": lambda: tables["R"], "col": lambda: tables["C"], "sum": lambda: tables["R"] + tables["C"]}[args.embeddings]()
    vocab = read_vocab(source["vocab_txt"])
    if len(vocab) != W.shape[0]:
        raise ValueError("%d vocabulary lines for a table of %d rows" % (len(vocab), W.shape[0]))
    if args.restrict_vocab is not None:
        vocab, W = vocab[:args.restrict_vocab], W[:args.restrict_vocab]
    seconds = {"load": time.perf_counter() - t0}
    t0 = time.perf_counter()
    row_ptr, col_idx, counts = read_lexicon(args.lexicon, vocab, lowercase=not args.no_lowercase)
    seconds["read_lexicon"] = time.perf_counter() - t0
    if counts["rows"] == 0:
        raise ValueError("%s leaves no row to update: none of its %d lines has a key and a neighbour in the vocabulary"
                         % (args.lexicon, counts["lines"]))
    out = retrofit_table(W.float(), row_ptr, col_idx, iterations=args.iterations, alpha=args.alpha, schedule=args.schedule,
                         backend=backend)
    seconds.update(out["seconds"])
    t0 = time.perf_counter()
    V, width = out["Y"].shape
    record = {"source_job_dir": str(source["job_dir"]), "source_step": int(tables["global_step"]), "embeddings": args.embeddings,
              "lexicon": str(args.lexicon), "lowercase": not args.no_lowercase, "iterations": args.iterations, "alpha": args.alpha,
              "schedule": args.schedule, "restrict_vocab": args.restrict_vocab, "optimizer": optimizer, "vocab_size": V,
              "embedding_size": width, "lexicon_counts": counts, "levels": out["levels"], "largest_level": out["largest_level"],
              "longest_row": out["longest_row"], "rows_updated": out["rows_updated"], "shift_mean": out["shift_mean"],
              "shift_max": out["shift_max"]}
    params = write_step0_job_dir(args.output_dir, vocab, out["Y"], args.optimizer, {"retrofit": record})
    seconds["write_job_dir"] = time.perf_counter() - t0
    Path(params["job_dir"], "retrofit.json").write_text(json.dumps(dict(record, seconds=seconds), indent=2))
    logger.info("%d x %d (%s of %s, step %d): %d rows retrofitted to %s, %d %s sweeps, %d levels, mean shift %.3g -> %s", V, width,
                args.embeddings, source["job_dir"], record["source_step"], out["rows_updated"], args.lexicon, args.iterations,
                args.schedule, out["levels"], out["shift_mean"], params["job_dir"])
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    try:
        main()
    except KeyboardInterrupt:
        pass
