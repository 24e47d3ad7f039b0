"""`python -m trainer.postprocess --job-dir J --output-dir P [--embeddings row|col|sum] [--remove-components D]
[--reduce-to M] [--no-center] [--restrict-vocab N] [--optimizer NAME]`

The post-processing the literature applies to a finished embedding table before scoring it: all-but-the-top (Mu &
Viswanath, ICLR 2018: subtract the mean vector, then remove the projections on the top D principal components; the
paper suggests D about d / 100) and PCA reduction to M columns (Raunak et al. 2019).  The reference does not have this.
The contractions over the table's rows (column sums, the d x d covariance, the product with the [m, d] projection) run
on the GPU (include/glove_factor_dense_hip.h); the d x d eigenproblem is numpy.linalg.eigh on the host in float64.

Writes a job directory at step 0 the way `trainer.vectors import` does: params.json with embedding_size = the new
width, the vocabulary (cut to N with --restrict-vocab), `model.ckpt-0` (R = the processed vectors, C = 0, zero biases,
the optimizer's slots at their initial values) and postprocess.json (settings, the source job directory and step, the
top eigenvalues, the variance shares, seconds per phase).  trainer.analogy, trainer.wordsim, trainer.categorize,
trainer.classes and `trainer.vectors export` open P unchanged.  Training from P is not supported, as for an imported
file: C and the biases are zero, not a model's.  --output-dir is used as given: no date suffix.

Chaining is running the tool on P: Raunak et al.'s scheme (all-but-the-top, PCA, all-but-the-top) is
`--remove-components D --reduce-to M` followed by `--remove-components D` on the result.

`postprocess_table` is backend-neutral like trainer.svd.svd_embeddings: `backend` has three operations (GloveHip is the
product one; the tests bring a NumPy one), on torch tensors that live on `backend.device` (the CPU without one):
    col_sums(X [n, d]) -> f64 [d]
    gram(X [n, d], mean [d] or None) -> f64 [d, d], the Gram matrix of the rows of X - mean
    rows_transform(X [n, d], T [m, d], shift [m] or None) -> Y [n, m] = X T^T - shift
Tables have `backend.dtype` (float32 without one) and the row stride of trainer.hip_api.row_width, zero padding columns.
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

logger = logging.getLogger(__name__)

EMBEDDINGS = ("row", "col", "sum")
TOP_EIGENVALUES = 32        # how many postprocess.json records


def _round_up4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


class _Phases:
    """Seconds per phase; a phase ends when the device has finished it."""

    def __init__(self, device):
        self.device, self.seconds, self._t = device, {}, time.perf_counter()

    def done(self, name: str):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.seconds[name] = self.seconds.get(name, 0.0) + now - self._t
        self._t = now


def default_remove(d: int) -> int:
    """The paper's D about d / 100, at least one component."""
    return max(1, int(round(int(d) / 100)))


def check_settings(d: int, remove: int, reduce_to=None):
    """ValueError for what no table of d columns can give."""
    if remove < 0:
        raise ValueError("--remove-components must not be negative, got %d" % remove)
    if reduce_to is not None and reduce_to < 1:
        raise ValueError("--reduce-to must be at least 1, got %d" % reduce_to)
    if remove + (reduce_to or 0) > d:
        raise ValueError("%d removed + %d kept components exceed the table's %d columns" % (remove, reduce_to or 0, d))


def principal_directions(G: np.ndarray):
    """(eigenvalues descending, eigenvectors as columns) of the symmetric float64 matrix G.  Each eigenvector's sign makes
    its largest-magnitude entry positive (ties: the lower index) — trainer.svd's rule."""
    lam, E = np.linalg.eigh(np.asarray(G, np.float64))
    lam, E = lam[::-1].copy(), np.ascontiguousarray(E[:, ::-1])
    top = np.abs(E).argmax(axis=0)                          # (numpy: the first of equal maxima)
    E = E * np.where(E[top, np.arange(E.shape[1])] < 0, -1.0, 1.0)
    return lam, E


def postprocess_table(W, remove: int, reduce_to=None, center: bool = True, backend=None) -> dict:
    """All-but-the-top (and PCA reduction) of the table W [n, d_model] — a numpy array or a tensor:
        Y [n, d_model] = (W - mean)(I - U_D U_D^T), U_D the top `remove` principal directions of the rows of W - mean, or,
        with `reduce_to` = m, Y [n, m] = (W - mean) U_{D .. D+m-1}: the next m directions (those removed are orthogonal
        to them, so removing and reducing is one product).  center=False leaves the mean in (and takes the directions of
        the uncentred second-moment matrix).
    Returns Y, mean [d_model] (the float64 column sums / n, rounded to the table's type), eigenvalues [d_model] descending
    (of the Gram matrix: n times the variances), components [remove + m, d_model] (the directions used, as rows),
    variance_removed, variance_kept (shares of the eigenvalue sum) and seconds per phase."""
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    from trainer.hip_api import row_width
    dev = torch.device(getattr(backend, "device", "cpu"))
    dt = getattr(backend, "dtype", torch.float32)
    np_dt = np.float64 if dt == torch.float64 else np.float32
    W = W if torch.is_tensor(W) else torch.from_numpy(np.ascontiguousarray(W))
    if W.dim() != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError("expected a table [n, d], got %s" % (tuple(W.shape),))
    n, d_model = int(W.shape[0]), int(W.shape[1])
    remove, m = int(remove), None if reduce_to is None else int(reduce_to)
    check_settings(d_model, remove, m)
    phases = _Phases(dev)
    d = row_width(n, d_model)
    X = torch.zeros(n, d, dtype=dt, device=dev)
    X[:, :d_model] = W.to(device=dev, dtype=dt)
    phases.done("upload")
    # 1. the mean; 2. the Gram matrix of the centred rows
    mean = (backend.col_sums(X).cpu().numpy().astype(np.float64) / n).astype(np_dt)
    mean_dev = torch.from_numpy(mean).to(dev) if center else None
    phases.done("col_sums")
    G = backend.gram(X, mean_dev).cpu().numpy().astype(np.float64)[:d_model, :d_model]
    phases.done("gram")
    # 3. the principal directions; 4. the projection, in the table's stride (the padding columns take no part)
    lam, E = principal_directions(G)
    if m is None:
        width = d_model
        T = np.zeros((d, d), np.float64)
        T[:d_model, :d_model] = np.eye(d_model) - E[:, :remove] @ E[:, :remove].T
    else:
        width = m
        T = np.zeros((_round_up4(m), d), np.float64)
        T[:m, :d_model] = E[:, remove:remove + m].T
    # 5. rounded to the table's type; the shift from the rounded operands in float64, rounded once
    T = T.astype(np_dt)
    shift = (T.astype(np.float64) @ mean.astype(np.float64)).astype(np_dt) if center else None
    phases.done("eigh")
    # 6. the product
    Y = backend.rows_transform(X, torch.from_numpy(T).to(dev), None if shift is None else torch.from_numpy(shift).to(dev))
    Y = Y[:, :width].cpu().numpy()
    phases.done("rows_transform")
    total = float(lam.sum())
    kept = lam[remove:remove + m] if m is not None else lam[remove:]
    return {"Y": np.ascontiguousarray(Y), "mean": mean[:d_model].copy(), "eigenvalues": lam,
            "components": np.ascontiguousarray(E[:, :remove + (m or 0)].T),
            "variance_removed": float(lam[:remove].sum()) / total if total > 0 else 0.0,
            "variance_kept": float(kept.sum()) / total if total > 0 else 0.0, "seconds": phases.seconds}


def build_cli() -> argparse.ArgumentParser:
    cli = argparse.ArgumentParser(description="all-but-the-top and PCA post-processing of a job directory's embeddings",
                                  formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory to read (trainer.estimator's, trainer.svd's, an imported one)")
    cli.add_argument("--output-dir", required=True, help="where params.json, vocab.txt, model.ckpt-0 and postprocess.json go (used as given)")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--remove-components", type=int, default=None, help="top principal components to remove (default: max(1, round(d / 100)))")
    cli.add_argument("--reduce-to", type=int, default=None, help="keep the next M components only: the new embedding size")
    cli.add_argument("--no-center", action="store_true", help="leave the mean vector in")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only")
    cli.add_argument("--optimizer", default=config.OPTIMIZER, help="optimizer whose initial slots the checkpoint holds")
    return cli


def write_step0_job_dir(output_dir, vocab, Y: np.ndarray, optimizer_name: str, extra: dict) -> dict:
    """A job directory at step 0 around the finished vectors Y [V, width] (trainer.retrofit writes its own through this
    too): vocab.txt, params.json the way trainer.estimator builds it, and `model.ckpt-0` with R = Y, C = 0, zero biases
    and `optimizer_name`'s slots at their initial values; `extra` goes into the checkpoint beside the tables.
    -> the params that were written."""
    from trainer.config_utils import build_parser, init_params
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager, get_optimizer
    optimizer = get_optimizer(optimizer_name)["class_name"]
    job = Path(output_dir)
    job.mkdir(parents=True, exist_ok=True)
    vocab_txt = job / "vocab.txt"
    vocab_txt.write_bytes("\n".join(vocab).encode("utf8"))
    V, width = Y.shape
    # params.json the way trainer.estimator builds it: its parser's defaults under the flags the two commands share
    params = vars(build_parser().parse_args([
        "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path", "--embedding-size", str(width),
        "--optimizer", optimizer_name])).copy()
    params = init_params(params)
    new = DeviceTables(V, width, optimizer, device="cpu", seed=0)           # slots and scalars at step 0
    new.embeddings("R").copy_(torch.from_numpy(Y.astype(np.float32)))
    new.embeddings("C").zero_()
    new.br.zero_()
    new.bc.zero_()
    CheckpointManager(params["job_dir"]).save(new, extra=extra)
    return params


def main(argv=None, backend=None) -> dict:
    from trainer.data_utils import read_vocab
    from trainer.train_utils import CheckpointManager, get_optimizer
    args = build_cli().parse_args(argv)
    optimizer = get_optimizer(args.optimizer)["class_name"]
    source = json.loads(Path(args.job_dir, "params.json").read_text())
    d_model = int(source["embedding_size"])
    remove = default_remove(d_model) if args.remove_components is None else args.remove_components
    # everything that can be refused is refused before any directory is made
    check_settings(d_model, remove, args.reduce_to)
    if Path(args.output_dir).resolve() == Path(args.job_dir).resolve():
        raise ValueError("--output-dir must differ from --job-dir (%s): the source is not overwritten" % args.job_dir)
    if args.restrict_vocab is not None and args.restrict_vocab < 1:
        raise ValueError("--restrict-vocab must be positive, got %d" % args.restrict_vocab)
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
    out = postprocess_table(W.float(), remove, args.reduce_to, center=not args.no_center, backend=backend)
    seconds.update(out["seconds"])
    t0 = time.perf_counter()
    V, width = out["Y"].shape
    record = {"source_job_dir": str(source["job_dir"]), "source_step": int(tables["global_step"]), "embeddings": args.embeddings,
              "remove_components": remove, "reduce_to": args.reduce_to, "center": not args.no_center,
              "restrict_vocab": args.restrict_vocab, "optimizer": optimizer, "vocab_size": V, "source_embedding_size": d_model,
              "embedding_size": width, "top_eigenvalues": [float(x) for x in out["eigenvalues"][:TOP_EIGENVALUES]],
              "variance_removed": out["variance_removed"], "variance_kept": out["variance_kept"]}
    params = write_step0_job_dir(args.output_dir, vocab, out["Y"], args.optimizer, {"postprocess": record})
    seconds["write_job_dir"] = time.perf_counter() - t0
    Path(params["job_dir"], "postprocess.json").write_text(json.dumps(dict(record, seconds=seconds), indent=2))
    logger.info("%d x %d (%s of %s, step %d): %d components removed (%.3g of the variance), %d columns kept -> %s", V, d_model,
                args.embeddings, source["job_dir"], record["source_step"], remove, out["variance_removed"], width, params["job_dir"])
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    try:
        main()
    except KeyboardInterrupt:
        pass
