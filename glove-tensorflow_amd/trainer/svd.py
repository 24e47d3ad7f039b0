"""`python -m trainer.svd --train-csv CSV --vocab-txt VOCAB --job-dir J [--embedding-size d] [--transform ppmi|log1p|sqrt|none]
[--cds 0.75] [--shift 1] [--eig 0.5] [--oversample 10] [--power-iterations 2] [--seed 0] [--optimizer NAME]`

The count-based baselines a GloVe score is put against: a truncated SVD of the reweighted co-occurrence matrix — shifted,
smoothed PPMI (Levy, Goldberg & Dagan 2015), or the GloVe paper's SVD / SVD-S (square root) / SVD-L (log(1 + x)) of the
same counts.  The reference does not have this.  The factorisation is a randomized range finder (Halko, Martinsson &
Tropp 2011) whose sparse products, marginals and reweighting run on the GPU (include/glove_factor_hip.h).

Writes a job directory like trainer.estimator's: params.json, the vocabulary, a whole-model checkpoint `model.ckpt-0`
(R = U S^eig, C = V S^eig, zero biases, the optimizer's slots at their initial values) and svd.json (settings, singular
values, nonzero counts, seconds per phase).  trainer.analogy, trainer.wordsim, trainer.categorize, trainer.classes and
trainer.export_embeddings open it unchanged, and trainer.estimator on it (same --optimizer, --embedding-size and
--disable-datetime-path) continues from the SVD vectors.  --job-dir is used as given: no date suffix.

`svd_embeddings` is backend-neutral like trainer.cooccur.CoocAccumulator: `backend` has three operations (GloveHip is
the product one; the tests bring a NumPy one), on torch tensors that live on `backend.device` (the CPU without one):
    csr_spmm(row_ptr i64[n + 1], col_idx i32[nnz], val [nnz], n_rows, n_cols, B [n_cols, l]) -> Y [n_rows, l]
    csr_row_sums(row_ptr, val, n_rows) -> f64 [n_rows]
    coo_reweight(row i32, col i32, val, kind, row_sums f64, col_weights f64, total, log_shift) -> val'
Values and dense operands have `backend.dtype` (float32 without one).  Sorting, transposition, compaction and the dense
[V, l] algebra go through torch; nothing here adds values with float atomics.
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

logger = logging.getLogger(__name__)

TRANSFORMS = ("ppmi", "log1p", "sqrt", "none")
ORTH_FLOOR = 1e-14          # eigenvalues of a Gram matrix below this share of the largest are taken for it
RANK_FLOOR = 1e-7           # singular values at or below this share of the largest have no right vector


def _round_up4(n: int) -> int:
    return (int(n) + 3) // 4 * 4


def _csr(row: torch.Tensor, col: torch.Tensor, val: torch.Tensor, n: int, presorted: bool = False):
    """(row_ptr i64 [n + 1], col_idx i32, val) of the COO entries (ids int64), put in (row, col) order unless they are."""
    if not presorted:
        order = torch.argsort(row * n + col)
        col, val = col[order], val[order]
    counts = torch.bincount(row, minlength=n)               # (integer counts: their order of arrival does not show)
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=row.device)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return row_ptr, col.to(torch.int32).contiguous(), val.contiguous()


def _orth(Y: torch.Tensor) -> torch.Tensor:
    """Orthonormal columns spanning Y's (zero columns where Y has no further direction): whitening by the float64 Gram
    matrix's eigendecomposition, the eigenvalues floored at ORTH_FLOOR of the largest, applied twice — the first pass
    leaves an error of the operand's condition times the rounding, the second removes it.  The operand may be rank
    deficient (a matrix of rank < l; the zero padding columns of the row stride)."""
    for _ in range(2):
        Yd = Y.double()
        lam, E = np.linalg.eigh((Yd.T @ Yd).cpu().numpy())
        top = float(lam.max())
        if not top > 0.0:
            return torch.zeros_like(Y)
        W = E / np.sqrt(np.maximum(lam, ORTH_FLOOR * top))
        Y = (Yd @ torch.from_numpy(W).to(Y.device)).to(Y.dtype)
    return Y


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


def svd_embeddings(row, col, value, V: int, d: int, transform: str = "ppmi", cds: float = 0.75, shift: float = 1.0,
                   eig: float = 0.5, oversample: int = 10, power_iterations: int = 2, seed: int = 0, backend=None) -> dict:
    """Rank-d factors of the V x V matrix f(X), X the co-occurrence table (row, col, value) — numpy arrays or device
    tensors (glove_cooc_finalize's output as it is) with every (row, col) pair listed once:
        R = U S^eig [V, d], C = V_ S^eig [V, d], singular_values [d] descending (float64), nnz, nnz_reweighted, seconds.
    `transform`: ppmi — max(0, log(x total / (r_i c_j^cds)) - log(shift)), r and c the row and column sums, total the sum
    of c_j^cds (cds = 1, shift = 1: plain PPMI) —, log1p, sqrt or none; entries that become 0 (and values <= 0) leave the
    matrix.  The range finder draws numpy.random.default_rng(seed).standard_normal((V, l), float32) with
    l = min(d + oversample, V) and runs `power_iterations` rounds of Q <- orth(M orth(M^T Q)).  Each singular pair's
    sign makes the largest-magnitude entry of u_k positive (ties: the lower index).  Columns of V_ whose singular value is
    at most 1e-7 of the largest are zero."""
    if transform not in TRANSFORMS:
        raise ValueError("transform must be one of %s, got %r" % (", ".join(TRANSFORMS), transform))
    V, d = int(V), int(d)
    if V < 1 or d < 1 or d > V:
        raise ValueError("the embedding size must lie in [1, V = %d], got %d" % (V, d))
    if oversample < 0 or power_iterations < 0:
        raise ValueError("oversample and power_iterations must not be negative, got %d and %d" % (oversample, power_iterations))
    if transform == "ppmi" and not (shift > 0 and cds >= 0):
        raise ValueError("ppmi takes shift > 0 and cds >= 0, got %r and %r" % (shift, cds))
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    dev = torch.device(getattr(backend, "device", "cpu"))
    dt = getattr(backend, "dtype", torch.float32)
    phases = _Phases(dev)

    def tensor(x, dtype):
        return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(device=dev, dtype=dtype)
    row, col, val = tensor(row, torch.int64).reshape(-1), tensor(col, torch.int64).reshape(-1), tensor(value, dt).reshape(-1)
    nnz = int(val.numel())
    if row.numel() != nnz or col.numel() != nnz:
        raise ValueError("row, col and value must have one length, got %d, %d and %d" % (row.numel(), col.numel(), nnz))
    if nnz == 0:
        raise ValueError("the co-occurrence table is empty (nnz == 0)")
    lo, hi = int(torch.minimum(row.min(), col.min())), int(torch.maximum(row.max(), col.max()))
    if lo < 0 or hi >= V:
        raise ValueError("ids must lie in [0, V = %d): found %d .. %d" % (V, lo, hi))
    keys, order = torch.sort(row * V + col)
    dup = int((keys[1:] == keys[:-1]).sum())
    if dup:
        raise ValueError("%d (row, col) pairs are listed more than once: the transform of a split count would be wrong" % dup)
    row, col, val = row[order], col[order], val[order]      # (row, col) order from here on: compaction keeps it
    del keys, order

    # 1. CSR and transposed CSR of the counts; 2. the marginals
    log_shift, total, row_sums, col_weights = 0.0, 0.0, None, None
    if transform == "ppmi":
        A, At = _csr(row, col, val, V, presorted=True), _csr(col, row, val, V)
        row_sums = backend.csr_row_sums(A[0], A[2], V)
        col_sums = backend.csr_row_sums(At[0], At[2], V)
        col_weights = col_sums if cds == 1 else torch.where(col_sums > 0, col_sums, torch.zeros_like(col_sums)) ** cds
        total, log_shift = float(col_weights.sum()), math.log(shift)
        del A, At
    phases.done("csr_and_marginals")
    # 3. reweight; 4. drop what became exactly 0 and rebuild both CSRs
    r32, c32 = row.to(torch.int32), col.to(torch.int32)
    val = backend.coo_reweight(r32, c32, val, transform, row_sums, col_weights, total, log_shift)
    keep = val != 0
    row, col, val = row[keep], col[keep], val[keep].contiguous()
    nnz_after = int(val.numel())
    if nnz_after == 0:
        raise ValueError("no entry is positive after the %s transform" % transform)
    del r32, c32, keep
    A = _csr(row, col, val, V, presorted=True)
    At = _csr(col, row, val, V)
    phases.done("reweight_and_compact")

    def M(X):
        return backend.csr_spmm(A[0], A[1], A[2], V, V, X)

    def Mt(X):
        return backend.csr_spmm(At[0], At[1], At[2], V, V, X)

    # 5. the range finder, its dense operands stored at a row stride of a multiple of four floats (zero padding columns)
    l_model = min(d + int(oversample), V)
    l = _round_up4(l_model)
    omega = np.zeros((V, l), np.float32)
    omega[:, :l_model] = np.random.default_rng(seed).standard_normal((V, l_model), dtype=np.float32)
    Q = _orth(M(torch.from_numpy(omega).to(device=dev, dtype=dt)))
    for _ in range(int(power_iterations)):
        Q = _orth(M(_orth(Mt(Q))))
    T = Mt(Q)
    phases.done("range_finder")
    Td = T.double()
    lam, E = np.linalg.eigh((Td.T @ Td).cpu().numpy())
    lam, E = lam[::-1][:d], np.ascontiguousarray(E[:, ::-1][:, :d])
    sigma = np.sqrt(np.maximum(lam, 0.0))
    live = sigma > RANK_FLOOR * sigma[0]
    Ed = torch.from_numpy(E).to(dev)
    U = (Q.double() @ Ed).cpu().numpy()
    Vt = (Td @ Ed).cpu().numpy()
    Vt = np.where(live, Vt / np.where(live, sigma, 1.0), 0.0)
    # 7. signs; 8. the embeddings
    top = np.abs(U).argmax(axis=0)                          # (numpy: the first of equal maxima)
    sign = np.where(U[top, np.arange(d)] < 0, -1.0, 1.0)
    scale = sign * sigma ** eig
    np_dt = np.float64 if dt == torch.float64 else np.float32
    phases.done("small_eigenproblem")
    return {"R": (U * scale).astype(np_dt), "C": (Vt * scale).astype(np_dt), "singular_values": sigma,
            "nnz": nnz, "nnz_reweighted": nnz_after, "l": l_model, "seconds": phases.seconds}


def main(argv=None, backend=None) -> dict:
    from trainer.config_utils import build_parser, init_params
    from trainer.data_utils import file_lines, load_interaction_csv
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager, get_optimizer
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--train-csv", default=config.TRAIN_CSV, help="interaction CSV (co-occurrence nonzeros) to factorise")
    cli.add_argument("--vocab-txt", default=config.VOCAB_TXT, help="vocabulary, one token per line; the line number is the id")
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="where params.json, vocab.txt, model.ckpt-0 and svd.json go (used as given)")
    cli.add_argument("--embedding-size", type=int, default=config.EMBEDDING_SIZE, help="singular pairs kept: columns of both tables")
    cli.add_argument("--value-name", default="value", help="CSV column holding the co-occurrence value (value: distance-weighted; count: raw)")
    cli.add_argument("--transform", choices=TRANSFORMS, default="ppmi", help="entrywise transform of the counts before the SVD")
    cli.add_argument("--cds", type=float, default=0.75, help="ppmi: context-distribution smoothing exponent (1: none)")
    cli.add_argument("--shift", type=float, default=1.0, help="ppmi: k of the shifted PPMI, log(k) is subtracted (1: none)")
    cli.add_argument("--eig", type=float, default=0.5, help="exponent of the singular values in both tables (0.5: symmetric; 1: U S; 0: U)")
    cli.add_argument("--oversample", type=int, default=10, help="extra columns of the range finder")
    cli.add_argument("--power-iterations", type=int, default=2, help="power iterations of the range finder")
    cli.add_argument("--seed", type=int, default=0, help="seed of the range finder's random matrix")
    cli.add_argument("--optimizer", default=config.OPTIMIZER, help="optimizer whose initial slots the checkpoint holds (what trainer.estimator continues with)")
    args = cli.parse_args(argv)
    optimizer = get_optimizer(args.optimizer)["class_name"]
    # params.json the way trainer.estimator builds it: its parser's defaults under the flags the two commands share
    params = vars(build_parser().parse_args([
        "--train-csv", args.train_csv, "--vocab-txt", args.vocab_txt, "--job-dir", args.job_dir, "--disable-datetime-path",
        "--embedding-size", str(args.embedding_size), "--optimizer", args.optimizer, "--seed", str(args.seed)])).copy()
    V = file_lines(args.vocab_txt)
    t0 = time.perf_counter()
    coo = load_interaction_csv(args.train_csv, args.vocab_txt, params["row_name"], params["col_name"],
                               params["weight_name"], args.value_name)
    seconds = {"load_csv": time.perf_counter() - t0}
    out = svd_embeddings(coo["row"], coo["col"], coo["y"], V, args.embedding_size, transform=args.transform, cds=args.cds,
                         shift=args.shift, eig=args.eig, oversample=args.oversample, power_iterations=args.power_iterations,
                         seed=args.seed, backend=backend)
    seconds.update(out["seconds"])
    params = init_params(params)
    tables = DeviceTables(V, args.embedding_size, optimizer, device="cpu", seed=args.seed)       # slots and scalars at step 0
    tables.embeddings("R").copy_(torch.from_numpy(out["R"].astype(np.float32)))
    tables.embeddings("C").copy_(torch.from_numpy(out["C"].astype(np.float32)))
    tables.br.zero_()
    tables.bc.zero_()
    settings = {k: getattr(args, k) for k in ("transform", "cds", "shift", "eig", "oversample", "power_iterations", "seed",
                                               "value_name", "embedding_size")}
    CheckpointManager(params["job_dir"]).save(tables, extra={"svd": settings})
    record = dict(settings, optimizer=optimizer, vocab_size=V, singular_values=[float(s) for s in out["singular_values"]],
                  nnz=out["nnz"], nnz_reweighted=out["nnz_reweighted"], range_finder_columns=out["l"], seconds=seconds)
    Path(params["job_dir"], "svd.json").write_text(json.dumps(record, indent=2))
    logger.info("SVD of %d of %d nonzeros (%s), sigma %.4g .. %.4g -> %s", out["nnz_reweighted"], out["nnz"], args.transform,
                out["singular_values"][0], out["singular_values"][-1], params["job_dir"])
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    try:
        main()
    except KeyboardInterrupt:
        pass
