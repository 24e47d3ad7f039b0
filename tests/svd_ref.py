"""NumPy restatement of the three operations trainer.svd drives (include/glove_factor_hip.h), as a backend of
svd_embeddings and as plain functions for the kernel tests; and the matrices the SVD tests share.

The float64 mode is the reference.  The float32 mode keeps values and dense operands in float32 and lets the sparse
product accumulate in float32 (scipy's CSR product, position by position): the rounding level a float32 implementation
has whatever its summation order — what the driver tests measure the device against."""
from pathlib import Path

import numpy as np
import scipy.sparse as sp
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"


def spmm(row_ptr, col_idx, val, n_rows, n_cols, B, dtype=np.float64):
    """Y = A B with every product and sum in `dtype` (a column listed twice in a row is added twice)."""
    A = sp.csr_matrix((np.asarray(val, dtype), np.asarray(col_idx, np.int64), np.asarray(row_ptr, np.int64)), shape=(n_rows, n_cols))
    return np.ascontiguousarray(A @ np.asarray(B, dtype))


def row_sums(row_ptr, val, n_rows):
    """float64 sums of every row's values."""
    row_ptr, val = np.asarray(row_ptr, np.int64), np.asarray(val, np.float64)
    return np.array([val[row_ptr[i]:row_ptr[i + 1]].sum() for i in range(n_rows)], np.float64)


def reweight(row, col, val, kind, row_sums=None, col_weights=None, total=0.0, log_shift=0.0):
    """The entrywise transform in float64 (not rounded): 0 wherever x <= 0."""
    x = np.asarray(val, np.float64)
    pos = x > 0
    xs = np.where(pos, x, 1.0)
    if kind == "none":
        y = xs
    elif kind == "sqrt":
        y = np.sqrt(xs)
    elif kind == "log1p":
        y = np.log1p(xs)
    elif kind == "ppmi":
        r, c = np.asarray(row_sums, np.float64)[np.asarray(row)], np.asarray(col_weights, np.float64)[np.asarray(col)]
        y = np.maximum(0.0, np.log(xs * total / (r * c)) - log_shift)
    else:
        raise ValueError(kind)
    return np.where(pos, y, 0.0)


class NumpyBackend:
    """svd_embeddings' backend on the CPU: torch tensors in and out, NumPy / SciPy inside."""

    def __init__(self, float32: bool = False):
        self.dtype = torch.float32 if float32 else torch.float64
        self._np = np.float32 if float32 else np.float64

    def csr_spmm(self, row_ptr, col_idx, val, n_rows, n_cols, B):
        return torch.from_numpy(spmm(row_ptr.numpy(), col_idx.numpy(), val.numpy(), n_rows, n_cols, B.numpy(), self._np))

    def csr_row_sums(self, row_ptr, val, n_rows):
        return torch.from_numpy(row_sums(row_ptr.numpy(), val.numpy(), n_rows))

    def coo_reweight(self, row, col, val, kind, row_sums=None, col_weights=None, total=0.0, log_shift=0.0):
        y = reweight(row.numpy(), col.numpy(), val.numpy(), kind, None if row_sums is None else row_sums.numpy(),
                     None if col_weights is None else col_weights.numpy(), total, log_shift)
        return torch.from_numpy(y.astype(self._np))


# ---- the matrices the tests share

PLANTED_SHAPE, PLANTED_BLOCKS = (700, 530), 12


def planted_matrix(seed: int = 0):
    """A 700 x 530 matrix of 12 disjoint blocks, block k filled with s_k (5 down to 0.5): its singular values are
    s_k sqrt(|rows_k| |cols_k|) in closed form and its rank, 12, lies below the range finder's width.
    -> (row, col, val) int32 / int32 / float64 in a shuffled order, the dense matrix, the singular values descending."""
    rng = np.random.default_rng(seed)
    n, m = PLANTED_SHAPE
    rows = np.array_split(rng.permutation(n), 15)[:PLANTED_BLOCKS]
    cols = np.array_split(rng.permutation(m), 14)[:PLANTED_BLOCKS]
    s = np.linspace(5.0, 0.5, PLANTED_BLOCKS)
    M = np.zeros((n, m))
    for k in range(PLANTED_BLOCKS):
        M[np.ix_(rows[k], cols[k])] = s[k]
    sv = np.sort(s * np.sqrt([len(r) * len(c) for r, c in zip(rows, cols)]))[::-1]
    r, c = np.nonzero(M)
    order = rng.permutation(len(r))
    return r[order].astype(np.int32), c[order].astype(np.int32), M[r, c][order], M, sv


def golden_cooccurrence():
    """(row, col, value, V) of tests/golden/text8_cov100_ctx2_cooccurrence.csv: 2,480 entries."""
    t = np.loadtxt(GOLDEN / "text8_cov100_ctx2_cooccurrence.csv", delimiter=",", skiprows=1)
    from trainer.data_utils import file_lines
    V = file_lines(GOLDEN / "text8_cov100_ctx2_vocab.txt")
    return t[:, 0].astype(np.int32), t[:, 1].astype(np.int32), t[:, 3].astype(np.float64), V
