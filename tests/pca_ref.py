"""NumPy restatement of the three operations trainer.postprocess drives (include/glove_factor_dense_hip.h), as a backend
of postprocess_table and as plain functions for the kernel tests; and the planted table the tests share.

The float64 mode is the reference.  The float32 mode keeps the table, the mean, the projection and the results of the
products in float32 (NumPy's own float32 matrix products): the rounding level a float32 implementation has whatever its
summation order — what the driver tests measure the device against."""
import numpy as np
import torch


def col_sums(X):
    """float64 column sums."""
    return np.asarray(X, np.float64).sum(axis=0)


def gram(X, mean=None):
    """G = X~^T X~, x~ the difference X - mean IN THE TABLE'S TYPE (float32 for a float32 table: what the kernel forms),
    every product and sum in float64."""
    X = np.asarray(X)
    Xc = X if mean is None else X - np.asarray(mean, X.dtype)
    Xc = Xc.astype(np.float64)
    return Xc.T @ Xc


def rows_transform(X, T, shift=None):
    """Y = X T^T - shift in float64 (not rounded)."""
    Y = np.asarray(X, np.float64) @ np.asarray(T, np.float64).T
    return Y if shift is None else Y - np.asarray(shift, np.float64)


class NumpyBackend:
    """postprocess_table's backend on the CPU: torch tensors in and out, NumPy inside."""

    def __init__(self, float32: bool = False):
        self.dtype = torch.float32 if float32 else torch.float64
        self._np = np.float32 if float32 else np.float64

    def col_sums(self, X):
        return torch.from_numpy(col_sums(X.numpy()))

    def gram(self, X, mean=None):
        if self._np is np.float64:
            return torch.from_numpy(gram(X.numpy(), None if mean is None else mean.numpy()))
        Xc = X.numpy() if mean is None else X.numpy() - mean.numpy()
        return torch.from_numpy((Xc.T @ Xc).astype(np.float64))                # a float32 product

    def rows_transform(self, X, T, shift=None):
        if self._np is np.float64:
            return torch.from_numpy(rows_transform(X.numpy(), T.numpy(), None if shift is None else shift.numpy()))
        Y = X.numpy() @ T.numpy().T
        return torch.from_numpy(np.ascontiguousarray(Y if shift is None else Y - shift.numpy()))


# ---- the table the tests share
PLANTED_SCALES = np.concatenate([[6.0, 4.0], 0.85 ** np.arange(22)])


def planted(seed: int = 0, n: int = 20000, d: int = 24):
    """A float32 table [n, d] = Z diag(scales) Q^T + mean: Z standard normal, Q a random orthogonal basis, the scales 6, 4,
    0.85^0 ... 0.85^21 per direction (the first two are the planted dominant directions) and a mean of 2 N(0, 1) per
    column.  -> (W float32, Q [d, d] whose columns are the directions in the order of the scales, mean float64)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    scales = PLANTED_SCALES[:d]
    mean = 2.0 * rng.standard_normal(d)
    W = (rng.standard_normal((n, d)) * scales) @ Q.T + mean
    return W.astype(np.float32), Q, mean
