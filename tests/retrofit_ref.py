"""TEST-ONLY restatement of the retrofitting update (include/glove_factor_graph_hip.h): the scalar sequential sweep over the
ids 0, 1, 2, ... in place, a NumPy backend of trainer.retrofit.retrofit_table, and the cases the CPU and the GPU tests
share.  Never imported by the product.

The update of row i, every column on its own (vectorised over the columns, which are independent), in the header's order:
    s = 0, then s = beta[p] * Q_in[col[p]] + s over the row's positions in ascending order (written a * b + c: NumPy has
    no fused multiply-add); w = 0, then w = w + beta[p]; t = alpha * w; num = t * Q_hat[i] + s; den = t + w; num / den.
In float64 it is the reference.  In float32 it states the kernel bit for bit wherever the products beta q and t q^ are
exact, so that a * b + c and fmaf(a, b, c) round the same number once:

Exact tables.  Q^ takes its entries from row_shape_cases.LEVELS = {+-1, +-2, +-3} / 8 (two significant bits), beta is null
or a power of two in {1/4, 1/2, 1, 2}, alpha one of {1/2, 1, 2}.  beta q is then a float32 number whatever q is (a change
of exponent), and t = alpha w is a multiple of 1/8 below 2^13 (w <= 1,100 * 2), so t q^ has at most 16 + 2 significant
bits.  tests/test_retrofit.py asserts both on every operand the sweeps meet."""
import functools

import numpy as np
import torch

from row_shape_cases import LEVELS, TABLES, frozen, padded  # noqa: F401 (the tests read TABLES here)


def updated_row(i, row_ptr, col_idx, beta, Q_hat, Q_in, alpha):
    """Row i after the update, in the type of Q_in: steps 1 to 4, or a copy of Q_in[i] when w == 0."""
    f = Q_in.dtype.type
    n = Q_in.shape[0]
    s, w = np.zeros(Q_in.shape[1], f), f(0)
    for p in range(int(row_ptr[i]), int(row_ptr[i + 1])):
        c = int(col_idx[p])
        if c < 0 or c >= n:
            continue
        b = f(1) if beta is None else f(beta[p])
        s = b * Q_in[c] + s
        w = w + b
    if w == 0:
        return Q_in[i].copy()
    t = f(alpha) * w
    num = t * Q_hat[i] + s
    den = t + w
    out = num / den
    assert out.dtype == Q_in.dtype
    return out


def sequential_sweeps(row_ptr, col_idx, beta, Q_hat, alpha, iterations):
    """The scalar restatement: `iterations` times a loop over the ids 0, 1, 2, ... in order, in place, from Q = Q^."""
    Q = Q_hat.copy()
    for _ in range(iterations):
        for i in range(Q.shape[0]):
            if row_ptr[i + 1] > row_ptr[i]:
                Q[i] = updated_row(i, row_ptr, col_idx, beta, Q_hat, Q, alpha)
    return Q


def update_rows(row_ptr, col_idx, beta, rows, Q_hat, Q_in, Q_out, alpha):
    """glove_retrofit_rows_f32 on NumPy arrays: the listed rows (None: all) from a SNAPSHOT of Q_in into Q_out, which may
    be Q_in; a listed id outside [0, n) is skipped."""
    n = Q_in.shape[0]
    snapshot = Q_in.copy()
    for i in (range(n) if rows is None else [int(r) for r in rows]):
        if 0 <= i < n:
            Q_out[i] = updated_row(i, row_ptr, col_idx, beta, Q_hat, snapshot, alpha)
    return Q_out


class NumpyBackend:
    """retrofit_table's backend on the CPU: torch tensors in and out (shared with NumPy, so Q_out is written in place)."""

    def __init__(self, float32: bool = False):
        self.dtype = torch.float32 if float32 else torch.float64

    def retrofit_rows(self, row_ptr, col_idx, beta, rows, Q_hat, Q_in, Q_out, alpha):
        assert Q_hat.dtype == Q_in.dtype == Q_out.dtype == self.dtype and Q_out.data_ptr() != Q_hat.data_ptr()
        update_rows(row_ptr.numpy(), col_idx.numpy(), None if beta is None else beta.numpy(),
                    None if rows is None else rows.numpy(), Q_hat.numpy(), Q_in.numpy(), Q_out.numpy(), alpha)
        return Q_out


def level_sweeps(row_ptr, col_idx, beta, Q_hat, alpha, iterations, levels):
    """The level schedule on NumPy arrays: per sweep one in-place update_rows per level -> Q."""
    Q = Q_hat.copy()
    for _ in range(iterations):
        for rows in levels:
            update_rows(row_ptr, col_idx, beta, rows, Q_hat, Q, Q, alpha)
    return Q


def lists_of(rows_by_level, offsets):
    return [rows_by_level[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


# ---- the graph every kernel test shares: 300 rows
N = 300
ROW_LENGTHS = (0, 1, 3, 4, 5, 9, 23, 200, 1100)            # the four-in-flight loop, its tail and one long chain
# where the rows of those lengths sit (spread, so that the long rows have neighbours on both sides of them)
SPECIAL = {2: 0, 11: 1, 37: 3, 64: 4, 90: 5, 128: 9, 171: 23, 222: 200, 150: 1100}
SELF_ROW, REPEAT_ROW = 90, 128                              # a row that lists itself; a row that lists one column twice
ALPHAS = (0.5, 1.0, 2.0)
BETAS = np.array([0.25, 0.5, 1.0, 2.0], np.float32)
ITERATIONS = 3


@functools.lru_cache(maxsize=None)
def graph():
    """(row_ptr, col_idx, lens): the special rows above; every other row has 0 to 6 positions (a fifth of them none)."""
    rng = np.random.default_rng(11)
    lens = rng.choice([0, 1, 2, 3, 4, 6], N, p=[0.2, 0.2, 0.2, 0.2, 0.1, 0.1]).astype(np.int64)
    for i, k in SPECIAL.items():
        lens[i] = k
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, N, int(row_ptr[-1])).astype(np.int32)
    col[row_ptr[SELF_ROW] + 2] = SELF_ROW
    col[row_ptr[REPEAT_ROW] + 1] = col[row_ptr[REPEAT_ROW]]
    return frozen(row_ptr, col, lens)


@functools.lru_cache(maxsize=None)
def exact_case(k):
    """Table k of row_shape_cases.TABLES: (Q_hat [N, stride] exact, alpha, beta or None).  alpha cycles through ALPHAS and
    beta is null on every second table, so the fifteen tables meet all six combinations."""
    dm, stride = TABLES[k]
    rng = np.random.default_rng(1200 + dm)
    Q_hat = padded(rng.choice(LEVELS, (N, dm)), stride)
    beta = None if k % 2 == 0 else rng.choice(BETAS, len(graph()[1])).astype(np.float32)
    frozen(Q_hat, *([] if beta is None else [beta]))
    return Q_hat, ALPHAS[k % 3], beta


@functools.lru_cache(maxsize=None)
def exact_sequential(k):
    """The scalar sequential restatement on table k in float32, ITERATIONS sweeps (computed once, never written)."""
    row_ptr, col, _ = graph()
    Q_hat, alpha, beta = exact_case(k)
    return frozen(sequential_sweeps(row_ptr, col, beta, Q_hat, alpha, ITERATIONS))[0]


@functools.lru_cache(maxsize=None)
def exact_jacobi_step(k):
    """One out-of-place update of every row of table k from Q_in = Q^ with its rows rolled by one (so that Q_in differs
    from Q^ and is exact too) -> (Q_in, Q_out) in float32."""
    row_ptr, col, _ = graph()
    Q_hat, alpha, beta = exact_case(k)
    Q_in = np.roll(Q_hat, 1, axis=0).copy()
    Q_out = np.full_like(Q_hat, -7.0)
    update_rows(row_ptr, col, beta, None, Q_hat, Q_in, Q_out, alpha)
    return frozen(Q_in, Q_out)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- general data
U32 = 2.0 ** -24


def g(k):
    return (k + 2) * U32 / (1 - (k + 2) * U32)


def error_bound(longest_row, alpha, q_hat_max):
    """|got - ref| of a float32 implementation after any number of sweeps.  One update errs by at most
    eps = g(L + 3) max|Q^| (a chain of L fused multiply-adds, then t, num, den and the quotient); the update is a convex
    combination that hands on the error its inputs had with weight w / (t + w) = 1 / (1 + alpha): the errors sum to at
    most eps (1 + 1 / alpha)."""
    return g(longest_row + 3) * q_hat_max * (1.0 + 1.0 / alpha)


@functools.lru_cache(maxsize=None)
def general_case(dm, stride, seed=0):
    """(row_ptr, col, beta in (0, 2], Q_hat [N, stride] standard normal, alpha = 0.7 as float32 holds it)."""
    rng = np.random.default_rng([77, dm, seed])
    lens = rng.integers(0, 24, N).astype(np.int64)
    lens[5], lens[140] = 200, 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, N, int(row_ptr[-1])).astype(np.int32)
    beta = (2.0 * (1.0 - rng.random(len(col)))).astype(np.float32)
    beta[beta == 0] = 2.0
    Q_hat = padded(rng.standard_normal((N, dm)).astype(np.float32), stride)
    return frozen(row_ptr, col, beta, Q_hat) + (float(np.float32(0.7)),)
