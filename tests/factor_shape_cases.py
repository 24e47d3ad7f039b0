"""TEST-ONLY generator of the cases of tests/test_gpu_factor_row_shapes.py: the sparse product and the row sums of
glove_factor.hip, the k-means update and assignment of glove_kmeans.hip and the column sums, the Gram matrix and the row
transform of glove_pca.hip, at the first and the last width of each of the seven row shapes of pick_row_shape (the tables
of tests/row_shape_cases.py) and at every count of 64-column blocks up to the limit of 16, with their float64 references.
tests/test_factor_shape_cases.py proves on the references alone what the GPU tests rely on.  Never imported by the product.

Exact tables.  B, X, mean, T and W take their entries from LEVELS = {+-1, +-2, +-3} / 8 (no zero: a dropped element always
changes a sum), val and shift are multiples of 1/8.
  - sparse product: a term val B is a multiple of 1/64 of magnitude <= 3/8, the longest row (3 S + 3 = 1,539 nonzeros)
    sums to less than 578: every partial sum in any order, with or without fma, chunked or not, is a float32 number;
  - Gram matrix: |x - mean| <= 6/8 in eighths, a chunk chain of 1,024 products stays <= 576;
  - transform: a chain of 1,024 products stays <= 144, the shift (<= 4) is subtracted from a multiple of 1/64;
  - the float64 sums of all of these are exact in any order.
So Y, the row sums, the column sums, G and the transform equal the float64 results bit for bit, and a kernel that drops,
repeats or misaddresses one float4, one chunk sum or one row moves an entry by one unit of 1/64 at least.

The k-means update normalises its rows (not exact): its table is exact only so that the padding stays zero and the rows
are far from degenerate; the centroids are compared at the project's rtol 1e-5 / atol 1e-6, and removal_factor shows that
one member's float4 lost from a cluster sum misses that tolerance tenfold at least."""
import functools

import numpy as np
import scipy.sparse as sp

import kmeans_ref
from row_shape_cases import LEVELS, TABLES, WIDTHS, frozen, padded, pick_row_shape  # noqa: F401 (the tests read them here)
from trainer.hip_api import FACTOR_CHUNK as S, GRAM_CHUNK, GRAM_SLICE

RTOL, ATOL = 1e-5, 1e-6             # the project's figures for cosines and centroids (tests/test_gpu_kmeans.py)
UNDECIDED = 2.5e-5                  # tests/test_gpu_kmeans.py: UNDECIDED, the margin below which a point is undecided
V = 300                             # rows of B and of W

# ---- the sparse product
SHORT_LENGTHS = (0, 1, 3, 4, 5, 9)                          # the four-in-flight loop and its tail
LONG_LENGTHS = (S + 1, 2 * S, 2 * S + 1, 3 * S + 3)         # two chunks (the second of one nonzero), two, three, four
FILL = 23                                                   # the longest of the short rows that move a long row into place


@functools.lru_cache(maxsize=None)
def spmm_row_lengths():
    """The row lengths of every SpMM case.  Long rows (more than one chunk of S) begin at position 0, at a position
    a % S == 0 further in, at a % S == S - 1 and mid-tile; one is followed by an empty row, one is the last row."""
    lens = []

    def fill_to(residue):
        gap = (residue - sum(lens)) % S
        while gap:
            lens.append(min(gap, FILL))
            gap -= lens[-1]
    lens += [2 * S + 1, 0]                                  # a long row at position 0, an empty row behind it
    lens += [S - 1]                                         # (1,025 + 511 = 3 S)
    lens += [S + 1]                                         # a long row at a % S == 0
    lens += list(SHORT_LENGTHS)
    fill_to(S - 1)
    lens += [2 * S]                                         # a long row at a % S == S - 1: every chunk begins on a tile's last position
    lens += [S]                                             # exactly one chunk, not long
    lens += [7, 200]
    lens += [3 * S + 3]                                     # a long row mid-tile (a % S == 206)
    lens += [S + 1]                                         # the last row is long
    lens = np.array(lens, np.int64)
    lens.setflags(write=False)
    return lens


@functools.lru_cache(maxsize=None)
def spmm_case(dm, l):
    """A CSR matrix [n_rows, V], B [V, l] (the padding columns zero) and the exact float64 product and row sums."""
    rng = np.random.default_rng(400 + dm)
    lens = spmm_row_lengths()
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(row_ptr[-1])
    col = rng.integers(0, V, nnz).astype(np.int32)                              # with repetition, also inside a row
    val = (rng.choice(np.r_[-8:0, 1:9], nnz) / 8).astype(np.float32)            # nonzero multiples of 1/8 in [-1, 1]
    B = padded(rng.choice(LEVELS, (V, dm)), l)
    A = sp.csr_matrix((val.astype(np.float64), col, row_ptr), shape=(len(lens), V))
    Y = np.asarray(A @ B.astype(np.float64))
    sums = np.array([val[a:b].astype(np.float64).sum() for a, b in zip(row_ptr[:-1], row_ptr[1:])])
    m = dict(row_ptr=row_ptr, col=col, val=val, B=B, Y=Y, sums=sums, lens=lens, n_rows=len(lens), n_cols=V, l=l, dm=dm)
    frozen(row_ptr, col, val, B, Y, sums)
    return m


def spmm_terms(m, i):
    """[len, l] float32: the terms val B[col] of row i in position order (each exact: a multiple of 1/64)."""
    a, b = m["row_ptr"][i], m["row_ptr"][i + 1]
    return m["val"][a:b, None] * m["B"][m["col"][a:b]]


# ---- the dense contractions
DENSE_WIDTHS = (4, 60, 64, 68, 128, 132, 516, 1020, 1024)   # 1 block, a 60- and a 4-column edge, 2 - 3, 9, 16 with and without an edge
GRAM_COLS = 64
XF_ROWS = (1, 127, 128, 129, 300)                           # around the transform's tile of 128 table rows, and three tiles


def gram_blocks(d):
    return (d + GRAM_COLS - 1) // GRAM_COLS


def gram_rows(d):
    """One row, around a slab of 64 rows, one chunk and a one-row second chunk; a one-row second slice where d <= 132."""
    return (1, 63, 64, 65, GRAM_CHUNK + 1) + ((GRAM_SLICE + 1,) if d <= 132 else ())


def transform_ms(d):
    return tuple(sorted({4, 60, 64, 68, d}))                # around the tile of 64 rows of T, and the square transform


@functools.lru_cache(maxsize=None)
def dense_table(d):
    """(X [the most rows of gram_rows(d), d], mean [d]): the cases of n rows are X[:n].  `mean` is an arbitrary shift
    drawn from LEVELS, not the mean of X: the entry points compute X - mean whatever it is."""
    rng = np.random.default_rng(500 + d)
    return frozen(rng.choice(LEVELS, (max(gram_rows(d)), d)), rng.choice(LEVELS, d))


def col_sums_reference(n, d):
    return dense_table(d)[0][:n].astype(np.float64).sum(axis=0)


@functools.lru_cache(maxsize=4)
def gram_reference(n, d):
    """(G with the mean, G with a null mean) in float64."""
    X, mean = dense_table(d)
    out = []
    for m_ in (mean, None):
        Xc = (X[:n] if m_ is None else X[:n] - m_).astype(np.float64)
        out.append(Xc.T @ Xc)
    return frozen(*out)


@functools.lru_cache(maxsize=None)
def transform_case(d, m):
    """(T [m, d], shift [m], X[:300] T^T in float64): the cases of n rows are its first n rows."""
    rng = np.random.default_rng(600 + 1031 * d + m)
    T = rng.choice(LEVELS, (m, d))
    shift = (rng.integers(-32, 33, m) / 8).astype(np.float32)
    plain = dense_table(d)[0][:max(XF_ROWS)].astype(np.float64) @ T.astype(np.float64).T
    return frozen(T, shift, plain)


# ---- k-means
KM_SIZES = (63, 0, 4097, 1, 64, 130, 65)                    # members of cluster c: 4,097 = 64 * 64 + 1 reach the third summation level
KM_EMPTY, KM_SINGLETON = 1, 3
ASSIGN_K = 33
# The seed per model width of the assign case, chosen so that the float64 reference alone leaves no point undecided
# (tests/test_factor_shape_cases.py asserts it); seed 0 elsewhere (at these two it leaves one point undecided)
ASSIGN_SEEDS = {4: 1, 388: 1}


@functools.lru_cache(maxsize=None)
def kmeans_case(dm, stride):
    """(W [V, stride], ids [4,420], assign [4,420], C_in [7, stride]): ids with repetition, the members of the clusters
    interleaved; three sort tiles of 2,048 points and three summation levels."""
    rng = np.random.default_rng(700 + dm)
    W = padded(rng.choice(LEVELS, (V, dm)), stride)
    n = sum(KM_SIZES)
    ids = rng.integers(0, V, n).astype(np.int32)
    a = np.repeat(np.arange(len(KM_SIZES)), KM_SIZES)[rng.permutation(n)].astype(np.int32)
    C_in = padded(rng.standard_normal((len(KM_SIZES), dm)).astype(np.float32), stride)
    return frozen(W, ids, a, C_in)


@functools.lru_cache(maxsize=None)
def kmeans_update_reference(dm, stride):
    """(centroids [7, dm] float64, counts [7]) of kmeans_ref.update on the model's columns."""
    W, ids, a, C_in = kmeans_case(dm, stride)
    return frozen(*kmeans_ref.update(W[:, :dm], ids, a, C_in[:, :dm]))


def removal_factor(dm, stride, c, k4):
    """By how many times the tolerance (ATOL + RTOL |centroid|) the centroid of cluster c moves, in its worst entry, when
    float4 k4 of one member's unit row is left out of the float64 cluster sum: the smallest over the members."""
    W, ids, a, _ = kmeans_case(dm, stride)
    rows = np.unique(ids[a == c])
    U = kmeans_ref.unit_points(W[:, :dm], rows)
    total = kmeans_ref.unit_points(W[:, :dm], ids[a == c]).sum(axis=0)
    want = total / np.sqrt(total @ total)
    cut = np.repeat(total[None, :], len(rows), axis=0)
    cut[:, 4 * k4:4 * k4 + 4] -= U[:, 4 * k4:4 * k4 + 4]
    cut /= np.sqrt((cut * cut).sum(axis=1, keepdims=True))
    return float((np.abs(cut - want) / (ATOL + RTOL * np.abs(want))).max(axis=1).min())


@functools.lru_cache(maxsize=None)
def assign_case(dm, stride):
    """(W [V, stride], ids [V]: a permutation with 0 and V - 1 first, C [33, stride], the reference scores [V, 33]):
    Gaussian, like the cases of tests/test_gpu_kmeans.py."""
    rng = np.random.default_rng([900 + dm, ASSIGN_SEEDS.get(dm, 0)])
    W = padded(rng.standard_normal((V, dm)).astype(np.float32), stride)
    rest = rng.permutation(np.arange(1, V - 1))
    ids = np.concatenate([[0, V - 1], rest]).astype(np.int32)
    C = (W[rng.choice(V, ASSIGN_K, replace=False), :dm] + 0.5 * rng.standard_normal((ASSIGN_K, dm))).astype(np.float32)
    C = padded(C, stride)
    scores = kmeans_ref.scores(W[:, :dm], ids, C[:, :dm])
    return frozen(W, ids, C, scores)


def undecided(scores):
    """[n] bool: the points whose best score leads the second best by less than UNDECIDED."""
    top = np.sort(scores, axis=1)[:, -2:]
    return top[:, 1] - top[:, 0] < UNDECIDED
