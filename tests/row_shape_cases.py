"""TEST-ONLY generator of the cases of tests/test_gpu_eval_row_shapes.py: tables at the first and the last width of each of
the seven row shapes of the lane-group kernels (pick_row_shape of csrc/glove_common.h), the float64 references on them,
and the float32 restatement of the two analogy scores that sets their tolerance.  tests/test_row_shape_cases.py proves on
the references alone what the GPU tests rely on.  Never imported by the product.

Exact tables.  Every entry of R and C, the biases and g is one of {+-1, +-2, +-3} / 8 (no zero: a dropped element always
changes a dot product), w a multiple of 1/8 in (0, 4], y a multiple of 1/8.  A product is a multiple of 1/64 below 1/4,
a dot product of up to 1,024 of them an integer multiple of 1/64 below 2^8: every product and every partial sum is exact
in float32 whatever the summation order, so p = r . c + br + bc + g is exact, and a kernel that drops, repeats or
misaddresses one float4 moves it by one unit of 1/64 at least.  The terms of the four regression sums are multiples of
2^-15 far below 2^53: the float64 sums are exact too, in any order."""
import functools

import numpy as np

import analogy_ref
import cosmul_ref
import glove_ref as ref

# (lpr, nv): the widths d = 4 (slots) it serves, first and last
ROW_SHAPES = {(16, 1): (4, 64), (32, 1): (68, 128), (64, 1): (132, 256), (32, 3): (260, 384), (64, 2): (388, 512),
              (64, 3): (516, 768), (64, 4): (772, 1024)}
WIDTHS = tuple(d for ends in ROW_SHAPES.values() for d in ends)
# (d_model, row stride): every width unpadded, and one table whose padding crosses a shape boundary (257 -> 260: the
# model's columns end inside (32, 3)'s first float4 beyond (64, 1)); the padding columns are zero
TABLES = tuple((d, d) for d in WIDTHS) + ((257, 260),)
REFUSED_STRIDE = 1028               # one float4 beyond the widest shape: every entry point answers GLOVE_E_BADARG

V_EVAL, B_EVAL = 300, 3001          # 3,001 pairs: no multiple of a block's 4, 8 or 16 lane groups
K, N_QUERIES = 9, 130               # two query tiles of 128 (predict, 3CosAdd), three of 64 (3CosMul)
V_ANALOGY = 300
COSMUL_EPS = 1e-3
RTOL, ATOL, GAP, LEFT_OUT_MAX = 1e-5, 1e-6, 1e-5, 0.02

LEVELS = np.array([-3, -2, -1, 1, 2, 3], np.float32) / 8


def pick_row_shape(d4):
    """csrc/glove_common.h:pick_row_shape restated: the listed shape with the fewest slots that holds d4 float4."""
    best = None
    for lpr, nv in [(16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4)]:
        if lpr * nv >= d4 and (best is None or lpr * nv < best[0] * best[1]):
            best = (lpr, nv)
    return best


def padded(a, stride):
    out = np.zeros((a.shape[0], stride), np.float32)
    out[:, :a.shape[1]] = a
    return out


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- EVAL
@functools.lru_cache(maxsize=None)
def eval_tables(dm, stride, V=V_EVAL):
    """(R, C [V, stride], br, bc [V], g): exact tables, the padding columns zero."""
    rng = np.random.default_rng(100 + dm)
    R, C = (padded(rng.choice(LEVELS, (V, dm)), stride) for _ in range(2))
    br, bc = rng.choice(LEVELS, V), rng.choice(LEVELS, V)
    return frozen(R, C, br, bc) + (float(rng.choice(LEVELS)),)


@functools.lru_cache(maxsize=None)
def eval_batch(B, V=V_EVAL, seed=0):
    """(row, col, w, y): w multiples of 1/8 in (0, 4], y multiples of 1/8 in [-4, 4]."""
    rng = np.random.default_rng(200 + B + seed)
    row, col = rng.integers(0, V, B).astype(np.int32), rng.integers(0, V, B).astype(np.int32)
    w = (rng.integers(1, 33, B) / 8).astype(np.float32)
    y = (rng.integers(-32, 33, B) / 8).astype(np.float32)
    return frozen(row, col, w, y)


def logits(tables, dm, row, col):
    R, C, br, bc, g = tables
    R, C = R[:, :dm].astype(np.float64), C[:, :dm].astype(np.float64)
    return (R[row] * C[col]).sum(1) + br.astype(np.float64)[row] + bc.astype(np.float64)[col] + g


def regression_sums(tables, dm, row, col, w, y):
    """float64[4]: sum w (p - y)^2, sum w, sum w p, sum w y (include/glove_hip.h: glove_eval_f32)."""
    p, w, y = logits(tables, dm, row, col), w.astype(np.float64), y.astype(np.float64)
    return np.array([(w * (p - y) ** 2).sum(), w.sum(), (w * p).sum(), (w * y).sum()])


def logistic_sums(tables, dm, row, col, pos, neg):
    """float64[6]: sum pos xent(p, 1), sum pos, sum neg xent(p, 0), sum neg, sum pos sigmoid(p), sum neg sigmoid(p)."""
    p, pos, neg = logits(tables, dm, row, col), pos.astype(np.float64), neg.astype(np.float64)
    lse = np.log1p(np.exp(-np.abs(p)))
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-p))
    return np.array([(pos * (np.maximum(-p, 0) + lse)).sum(), pos.sum(), (neg * (np.maximum(p, 0) + lse)).sum(), neg.sum(),
                     (pos * sg).sum(), (neg * sg).sum()])


def saturated(tables, dm, row, col):
    """The tables and the batch with one row pair scaled up on each sign: R[1] = 16, C[2] = 2 and C[3] = -2 in every model
    column, so that p(1, 2) >= 4 * 32 - 1 > 100 and p(1, 3) <= -127 (still exact), as the first two pairs of the batch."""
    R, C, br, bc, g = tables
    R, C, row, col = R.copy(), C.copy(), row.copy(), col.copy()
    R[1, :dm], C[2, :dm], C[3, :dm] = 16.0, 2.0, -2.0
    row[:2], col[:2] = 1, (2, 3)
    return (R, C, br, bc, g), row, col


# ---- PREDICT and the pair cosine
# The vocabulary size and the seed per model width, chosen so that the float64 reference alone leaves out no position of
# the 5-query call and at most 2 % of the 130-query call (tests/test_row_shape_cases.py asserts it).  d = 4: there are only
# 6^4 = 1,296 possible rows and a few hundred distinct cosines, so at V = 300 every seed leaves out about 43 % of the
# positions to exact ties of the formula; 20 rows is the largest table for which a seed without a tie among the first ten
# neighbours of every row turned up (3 of 3,000 seeds; none at V = 24).  20 rows are still two blocks of inv_norm_kernel.
PREDICT_TABLES = {4: (20, 834)}
PREDICT_SEEDS = {64: 1, 256: 1}      # (seed 0 elsewhere; at these two it puts a near-tie into the 5-query call)


@functools.lru_cache(maxsize=None)
def predict_case(dm, stride):
    """(R [V, stride], queries [130], pairs [300, 2]): an exact table; the first five queries are the 5-query call."""
    V, seed = PREDICT_TABLES.get(dm, (300, PREDICT_SEEDS.get(dm, 0)))
    rng = np.random.default_rng(seed)
    R = padded(rng.choice(LEVELS, (V, dm)), stride)
    queries = rng.integers(0, V, N_QUERIES).astype(np.int32)
    edges = list(dict.fromkeys(e for e in (0, 127, 128, V - 1) if e < V))
    queries[:len(edges)] = edges
    pairs = rng.integers(0, V, (300, 2)).astype(np.int32)
    pairs[:len(edges)] = [(e, e) for e in edges]
    return frozen(R, queries, pairs)


@functools.lru_cache(maxsize=None)
def predict_reference(dm, stride):
    """(sims [130, K + 1], idx [130, K + 1]) of ref.cosine_topk on the model's columns."""
    R, queries, _ = predict_case(dm, stride)
    return frozen(*ref.cosine_topk(R[:, :dm].astype(np.float64), queries, K + 1))


# ---- 3CosAdd and 3CosMul: Gaussian tables
@functools.lru_cache(maxsize=None)
def analogy_case(dm, stride):
    """(W [300, stride], abc [130, 3]): three distinct ids per question, the first on the tile edges."""
    rng = np.random.default_rng(300 + dm)
    V = V_ANALOGY
    W = padded(rng.standard_normal((V, dm)).astype(np.float32), stride)
    abc = np.stack([rng.choice(V, 3, replace=False) for _ in range(N_QUERIES)]).astype(np.int32)
    for i, e in enumerate((0, 127, 128, V - 1)):
        others = [x for x in rng.choice(V, 3, replace=False) if x != e][:2]
        abc[i] = np.roll([e] + others, i % 3)
    assert all(len(set(q)) == 3 for q in abc.tolist())
    return frozen(W, abc)


@functools.lru_cache(maxsize=None)
def analogy_reference(dm, stride, path):
    """(scores [130, K + 1], idx [130, K + 1]) in float64, path "cosadd" or "cosmul"."""
    W, abc = analogy_case(dm, stride)
    if path == "cosadd":
        return frozen(*analogy_ref.topk(W[:, :dm], abc, K, extra=1))
    return frozen(*cosmul_ref.topk(W[:, :dm], abc, K, COSMUL_EPS, extra=1))


def separated(path, sims_ext):
    return (analogy_ref if path != "cosmul" else cosmul_ref).separated(sims_ext, K, GAP)


def dot_in_k_order(Q, W):
    """[n, V] float32: q . w as a float32 running sum over the columns in order — the order of the MFMA chain."""
    acc = np.zeros((Q.shape[0], W.shape[0]), np.float32)
    for k in range(Q.shape[1]):
        acc += Q[:, k, None] * W[None, :, k]
    return acc


@functools.lru_cache(maxsize=None)
def restated_f32(dm, stride, path):
    """[130, V] float32 scores of the formula spelled in float32 NumPy, the dot products in k order (no fused
    multiply-add, plain sums for the norms): what float32 costs, before any kernel."""
    W, abc = analogy_case(dm, stride)
    W = W[:, :dm]
    f = np.float32
    inv = (f(1) / np.sqrt(np.maximum((W * W).sum(1, dtype=f), f(1e-12)))).astype(f)
    a, b, c = abc[:, 0], abc[:, 1], abc[:, 2]
    if path == "cosadd":
        Q = W[b] * inv[b, None] - W[a] * inv[a, None] + W[c] * inv[c, None]
        q_inv = f(1) / np.sqrt(np.maximum((Q * Q).sum(1, dtype=f), f(1e-12)))
        s = dot_in_k_order(Q, W) * q_inv[:, None] * inv[None, :]
    else:
        sa, sb, sc = (f(0.5) * (f(1) + np.clip(dot_in_k_order(W[i], W) * inv[i, None] * inv[None, :], f(-1), f(1)))
                      for i in (a, b, c))
        s = sb * sc / (sa + f(COSMUL_EPS))
    assert s.dtype == f
    s.setflags(write=False)
    return s


def deviation(got, want):
    """The largest |got - want| in units of max(1, |want|): absolute for cosines, relative for 3CosMul scores above 1."""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))).max())


@functools.lru_cache(maxsize=None)
def restatement_deviation(dm, stride, path):
    want_s, want_i = analogy_reference(dm, stride, path)
    got = np.take_along_axis(restated_f32(dm, stride, path), want_i[:, :K].astype(np.int64), 1)
    return deviation(got, want_s[:, :K])


def allowed(dm, stride, path, want):
    """The score tolerance of a width, elementwise: the larger of the project's (rtol 1e-5, atol 1e-6) and twice the
    float32 restatement's deviation from float64 — twice, because NumPy has no fused multiply-add and the lane-group
    query builder sums in a butterfly."""
    want = np.abs(np.asarray(want, np.float64))
    return np.maximum(ATOL + RTOL * want, 2 * restatement_deviation(dm, stride, path) * np.maximum(1.0, want))
