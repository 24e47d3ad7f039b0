"""The cases of tests/test_gpu_factor_row_shapes.py, proved on the references alone (no GPU): the tables reach every row
shape twice and every count of column blocks up to 16, the sparse matrices have their long rows where the slot
arithmetic can go wrong, the exact cases are exact in float32 in either summation order, one float4 lost from a k-means
cluster sum misses the centroid tolerance tenfold at least, and the assign cases leave no point undecided."""
from collections import Counter

import numpy as np
import pytest

import factor_shape_cases as fc
import row_shape_cases as rc

S = fc.S
TABLE_IDS = ["d%d_stride%d" % t for t in fc.TABLES]
F32, F64 = np.float32, np.float64


def in_levels(a):
    return bool(np.isin(np.abs(a) * 8, (1, 2, 3)).all())


def test_the_cases_reach_every_row_shape_twice_and_sixteen_column_blocks():
    assert fc.WIDTHS == (4, 64, 68, 128, 132, 256, 260, 384, 388, 512, 516, 768, 772, 1024)
    for shape, (first, last) in rc.ROW_SHAPES.items():
        assert fc.pick_row_shape(first // 4) == fc.pick_row_shape(last // 4) == shape
        assert first == 4 or fc.pick_row_shape(first // 4 - 1) != shape
        assert fc.pick_row_shape(last // 4 + 1) != shape
    assert fc.TABLES == tuple((d, d) for d in fc.WIDTHS) + ((257, 260),)
    hits = Counter(fc.pick_row_shape(l // 4) for _, l in fc.TABLES)
    assert set(hits) == set(rc.ROW_SHAPES) and min(hits.values()) >= 2
    assert Counter(fc.pick_row_shape(d // 4) for d in fc.WIDTHS) == {shape: 2 for shape in rc.ROW_SHAPES}
    # the dense widths: one block, a block with a 60- and a 4-column edge, two, three, nine and sixteen blocks
    assert [fc.gram_blocks(d) for d in fc.DENSE_WIDTHS] == [1, 1, 1, 2, 2, 3, 9, 16, 16]
    assert [d % 64 for d in fc.DENSE_WIDTHS] == [4, 60, 0, 4, 0, 4, 4, 60, 0]
    assert 16 * 17 // 2 == 136 and max(fc.DENSE_WIDTHS) == 1024
    for d in fc.DENSE_WIDTHS:
        assert fc.gram_rows(d)[:5] == (1, 63, 64, 65, fc.GRAM_CHUNK + 1)
        assert (fc.GRAM_SLICE + 1 in fc.gram_rows(d)) == (d <= 132)
        assert set(fc.transform_ms(d)) == {4, 60, 64, 68, d}
    assert fc.XF_ROWS == (1, 127, 128, 129, 300)


def test_spmm_rows_put_long_rows_where_the_slots_can_go_wrong():
    lens = fc.spmm_row_lengths()
    begins = np.concatenate([[0], np.cumsum(lens)])[:-1]
    long_ = lens > S
    print("%d rows, %d nonzeros; long rows (length, begin %% S): %s"
          % (len(lens), lens.sum(), [(int(n), int(a % S)) for n, a in zip(lens[long_], begins[long_])]))
    assert set(fc.SHORT_LENGTHS + (S - 1, S) + fc.LONG_LENGTHS) <= set(lens.tolist())
    assert fc.SHORT_LENGTHS == (0, 1, 3, 4, 5, 9) and fc.LONG_LENGTHS == (S + 1, 2 * S, 2 * S + 1, 3 * S + 3)
    assert len(lens) % 16 != 0 and len(lens) % 4 != 0 and 5500 <= lens.sum() <= 6500
    a = begins[long_]
    assert a[0] == 0 and long_[0]                                       # at position 0 of the matrix
    assert ((a > 0) & (a % S == 0)).any()                               # on a tile's first position further in
    assert (a % S == S - 1).any()                                       # on a tile's last position
    assert ((a % S >= 64) & (a % S <= S - 64)).any()                    # mid-tile
    assert long_[-1] and long_[-2]                                      # the last two rows, cut out, are long rows again
    assert (long_[:-1] & (lens[1:] == 0)).any()                         # an empty row directly behind a long one
    assert ((lens > 0) & (lens < 4)).any() and ((lens > 4) & (lens % 4 != 0)).any()


@pytest.mark.parametrize("dm,l", fc.TABLES, ids=TABLE_IDS)
def test_spmm_cases_are_exact_tables(dm, l):
    m = fc.spmm_case(dm, l)
    assert m["B"].shape == (fc.V, l) and in_levels(m["B"][:, :dm]) and not m["B"][:, dm:].any()
    v8 = m["val"] * 8
    assert (v8 % 1 == 0).all() and (v8 != 0).all() and np.abs(m["val"]).max() <= 1
    assert m["col"].min() >= 0 and m["col"].max() < fc.V and m["row_ptr"][-1] == len(m["col"]) == len(m["val"])
    rows = np.repeat(np.arange(m["n_rows"]), m["lens"])
    assert max(Counter(zip(rows.tolist(), m["col"].tolist())).values()) > 1      # a column more than once in a row
    Y = m["Y"]
    assert ((Y * 64) % 1 == 0).all() and np.abs(Y).max() < 578 and not Y[:, dm:].any() and not Y[m["lens"] == 0].any()
    assert (Y.astype(F32).astype(F64) == Y).all() and (Y[m["lens"] > 0, :dm] != 0).mean() > 0.9
    assert ((m["sums"] * 8) % 1 == 0).all() and len(set(m["sums"].tolist())) > 10
    # the bound of the argument: the largest sum of magnitudes a row can reach
    assert m["lens"].max() * (3 / 8) < 578 < 2 ** 24 / 64


def test_widest_spmm_case_is_exact_in_float32_in_either_order():
    m = fc.spmm_case(1024, 1024)
    for i in range(m["n_rows"]):
        terms = fc.spmm_terms(m, i)
        assert terms.dtype == F32
        a, b = m["row_ptr"][i], m["row_ptr"][i + 1]
        assert (terms.astype(F64) == m["val"][a:b, None].astype(F64) * m["B"][m["col"][a:b]]).all()     # the products
        up, down = np.zeros(1024, F32), np.zeros(1024, F32)
        for t in range(len(terms)):
            up += terms[t]
            down += terms[len(terms) - 1 - t]
        assert up.dtype == F32 and (up.astype(F64) == m["Y"][i]).all() and (down.astype(F64) == m["Y"][i]).all(), i
        # ... and chunk by chunk, the chunk sums added in order
        chunks = np.zeros(1024, F32)
        for c in range(0, len(terms), S):
            chunks += terms[c:c + S].sum(axis=0, dtype=F32)
        assert (chunks.astype(F64) == m["Y"][i]).all(), i


def test_widest_gram_case_is_exact_in_float32_in_either_order():
    """d = 1024, n = CHUNK + 1, the chain not even cut at the chunk: 64 columns of G (the first and the last 32)."""
    d, n = 1024, fc.GRAM_CHUNK + 1
    X, mean = fc.dense_table(d)
    assert in_levels(X) and in_levels(mean) and X.shape == (n, d)
    cols = np.r_[0:32, d - 32:d]
    for which, m_ in enumerate((mean, None)):
        Xc = X[:n] if m_ is None else X[:n] - m_
        assert Xc.dtype == F32 and (Xc.astype(F64) == (X[:n].astype(F64) - (0 if m_ is None else m_.astype(F64)))).all()
        assert np.abs(Xc).max() <= 6 / 8
        want = fc.gram_reference(n, d)[which]
        assert ((want * 64) % 1 == 0).all() and np.abs(want).max() <= 576 + 36 / 64 and (want == want.T).all()
        for order in (range(n), range(n - 1, -1, -1)):
            acc = np.zeros((d, len(cols)), F32)
            for v in order:
                acc += Xc[v][:, None] * Xc[v][None, cols]
            assert acc.dtype == F32 and (acc.astype(F64) == want[:, cols]).all()
    sums = fc.col_sums_reference(n, d)
    assert ((sums * 8) % 1 == 0).all() and (sums == X[::-1].astype(F64).sum(axis=0)).all()


def test_widest_transform_case_is_exact_in_float32_in_either_order():
    d = m = 1024
    n = 129
    X = fc.dense_table(d)[0][:n]
    T, shift, plain = fc.transform_case(d, m)
    assert in_levels(T) and ((shift * 8) % 1 == 0).all() and np.abs(shift).max() <= 4 and len(set(shift.tolist())) > 20
    assert ((plain * 64) % 1 == 0).all() and np.abs(plain).max() <= 144
    for order in (range(d), range(d - 1, -1, -1)):
        acc = np.zeros((n, m), F32)
        for k in order:
            acc += X[:, k, None] * T[None, :, k]
        assert acc.dtype == F32 and (acc.astype(F64) == plain[:n]).all()
        assert ((acc - shift).astype(F64) == plain[:n] - shift.astype(F64)).all()


@pytest.mark.parametrize("d", fc.DENSE_WIDTHS)
def test_dense_cases_are_exact_tables(d):
    X, mean = fc.dense_table(d)
    assert in_levels(X) and in_levels(mean) and X.shape == (max(fc.gram_rows(d)), d)
    assert np.abs(mean - X.astype(F64).mean(axis=0)).min() > 0.05        # an arbitrary shift, not the mean
    for m in fc.transform_ms(d):
        T, shift, plain = fc.transform_case(d, m)
        assert T.shape == (m, d) and in_levels(T) and shift.shape == (m,) and plain.shape == (300, m)
        assert ((plain * 64) % 1 == 0).all() and ((shift * 8) % 1 == 0).all()
    # every Gram entry of the longest case is a multiple of 1/64 that float64 holds with room to spare
    n = max(fc.gram_rows(d))
    assert n * (6 / 8) ** 2 < 2 ** 53 / 64 and fc.GRAM_CHUNK * (6 / 8) ** 2 <= 576 < 2 ** 24 / 64


@pytest.mark.parametrize("dm,stride", fc.TABLES, ids=TABLE_IDS)
def test_kmeans_case_and_what_one_lost_float4_does_to_a_centroid(dm, stride):
    W, ids, a, C_in = fc.kmeans_case(dm, stride)
    assert W.shape == (fc.V, stride) and in_levels(W[:, :dm]) and not W[:, dm:].any() and not C_in[:, dm:].any()
    assert np.bincount(a, minlength=len(fc.KM_SIZES)).tolist() == list(fc.KM_SIZES) == [63, 0, 4097, 1, 64, 130, 65]
    assert fc.KM_SIZES[fc.KM_EMPTY] == 0 and fc.KM_SIZES[fc.KM_SINGLETON] == 1
    n = len(ids)
    assert n == len(a) == 4420 and -(-n // 2048) == 3 and len(np.unique(ids)) < n          # three sort tiles; ids repeat
    levels, most = 0, n                                                                     # the library's level count
    while levels == 0 or most > 1:
        levels, most = levels + 1, -(-most // 64)
    assert levels == 3 and -(-(-(-4097 // 64)) // 64) == 2                                 # 4,097 -> 65 -> 2 -> 1 rows
    big = np.flatnonzero(a == 2)                                                            # interleaved: members in every tile
    assert all(((big >= t * 2048) & (big < (t + 1) * 2048)).any() for t in range(3)) and (np.diff(big) > 1).any()
    want, counts = fc.kmeans_update_reference(dm, stride)
    assert counts.tolist() == list(fc.KM_SIZES) and (want[fc.KM_EMPTY] == C_in[fc.KM_EMPTY, :dm]).all()
    low = min((fc.removal_factor(dm, stride, c, k4), fc.KM_SIZES[c], k4)
              for c in (0, 6, 5, 2) for k4 in (0, (dm - 1) // 4))
    print("d_model %d stride %d: one float4 lost moves a centroid by %.1f tolerances at least (cluster of %d, float4 %d)"
          % ((dm, stride) + low))
    assert low[0] >= 10


@pytest.mark.parametrize("dm,stride", fc.TABLES, ids=TABLE_IDS)
def test_assign_cases_leave_no_point_undecided(dm, stride):
    import test_gpu_kmeans
    assert fc.UNDECIDED == test_gpu_kmeans.UNDECIDED == 2.5e-5
    assert (fc.RTOL, fc.ATOL) == (test_gpu_kmeans.RTOL, test_gpu_kmeans.ATOL)
    W, ids, C, scores = fc.assign_case(dm, stride)
    assert W.shape == (fc.V, stride) and C.shape == (fc.ASSIGN_K, stride) == (33, stride)
    assert not W[:, dm:].any() and not C[:, dm:].any()
    assert ids[:2].tolist() == [0, fc.V - 1] and sorted(ids.tolist()) == list(range(fc.V))
    assert scores.shape == (fc.V, 33) and not fc.undecided(scores).any()
    assert fc.ASSIGN_SEEDS.get(dm, 0) in (0, 1)
    assert len(set(scores.argmax(axis=1).tolist())) > (2 if dm == 4 else 20)     # the clusters are not one
