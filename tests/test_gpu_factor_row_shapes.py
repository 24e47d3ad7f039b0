"""Every row shape of the lane-group kernels of libglove_factor_hip.so and of k-means, and every count of 64-column blocks
of the dense contractions, on exact tables (tests/factor_shape_cases.py; tests/test_factor_shape_cases.py proves on the
references alone what is relied on here).

  - spmm_chunk_kernel / spmm_rows_kernel <LPR, NV> (glove_csr_spmm_f32) and the row sums (glove_csr_row_sums_f64): the
    fifteen tables of tests/row_shape_cases.py — the first and the last width of each of the seven shapes, and 257 model
    columns on a stride of 260 — times one matrix of 38 rows whose long rows begin at position 0, on a tile's first and
    last position and mid-tile, so that the slot and partial-sum path runs at every shape.  Y and the sums are compared
    for EQUALITY with float64: every term and every partial sum is a float32 number in any order.
  - kmeans_segsum_kernel <LPR, NV, FIRST> at three summation levels, kmeans_finish_kernel <LPR, NV> and
    gathered_inv_norm_kernel <LPR, NV> on the same tables: clusters of 0, 1, 63, 64, 65, 130 and 4,097 members.  The rows
    are normalised, so the centroids are compared at the project's rtol 1e-5 / atol 1e-6 (one float4 lost from a cluster
    sum misses it 53-fold at least); counts, the empty cluster's row and the padding are exact.
  - colsum_slice_kernel, gram_slice_kernel and rows_transform_kernel at d = 4 .. 1024: one to sixteen column blocks (136
    block pairs, the pair decoding's longest walk), with a 4- and a 60-column edge; a one-row second chunk and, at
    d <= 132, a one-row second slice.  Column sums, G with and without the mean and the transform with and without the
    shift EQUAL float64.

The tests elsewhere (test_gpu_svd.py, test_gpu_kmeans.py, test_gpu_postprocess.py) use derived error bounds at widths that
reach three of the seven shapes and five column blocks."""
import numpy as np
import pytest
import torch

import factor_shape_cases as fc
import kmeans_ref
import test_gpu_kmeans
from helpers import to_dev

pytestmark = pytest.mark.gpu
TABLE_IDS = ["d%d_stride%d" % t for t in fc.TABLES]
F64 = np.float64


def poison(*shape, dtype=torch.float32):
    """NaN into a block the size of the next result, then back to the allocator: what torch.empty hands out next is
    most likely that block, so a result the kernel leaves unwritten shows."""
    torch.full(shape, float("nan"), dtype=dtype, device="cuda:0")
    torch.cuda.synchronize()


# ---- the sparse product and the row sums
@pytest.mark.parametrize("dm,l", fc.TABLES, ids=TABLE_IDS)
def test_csr_spmm_equals_float64_at_every_row_shape(hip, dm, l):
    m = fc.spmm_case(dm, l)
    n_rows, n_cols = m["n_rows"], m["n_cols"]
    print("d_model %d l %d: shape (lpr, nv) = %s, %d rows, %d nonzeros" % (dm, l, fc.pick_row_shape(l // 4), n_rows, len(m["val"])))
    rp, col, val, B = to_dev(m["row_ptr"], m["col"], m["val"], m["B"])
    poison(n_rows, l)
    first = hip.csr_spmm(rp, col, val, n_rows, n_cols, B)
    assert first.shape == (n_rows, l) and first.dtype == torch.float32
    got = first.cpu().numpy()
    wrong = np.argwhere(got.astype(F64) != m["Y"])
    assert np.array_equal(got.astype(F64), m["Y"]), ("(row, column) of the first wrong entries", wrong[:8].tolist(),
                                                    "rows", np.unique(wrong[:, 0]).tolist())
    assert (got[m["lens"] == 0] == 0.0).all() and (m["lens"] == 0).sum() >= 2    # zeros the kernel wrote itself
    assert (got[:, dm:] == 0.0).all()                                            # the padding columns
    poison(n_rows, l)
    assert torch.equal(first, hip.csr_spmm(rp, col, val, n_rows, n_cols, B))     # bitwise repeatable
    # the last two rows (both longer than a chunk) as a matrix of their own: other slots, the same bits
    a = int(m["row_ptr"][-3])
    rp2, col2, val2 = to_dev(m["row_ptr"][-3:] - a, m["col"][a:], m["val"][a:])
    part = hip.csr_spmm(rp2, col2, val2, 2, n_cols, B)
    assert torch.equal(first[-2:], part)


@pytest.mark.parametrize("dm,l", fc.TABLES, ids=TABLE_IDS)
def test_csr_row_sums_equal_the_exact_sums(hip, dm, l):
    m = fc.spmm_case(dm, l)
    rp, val = to_dev(m["row_ptr"], m["val"])
    got = hip.csr_row_sums(rp, val, m["n_rows"])
    assert got.shape == (m["n_rows"],) and got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), m["sums"]), np.flatnonzero(got.cpu().numpy() != m["sums"])
    assert torch.equal(got, hip.csr_row_sums(rp, val, m["n_rows"]))
    a = int(m["row_ptr"][-3])
    part = hip.csr_row_sums(*to_dev(m["row_ptr"][-3:] - a, m["val"][a:]), 2)
    assert torch.equal(got[-2:], part)


# ---- k-means
@pytest.mark.parametrize("dm,stride", fc.TABLES, ids=TABLE_IDS)
def test_kmeans_update_at_every_row_shape(hip, dm, stride):
    W, ids, a, C_in = fc.kmeans_case(dm, stride)
    want, want_counts = fc.kmeans_update_reference(dm, stride)
    print("d_model %d stride %d: shape (lpr, nv) = %s, cluster sizes %s, three summation levels"
          % (dm, stride, fc.pick_row_shape(stride // 4), want_counts.tolist()))
    Wd, idsd, ad, Cd = to_dev(W, ids, a, C_in)
    poison(*C_in.shape)
    new, counts = hip.kmeans_update(Wd, idsd, ad, Cd)
    assert new.shape == C_in.shape and counts.dtype == torch.int32
    assert counts.cpu().tolist() == want_counts.tolist() == list(fc.KM_SIZES)                # exact
    got = new.cpu().numpy()
    print("d_model %d stride %d: largest centroid deviation %.3g" % (dm, stride, np.abs(got[:, :dm] - want).max()))
    np.testing.assert_allclose(got[:, :dm], want, rtol=fc.RTOL, atol=fc.ATOL)
    e = fc.KM_EMPTY
    assert np.array_equal(got[e].view(np.uint32), C_in[e].view(np.uint32))                   # bit for bit
    assert (got[:, dm:] == 0.0).all()                                                        # the padding columns
    again = hip.kmeans_update(Wd, idsd, ad, Cd)
    assert torch.equal(new, again[0]) and torch.equal(counts, again[1])                      # bitwise repeatable
    member = ids[a == fc.KM_SINGLETON]
    assert len(member) == 1
    np.testing.assert_allclose(got[fc.KM_SINGLETON, :dm], kmeans_ref.unit_points(W[:, :dm], member)[0], rtol=fc.RTOL, atol=fc.ATOL)


@pytest.mark.parametrize("dm,stride", fc.TABLES, ids=TABLE_IDS)
def test_kmeans_assign_at_every_row_shape(hip, dm, stride):
    W, ids, C, scores = fc.assign_case(dm, stride)
    assert not fc.undecided(scores).any()                    # the cap, asserted first: nothing is left to the GPU's choice
    print("d_model %d stride %d: shape (lpr, nv) = %s" % (dm, stride, fc.pick_row_shape(stride // 4)))
    Wd, idsd, Cd = to_dev(W, ids, C)
    a, cos = hip.kmeans_assign(Wd, idsd, Cd)
    assert a.shape == cos.shape == (len(ids),) and a.dtype == torch.int32 and cos.dtype == torch.float32
    test_gpu_kmeans.check_assign(a, cos, scores, "d_model %d stride %d" % (dm, stride))
    assert (a.cpu().numpy() == scores.argmax(axis=1)).all()  # (check_assign's, with nothing undecided: every point)
    again = hip.kmeans_assign(Wd, idsd, Cd)
    assert torch.equal(a, again[0]) and torch.equal(cos, again[1])               # bitwise repeatable
    part = hip.kmeans_assign(Wd, idsd[37:111].contiguous(), Cd)                  # a point's result does not depend on its place
    assert torch.equal(a[37:111], part[0]) and torch.equal(cos[37:111], part[1])


# ---- the dense contractions
@pytest.mark.parametrize("d", fc.DENSE_WIDTHS)
def test_col_sums_equal_float64(hip, d):
    X = to_dev(fc.dense_table(d)[0])[0]
    print("d %d: %d groups of 32 columns, n = %s" % (d, (d + 31) // 32, fc.gram_rows(d)))
    for n in fc.gram_rows(d):
        Xn = X[:n].contiguous()
        got = hip.col_sums(Xn)
        assert got.shape == (d,) and got.dtype == torch.float64
        want = fc.col_sums_reference(n, d)
        assert np.array_equal(got.cpu().numpy(), want), (n, np.flatnonzero(got.cpu().numpy() != want)[:8])
        assert torch.equal(got, hip.col_sums(Xn))


@pytest.mark.parametrize("d", fc.DENSE_WIDTHS)
def test_gram_equals_float64_and_is_symmetric(hip, d):
    Xh, meanh = fc.dense_table(d)
    X, mean = to_dev(Xh, meanh)
    nb = fc.gram_blocks(d)
    print("d %d: nb = %d column blocks, %d block pairs, n = %s" % (d, nb, nb * (nb + 1) // 2, fc.gram_rows(d)))
    for n in fc.gram_rows(d):
        Xn = X[:n].contiguous()
        for want, mu in zip(fc.gram_reference(n, d), (mean, None)):              # with the mean, and with a null mean
            poison(d, d, dtype=torch.float64)
            got = hip.gram(Xn, mu)
            assert got.shape == (d, d) and got.dtype == torch.float64
            G = got.cpu().numpy()
            wrong = np.argwhere(G != want)
            assert np.array_equal(G, want), (n, "mean" if mu is not None else "null mean", "first wrong (i, j)",
                                             wrong[:8].tolist(), "block pairs", np.unique(wrong // 64, axis=0)[:8].tolist())
            assert torch.equal(got, got.T)                                       # bitwise symmetric
            assert torch.equal(got, hip.gram(Xn, mu))                            # bitwise repeatable


@pytest.mark.parametrize("d", fc.DENSE_WIDTHS)
def test_rows_transform_equals_float64(hip, d):
    X = to_dev(fc.dense_table(d)[0][:max(fc.XF_ROWS)])[0]
    print("d %d: %d k-slabs, m = %s, n = %s" % (d, (d + 31) // 32, fc.transform_ms(d), fc.XF_ROWS))
    for m in fc.transform_ms(d):
        Th, shifth, plain = fc.transform_case(d, m)
        T, shift = to_dev(Th, shifth)
        for n in fc.XF_ROWS:
            Xn = X[:n].contiguous()
            for sh in (shift, None):                                             # with the shift, and null
                want = plain[:n] if sh is None else plain[:n] - shifth.astype(F64)
                poison(n, m)
                got = hip.rows_transform(Xn, T, sh)
                assert got.shape == (n, m) and got.dtype == torch.float32
                Y = got.cpu().numpy().astype(F64)
                assert np.array_equal(Y, want), (n, m, "shift" if sh is not None else "null shift", "first wrong (row, j)",
                                                 np.argwhere(Y != want)[:8].tolist())
                assert torch.equal(got, hip.rows_transform(Xn, T, sh))
