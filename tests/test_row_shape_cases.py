"""The cases of tests/test_gpu_eval_row_shapes.py, proved on the references alone (no GPU): the widths are the two ends of
every row shape, the exact tables are exact, and the id comparisons leave out at most 2 % of the positions."""
import numpy as np
import pytest

import row_shape_cases as rc


def test_the_widths_are_the_two_ends_of_every_row_shape():
    assert rc.WIDTHS == (4, 64, 68, 128, 132, 256, 260, 384, 388, 512, 516, 768, 772, 1024)
    for shape, (first, last) in rc.ROW_SHAPES.items():
        assert rc.pick_row_shape(first // 4) == rc.pick_row_shape(last // 4) == shape
        assert first == 4 or rc.pick_row_shape(first // 4 - 1) != shape
        assert rc.pick_row_shape(last // 4 + 1) != shape
    assert rc.pick_row_shape(rc.REFUSED_STRIDE // 4) is None and rc.pick_row_shape(1024 // 4) == (64, 4)
    assert (257, 260) in rc.TABLES and rc.pick_row_shape(256 // 4) != rc.pick_row_shape(260 // 4)
    for groups_per_block in (4, 8, 16):
        assert rc.B_EVAL % groups_per_block


@pytest.mark.parametrize("dm,stride", rc.TABLES)
def test_exact_tables_are_exact_in_float32_in_any_order(dm, stride):
    R, C, br, bc, g = rc.eval_tables(dm, stride)
    for t in (R[:, :dm], C[:, :dm], br, bc, np.float32(g)):
        assert np.isin(np.abs(t) * 8, (1, 2, 3)).all()
    assert not R[:, dm:].any() and not C[:, dm:].any() and R.shape == (rc.V_EVAL, stride)
    row, col, w, y = rc.eval_batch(rc.B_EVAL)
    assert ((w * 8) % 1 == 0).all() and w.min() > 0 and w.max() <= 4 and ((y * 8) % 1 == 0).all()
    p = rc.logits((R, C, br, bc, g), dm, row, col)
    # float32 sums of the products, forwards, backwards and pairwise, all give the float64 logit
    prod = R[row, :dm] * C[col, :dm]
    assert (prod.astype(np.float64) == R[row, :dm].astype(np.float64) * C[col, :dm]).all()
    tail = br[row] + bc[col] + np.float32(g)
    for s in (np.cumsum(prod, 1, dtype=np.float32)[:, -1], np.cumsum(prod[:, ::-1], 1, dtype=np.float32)[:, -1],
              prod.sum(1, dtype=np.float32)):
        assert ((s + tail).astype(np.float64) == p).all()
    assert ((p * 64) % 1 == 0).all()
    # dropping any one float4 of a row moves the logit by a unit of 1/64 at least
    for k4 in (0, (dm - 1) // 4):
        cut = prod.copy()
        cut[:, 4 * k4:4 * k4 + 4] = 0
        moved = np.abs(cut.sum(1, dtype=np.float64) - prod.sum(1, dtype=np.float64))
        assert (moved[moved > 0] >= 1 / 64).all() and (moved > 0).mean() > 0.5
    want = rc.regression_sums((R, C, br, bc, g), dm, row, col, w, y)
    assert ((want * 2 ** 15) % 1 == 0).all() and np.abs(want).max() < 2 ** 37          # exact in float64 in any order
    shuffled = np.random.default_rng(1).permutation(len(row))
    assert (rc.regression_sums((R, C, br, bc, g), dm, row[shuffled], col[shuffled], w[shuffled], y[shuffled]) == want).all()


@pytest.mark.parametrize("dm,stride", rc.TABLES)
def test_logistic_batch_reaches_both_softplus_branches_and_saturates(dm, stride):
    row, col, pos, _ = rc.eval_batch(rc.B_EVAL)
    tables, row, col = rc.saturated(rc.eval_tables(dm, stride), dm, row, col)
    p = rc.logits(tables, dm, row, col)
    assert p[0] > 100 and p[1] < -100 and (p > 0).sum() > 100 and (p < 0).sum() > 100
    assert ((np.abs(p) > 0.01) & (np.abs(p) < 10)).mean() > 0.5                          # the unsaturated sigmoid
    assert ((p * 64) % 1 == 0).all() and np.abs(p).max() < 2 ** 17                       # still exact in float32
    assert np.isfinite(rc.logistic_sums(tables, dm, row, col, pos, pos)).all()


@pytest.mark.parametrize("dm,stride", rc.TABLES)
def test_predict_reference_leaves_out_at_most_two_percent(dm, stride):
    R, queries, pairs = rc.predict_case(dm, stride)
    assert np.isin(np.abs(R[:, :dm]) * 8, (1, 2, 3)).all() and not R[:, dm:].any()
    sims, idx = rc.predict_reference(dm, stride)
    clear = rc.separated("predict", sims)
    assert clear[:5].all()                                   # the 5-query call: 45 positions, one left out is 2.2 %
    assert 1.0 - clear.mean() <= rc.LEFT_OUT_MAX
    assert (idx[:, 0] == queries).all()                      # a row is its own first neighbour
    assert len(R) > 256 // rc.pick_row_shape(stride // 4)[0]  # the inverse norms take more than one block of 256 threads


@pytest.mark.parametrize("path", ["cosadd", "cosmul"])
@pytest.mark.parametrize("dm,stride", rc.TABLES)
def test_analogy_references_leave_out_at_most_two_percent(dm, stride, path):
    W, abc = rc.analogy_case(dm, stride)
    assert W.shape == (rc.V_ANALOGY, stride) and not W[:, dm:].any() and abc.shape == (rc.N_QUERIES, 3)
    sims, idx = rc.analogy_reference(dm, stride, path)
    assert 1.0 - rc.separated(path, sims).mean() <= rc.LEFT_OUT_MAX
    assert not (idx[:, :, None] == abc[:, None, :]).any()
    # the float32 restatement is a restatement: a 3CosAdd cosine within the project's atol; a 3CosMul score within four ulps
    # of a cosine over the smallest denominator, eps (d = 4: some cos(a, v) comes within 1e-3 of -1)
    dev = rc.restatement_deviation(dm, stride, path)
    print("d_model %d stride %d %s: float32 restatement deviates by %.3g" % (dm, stride, path, dev))
    assert 0 < dev < (rc.ATOL if path == "cosadd" else 4 * 2.0 ** -23 / rc.COSMUL_EPS)
