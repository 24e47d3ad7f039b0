"""Every row shape of the lane-group kernels, at its first and its last width: eval_kernel (glove_eval_f32,
glove_eval_logistic_f32), inv_norm_kernel (glove_topk_cosine_f32 and both analogy paths), analogy_query_kernel
(glove_analogy_topk_f32), pair_cosine_kernel (glove_pair_cosine_f32) and the query gather of glove_cosmul_topk_f32.

pick_row_shape(d / 4) serves d = 4..64 with 16 lanes x 1 float4, 68..128 with 32 x 1, 132..256 with 64 x 1, 260..384
with 32 x 3, 388..512 with 64 x 2, 516..768 with 64 x 3 and 772..1024 with 64 x 4; the tests elsewhere run at
d <= 128 and d = 300, which reach three of the seven.  Here: all fourteen ends, one table of 257 model columns on a
stride of 260 (the padding crosses from 64 x 1 into 32 x 3), and the stride 1028 that every entry point refuses.

The entry points that read table rows directly run on exact tables (tests/row_shape_cases.py): every dot product is an
integer multiple of 1/64 that float32 holds exactly in any summation order, so the regression sums are compared for
EQUALITY with float64 NumPy, the logistic sums at rtol 1e-12 (only exp and log1p differ, in double), cosines at the
project's rtol 1e-5 / atol 1e-6 — at every width, the tolerance does not grow with d.  A lane group that drops, repeats
or misaddresses one float4 moves a dot product by 1/64 at least (d = 1024: 1e-4 of a cosine).

3CosAdd and 3CosMul build their query in float32 (not exact): Gaussian tables, V = 300, n = 130, k = 9, scores within
the larger of (1e-5, 1e-6) and twice the deviation from float64 of the formula restated in float32 NumPy with the dot
product summed in k order (row_shape_cases.restated_f32), in units of max(1, |score|).  Measured, restatement / kernel on
an MI355X:

    d_model  stride   3CosAdd                3CosMul
          4       4   2.34e-07 / 2.31e-07    2.5e-05  / 2.5e-05
         64      64   1.54e-07 / 1.5e-07     4.24e-07 / 4.24e-07
         68      68   1.57e-07 / 1.23e-07    2.41e-07 / 3.42e-07
        128     128   1.53e-07 / 1.32e-07    2.49e-07 / 1.91e-07
        132     132   1.78e-07 / 2.1e-07     2.07e-07 / 2.2e-07
        256     256   2.08e-07 / 1.78e-07    1.81e-07 / 1.68e-07
        260     260   1.57e-07 / 1.57e-07    1.94e-07 / 1.94e-07
        384     384   1.68e-07 / 1.46e-07    1.62e-07 / 1.75e-07
        388     388   1.46e-07 / 1.46e-07    1.65e-07 / 1.65e-07
        512     512   1.35e-07 / 1.33e-07    1.76e-07 / 1.72e-07
        516     516   1.62e-07 / 1.18e-07    2.16e-07 / 2.16e-07
        768     768   1.36e-07 / 1.3e-07     1.67e-07 / 1.67e-07
        772     772   1.69e-07 / 1.48e-07    1.61e-07 / 1.49e-07
       1024    1024   1.65e-07 / 1.59e-07    1.44e-07 / 1.45e-07
        257     260   1.39e-07 / 1.42e-07    2.23e-07 / 2.23e-07

(d = 4, 3CosMul: one cos(a, v) of the 130 x 300 comes within 1e-3 of -1, so its denominator is eps plus a float32
rounding error of a cosine; the tolerance there is 5e-5 of the score, at every other width the project's own.)

Ids follow the `separated` rule of the analogy tests (gap 1e-5, at most 2 % of the positions left out, asserted on the
references alone in tests/test_row_shape_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_shape_cases as rc
from helpers import to_dev

pytestmark = pytest.mark.gpu
TABLE_IDS = ["d%d_stride%d" % t for t in rc.TABLES]


class RawTables:
    """glove_tables over the arrays of a case at a row stride of the test's choosing (DeviceTables picks its own)."""

    def __init__(self, tables, dm, device="cuda:0"):
        from trainer.hip_api import GloveTables
        R, C_, br, bc, g = tables
        self.device = torch.device(device)
        self.keep = to_dev(R, C_, br.astype(np.float32), bc.astype(np.float32), np.array([g] + [0.0] * 7, np.float32))
        self.s = GloveTables()
        self.s.V, self.s.d = R.shape
        self.s.d_model = 0 if dm == R.shape[1] else dm
        for name, t in zip(("R", "C", "br", "bc", "scalars"), self.keep):
            setattr(self.s, name, t.data_ptr())

    def struct(self):
        return self.s


@pytest.mark.parametrize("dm,stride", rc.TABLES, ids=TABLE_IDS)
def test_regression_eval_equals_float64(hip, dm, stride):
    tables = rc.eval_tables(dm, stride)
    dt = RawTables(tables, dm)
    row, col, w, y = rc.eval_batch(rc.B_EVAL)
    want = rc.regression_sums(tables, dm, row, col, w, y)
    sums = hip.eval_sums(*to_dev(row, col, w, y), dt)
    got = sums.cpu().numpy()
    print("d_model %d: sums %s, reference %s" % (dm, got, want))
    assert (got == want).all()                               # equality: every term and every partial sum is exact
    # a second call accumulates into the sums it is handed: first + second, exactly
    row2, col2, w2, y2 = rc.eval_batch(517, seed=1)
    want2 = rc.regression_sums(tables, dm, row2, col2, w2, y2)
    again = hip.eval_sums(*to_dev(row2, col2, w2, y2), dt, sums=sums)
    assert again.data_ptr() == sums.data_ptr() and (again.cpu().numpy() == want + want2).all()
    # one pair, and none
    one = hip.eval_sums(*to_dev(row[:1], col[:1], w[:1], y[:1]), dt).cpu().numpy()
    assert (one == rc.regression_sums(tables, dm, row[:1], col[:1], w[:1], y[:1])).all()
    before = sums.clone()
    hip.eval_sums(*to_dev(row[:0], col[:0], w[:0], y[:0]), dt, sums=sums)
    assert torch.equal(sums, before)


@pytest.mark.parametrize("dm,stride", rc.TABLES, ids=TABLE_IDS)
def test_logistic_eval_matches_float64(hip, dm, stride):
    row, col, pos, _ = rc.eval_batch(rc.B_EVAL)
    _, _, neg, _ = rc.eval_batch(rc.B_EVAL, seed=2)
    # plain tables: |p| of order 1 - 10, both softplus branches and the unsaturated sigmoid
    tables = rc.eval_tables(dm, stride)
    want = rc.logistic_sums(tables, dm, row, col, pos, neg)
    got = hip.eval_sums_logistic(*to_dev(row, col, pos, neg), RawTables(tables, dm)).cpu().numpy()
    print("d_model %d: largest relative deviation %.3g" % (dm, np.abs(got / want - 1).max()))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    # one row pair scaled up on each sign: |p| > 100, the six sums stay finite and within the same rtol
    sat, srow, scol = rc.saturated(tables, dm, row, col)
    want = rc.logistic_sums(sat, dm, srow, scol, pos, neg)
    got = hip.eval_sums_logistic(*to_dev(srow, scol, pos, neg), RawTables(sat, dm)).cpu().numpy()
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    empty = hip.eval_sums_logistic(*to_dev(row[:0], col[:0], pos[:0], neg[:0]), RawTables(tables, dm))
    assert (empty == 0).all()


def check_ids(path, got_i, want_s_ext, want_i_ext, what):
    clear = rc.separated(path, want_s_ext)
    assert 1.0 - clear.mean() <= rc.LEFT_OUT_MAX, what
    want_i = want_i_ext[:, :rc.K]
    assert (got_i[clear] == want_i[clear]).all(), (what, np.argwhere(clear & (got_i != want_i))[:5])


@pytest.mark.parametrize("dm,stride", rc.TABLES, ids=TABLE_IDS)
def test_predict_and_pair_cosine_on_exact_tables(hip, dm, stride):
    import cosmul_ref
    R, queries, pairs = rc.predict_case(dm, stride)
    want_s, want_i = rc.predict_reference(dm, stride)
    Rd, qd, pd = to_dev(R, queries, pairs)
    for n in (5, rc.N_QUERIES):                              # one query tile, and two
        sims, idx = hip.topk_cosine(Rd, qd[:n].contiguous(), rc.K)
        got_s, got_i = sims.cpu().numpy(), idx.cpu().numpy()
        print("d_model %d n %d: largest cosine deviation %.3g" % (dm, n, np.abs(got_s - want_s[:n, :rc.K]).max()))
        np.testing.assert_allclose(got_s, want_s[:n, :rc.K], rtol=rc.RTOL, atol=rc.ATOL)
        check_ids("predict", got_i, want_s[:n], want_i[:n], "predict d_model %d n %d" % (dm, n))
        assert (got_i[:, 0] == queries[:n]).all()
    got = hip.pair_cosine(Rd, pd).cpu().numpy()
    want = cosmul_ref.pair_cosine(R[:, :dm], pairs)
    print("d_model %d: largest pair cosine deviation %.3g" % (dm, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=rc.RTOL, atol=rc.ATOL)
    assert len(np.unique(want)) > 100 or dm == 4             # the pairs do not agree by accident


@pytest.mark.parametrize("path", ["cosadd", "cosmul"])
@pytest.mark.parametrize("dm,stride", rc.TABLES, ids=TABLE_IDS)
def test_analogy_paths_at_every_row_shape(hip, dm, stride, path):
    W, abc = rc.analogy_case(dm, stride)
    want_s, want_i = rc.analogy_reference(dm, stride, path)
    if path == "cosadd":
        sims, idx = hip.analogy_topk(*to_dev(W, abc), rc.K)
    else:
        sims, idx = hip.analogy_cosmul_topk(*to_dev(W, abc), rc.K, rc.COSMUL_EPS)
    got_s, got_i = sims.cpu().numpy(), idx.cpu().numpy()
    assert got_s.shape == got_i.shape == (rc.N_QUERIES, rc.K)
    want = want_s[:, :rc.K]
    print("d_model %d stride %d %s: float32 restatement deviates by %.3g, the kernel by %.3g"
          % (dm, stride, path, rc.restatement_deviation(dm, stride, path), rc.deviation(got_s, want)))
    assert np.isfinite(got_s).all() and (got_i >= 0).all()
    assert (np.abs(got_s - want) <= rc.allowed(dm, stride, path, want)).all()
    check_ids(path, got_i, want_s, want_i, "%s d_model %d" % (path, dm))
    assert not (got_i[:, :, None] == abc[:, None, :]).any()  # a, b and c are no answers
    assert (got_s[:, :-1] >= got_s[:, 1:]).all()             # descending


def test_one_float4_beyond_the_widest_shape_is_refused_and_nothing_launched(hip):
    """Stride 1028: all six entry points answer GLOVE_E_BADARG, and what they were handed to write to stays as it was."""
    from trainer.hip_api import GloveHipError, load_eval_library
    stride, V, n, k = rc.REFUSED_STRIDE, 64, 5, 3
    rng = np.random.default_rng(0)
    W = rng.standard_normal((V, stride)).astype(np.float32)
    dt = RawTables((W, W, W[:, 0], W[:, 1], 0.5), stride)
    row, col, w, y = to_dev(*rc.eval_batch(64, V=V))
    Wd, qd, abc, pairs = to_dev(W, np.arange(n, dtype=np.int32), np.arange(3 * n, dtype=np.int32).reshape(n, 3),
                                np.arange(2 * n, dtype=np.int32).reshape(n, 2))
    ev = load_eval_library()
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.full((6,), 7.25, dtype=torch.float64, device="cuda:0")
    out_s = torch.full((n, k), -3.5, device="cuda:0")
    out_i = torch.full((n, k), -9, dtype=torch.int32, device="cuda:0")
    ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda:0")      # room for any of the workspaces
    p = lambda t: t.data_ptr()
    calls = {
        "glove_eval_f32": lambda: hip.lib.glove_eval_f32(p(row), p(col), p(w), p(y), 64, C.byref(dt.struct()), p(sums), st),
        "glove_eval_logistic_f32": lambda: hip.lib.glove_eval_logistic_f32(p(row), p(col), p(w), p(w), 64,
                                                                          C.byref(dt.struct()), p(sums), st),
        "glove_topk_cosine_f32": lambda: hip.lib.glove_topk_cosine_f32(p(Wd), V, stride, p(qd), n, k, p(out_s), p(out_i),
                                                                      p(ws), ws.numel(), st),
        "glove_analogy_topk_f32": lambda: ev.glove_analogy_topk_f32(p(Wd), V, stride, p(abc), n, k, p(out_s), p(out_i),
                                                                    p(ws), ws.numel(), st),
        "glove_cosmul_topk_f32": lambda: ev.glove_cosmul_topk_f32(p(Wd), V, stride, p(abc), n, k, 1e-3, p(out_s), p(out_i),
                                                                  p(ws), ws.numel(), st),
        "glove_pair_cosine_f32": lambda: ev.glove_pair_cosine_f32(p(Wd), V, stride, p(pairs), n, p(out_s), st),
    }
    for name, call in calls.items():
        assert call() == -1, name                            # GLOVE_E_BADARG
    torch.cuda.synchronize()
    assert (sums == 7.25).all() and (out_s == -3.5).all() and (out_i == -9).all() and (ws == 0x5A).all()
    assert ev.glove_analogy_workspace_bytes(n, V, stride, k) == 0 and ev.glove_cosmul_workspace_bytes(n, V, stride, k) == 0
    # ... and through the binding: an error, never a result
    for call in (lambda: hip.eval_sums(row, col, w, y, dt), lambda: hip.eval_sums_logistic(row, col, w, w, dt),
                 lambda: hip.topk_cosine(Wd, qd, k), lambda: hip.analogy_topk(Wd, abc, k),
                 lambda: hip.analogy_cosmul_topk(Wd, abc, k), lambda: hip.pair_cosine(Wd, pairs)):
        with pytest.raises(GloveHipError, match="BADARG"):
            call()
    # the widest stride that is served, with the same arguments, is accepted
    ok = to_dev(W[:, :1024])[0]
    assert ev.glove_pair_cosine_f32(p(ok), V, 1024, p(pairs), n, p(out_s), st) == 0
    torch.cuda.synchronize()
    assert (out_s.flatten()[:n] != -3.5).all()
