"""glove_retrofit_rows_f32 on the GPU (include/glove_factor_graph_hip.h) against the restatement of tests/retrofit_ref.py, then
trainer.retrofit's driver and command line.

Bits.  On the exact tables of tests/retrofit_ref.py (Q^ from {+-1, +-2, +-3} / 8, beta null or a power of two, alpha in
{1/2, 1, 2}: tests/test_retrofit.py proves that every product beta q and t q^ is exact) the float32 restatement in NumPy
states the kernel bit for bit, divisions included, over several sweeps.  Every row shape of pick_row_shape at its first and
last width; rows of 0, 1, 3, 4, 5, 9, 23, 200 and 1,100 positions; a row that lists itself, a column listed twice.

General data.  Random normal tables, alpha = 0.7, beta in (0, 2], 10 sweeps, both schedules, against the float64 backend.
The bound is derived, not measured (retrofit_ref.error_bound): one update errs by at most eps = g(L + 3) max|Q^|, L the
longest row, g(k) = (k + 2) u / (1 - (k + 2) u), u = 2^-24; the update is a convex combination with weight 1 / (1 + alpha)
on the error its inputs had: |got - ref| <= eps (1 + 1 / alpha).  The largest error over the bound is printed."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pca_ref
import retrofit_ref as ref
from helpers import to_dev
from trainer.retrofit import level_schedule, retrofit_table

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
TABLE_IDS = ["d%d_stride%d" % t for t in ref.TABLES]
DEV = "cuda:0"


def dev_opt(a):
    return None if a is None else to_dev(a)[0]


def level_lists():
    row_ptr, col, _ = ref.graph()
    rows, offsets = level_schedule(row_ptr, col, ref.N)
    return ref.lists_of(rows, offsets)


def same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    wrong = np.argwhere(ref.bits(got) != ref.bits(want))
    assert len(wrong) == 0, ("(row, column) of the first wrong entries", wrong[:8].tolist(), "rows", np.unique(wrong[:, 0])[:16].tolist())


# ---- 1. bits, at every row shape
@pytest.mark.parametrize("k", range(len(ref.TABLES)), ids=TABLE_IDS)
def test_all_rows_out_of_place_equal_the_restatement(hip, k):
    dm, stride = ref.TABLES[k]
    row_ptr, col, lens = ref.graph()
    Q_hat_h, alpha, beta_h = ref.exact_case(k)
    Q_in_h, want = ref.exact_jacobi_step(k)
    rp, ci, Q_hat, Q_in = to_dev(row_ptr, col, Q_hat_h, Q_in_h)
    beta = dev_opt(beta_h)
    Q_out = torch.full_like(Q_hat, float("nan"))
    assert hip.retrofit_rows(rp, ci, beta, None, Q_hat, Q_in, Q_out, alpha) is Q_out
    same_bits(Q_out, want)
    got = Q_out.cpu().numpy()
    empty = np.flatnonzero(lens == 0)
    assert len(empty) >= 20 and np.array_equal(ref.bits(got[empty]), ref.bits(Q_in_h[empty]))      # copies: nothing unwritten
    assert (got[:, dm:] == 0.0).all()                                                              # the padding columns
    again = torch.full_like(Q_hat, float("nan"))
    hip.retrofit_rows(rp, ci, beta, None, Q_hat, Q_in, again, alpha)
    assert torch.equal(Q_out.view(torch.int32), again.view(torch.int32))                           # bitwise repeatable
    assert torch.equal(Q_in.cpu(), torch.from_numpy(Q_in_h)) and torch.equal(Q_hat.cpu(), torch.from_numpy(Q_hat_h))


@pytest.mark.parametrize("k", range(len(ref.TABLES)), ids=TABLE_IDS)
def test_a_list_out_of_place_touches_the_listed_rows_only(hip, k):
    row_ptr, col, lens = ref.graph()
    Q_hat_h, alpha, beta_h = ref.exact_case(k)
    Q_in_h, want = ref.exact_jacobi_step(k)
    listed = np.array(sorted(set(range(1, ref.N, 3)) | set(ref.SPECIAL)), np.int32)
    assert (lens[listed] == 0).sum() >= 5
    unlisted = np.setdiff1d(np.arange(ref.N), listed)
    rp, ci, Q_hat, Q_in, rows = to_dev(row_ptr, col, Q_hat_h, Q_in_h, listed)
    Q_out = torch.full_like(Q_hat, -7.0)
    hip.retrofit_rows(rp, ci, dev_opt(beta_h), rows, Q_hat, Q_in, Q_out, alpha)
    got = Q_out.cpu().numpy()
    assert (got[unlisted] == -7.0).all()
    same_bits(got[listed], want[listed])                    # (listed rows without positions: copies of Q_in)


@pytest.mark.parametrize("k", range(len(ref.TABLES)), ids=TABLE_IDS)
def test_levels_in_place_equal_the_scalar_sequential_loop(hip, k):
    dm, stride = ref.TABLES[k]
    row_ptr, col, _ = ref.graph()
    Q_hat_h, alpha, beta_h = ref.exact_case(k)
    rp, ci, Q_hat = to_dev(row_ptr, col, Q_hat_h)
    beta = dev_opt(beta_h)
    lists = [to_dev(rows)[0] for rows in level_lists()]
    print("d_model %d stride %d: %d levels, the largest of %d rows" % (dm, stride, len(lists), max(len(r) for r in lists)))
    Q = Q_hat.clone()
    for _ in range(ref.ITERATIONS):
        for rows in lists:
            hip.retrofit_rows(rp, ci, beta, rows, Q_hat, Q, Q, alpha)
    same_bits(Q, ref.exact_sequential(k))
    assert (Q[:, dm:] == 0.0).all()


# ---- 2. the grid
@pytest.mark.parametrize("dm,stride", [(4, 4), (300, 304), (1024, 1024)])
def test_a_rows_bits_do_not_depend_on_the_list(hip, dm, stride):
    """A row alone, in its level and in the all-rows call: the same bits, on normal data (any other summation order
    would show)."""
    row_ptr, col, beta_h, Q_hat_h, alpha = ref.general_case(dm, stride)
    rows_h, offsets = level_schedule(row_ptr, col, ref.N)
    rp, ci, beta, Q_hat = to_dev(row_ptr, col, beta_h, Q_hat_h)
    Q_in = torch.roll(Q_hat, 1, 0).contiguous()
    whole = hip.retrofit_rows(rp, ci, beta, None, Q_hat, Q_in, torch.full_like(Q_hat, -7.0), alpha)
    for level in ref.lists_of(rows_h, offsets)[:3]:
        rows = to_dev(level)[0]
        part = hip.retrofit_rows(rp, ci, beta, rows, Q_hat, Q_in, torch.full_like(Q_hat, -7.0), alpha)
        assert torch.equal(part[rows.long()].view(torch.int32), whole[rows.long()].view(torch.int32))
        for i in (int(level[0]), int(level[-1])):
            one = hip.retrofit_rows(rp, ci, beta, torch.tensor([i], dtype=torch.int32, device=DEV), Q_hat, Q_in,
                                    torch.full_like(Q_hat, -7.0), alpha)
            assert torch.equal(one[i].view(torch.int32), whole[i].view(torch.int32))
            assert (one[:i] == -7.0).all() and (one[i + 1:] == -7.0).all()
    i = 5                                                   # the row of 200 positions
    one = hip.retrofit_rows(rp, ci, beta, torch.tensor([i], dtype=torch.int32, device=DEV), Q_hat, Q_in, torch.full_like(Q_hat, -7.0), alpha)
    assert row_ptr[i + 1] - row_ptr[i] == 200 and torch.equal(one[i].view(torch.int32), whole[i].view(torch.int32))


# ---- 3. general data
@pytest.mark.parametrize("schedule", ["sequential", "jacobi"])
@pytest.mark.parametrize("dm,stride", [(64, 64), (300, 304)])
def test_general_data_within_the_derived_bound(hip, dm, stride, schedule):
    row_ptr, col, beta, Q_hat, alpha = ref.general_case(dm, stride)
    W = Q_hat[:, :dm]
    want = retrofit_table(W, row_ptr, col, iterations=10, alpha=alpha, beta=beta, schedule=schedule, backend=ref.NumpyBackend())
    got = retrofit_table(W, row_ptr, col, iterations=10, alpha=alpha, beta=beta, schedule=schedule, backend=hip)
    assert got["Y"].dtype == np.float32 and want["Y"].dtype == np.float64 and got["Y"].shape == want["Y"].shape == (ref.N, dm)
    L = int(np.diff(row_ptr).max())
    bound = ref.error_bound(L, alpha, float(np.abs(W).max()))
    err = np.abs(got["Y"].astype(np.float64) - want["Y"]).max()
    print("d_model %d, %s: longest row %d, largest error %.3g, bound %.3g, error / bound %.3g" % (dm, schedule, L, err, bound, err / bound))
    assert L == 200 and err <= bound
    assert (got["levels"], got["largest_level"], got["rows_updated"]) == (want["levels"], want["largest_level"], want["rows_updated"])
    assert abs(got["shift_mean"] - want["shift_mean"]) <= 1e-5 * want["shift_mean"]
    assert not np.array_equal(got["Y"], W)


# ---- 4. ids out of range
def test_ids_out_of_range_are_skipped(hip):
    """What the header promises to tolerate, nothing beyond it: a listed id of -1 and one of n are skipped; a column of -1
    and one of n add nothing and do not count towards w.  The tables sit between guard words."""
    n, d, guard = 40, 64, 4096
    rng = np.random.default_rng(3)
    Q_hat_h = rng.choice(ref.LEVELS, (n, d))
    Q_in_h = np.roll(Q_hat_h, 1, axis=0).copy()
    lens = np.full(n, 5, np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(10, n, int(row_ptr[-1])).astype(np.int32)      # (no listed row is a column: the in-place contract)
    clean = col.copy()
    # row 3: two columns out of range among five (the four-in-flight trip and the tail); row 4: all five; row 6: one
    col[row_ptr[3] + 1], col[row_ptr[3] + 4] = -1, n
    col[row_ptr[4]:row_ptr[5]] = [n, -1, n + 7, -2 ** 31, 2 ** 31 - 1]
    col[row_ptr[6] + 2] = n
    want = np.full((n, d), -7.0, np.float32)
    listed = np.array([-1, 3, 4, n, 6, 9, 2 ** 31 - 1, -2 ** 31], np.int32)
    ref.update_rows(row_ptr, col, None, listed, Q_hat_h, Q_in_h, want, 1.0)
    # the restatement skips what the header says is skipped: row 3 is the mean over its three columns in range
    a = row_ptr[3]
    three = Q_in_h[clean[[a, a + 2, a + 3]]]
    assert np.array_equal(want[3], ((np.float32(3) * Q_hat_h[3] + (three[0] + three[1] + three[2])) / np.float32(6)))
    assert np.array_equal(want[4], Q_in_h[4])               # w == 0: a copy

    buf = torch.full((3 * guard + 2 * n * d,), -7.0, device=DEV)      # guard | Q_in | guard | Q_out | guard
    Q_in = buf[guard:guard + n * d].view(n, d)
    Q_out = buf[2 * guard + n * d:2 * guard + 2 * n * d].view(n, d)
    Q_in.copy_(torch.from_numpy(Q_in_h))
    rp, ci, Q_hat, rows = to_dev(row_ptr, col, Q_hat_h, listed)
    hip.retrofit_rows(rp, ci, None, rows, Q_hat, Q_in, Q_out, 1.0)
    torch.cuda.synchronize()
    same_bits(Q_out, want)
    assert (Q_out[[0, 1, 2, 5, 7, 8]] == -7.0).all()
    for a, b in ((0, guard), (guard + n * d, 2 * guard + n * d), (2 * guard + 2 * n * d, 3 * guard + 2 * n * d)):
        assert (buf[a:b] == -7.0).all()                     # the guard words
    assert torch.equal(Q_in.cpu(), torch.from_numpy(Q_in_h))
    # in place, the same ids
    hip.retrofit_rows(rp, ci, None, rows, Q_hat, Q_in, Q_in, 1.0)
    inplace = Q_in_h.copy()
    for i in (3, 4, 6, 9):                                  # (none of them a column in range of another: the contract)
        assert not np.isin(col[row_ptr[i]:row_ptr[i + 1]], [j for j in (3, 4, 6, 9) if j != i]).any()
    ref.update_rows(row_ptr, col, None, listed, Q_hat_h, inplace, inplace, 1.0)
    same_bits(Q_in, inplace)
    for a, b in ((0, guard), (guard + n * d, 2 * guard + n * d), (2 * guard + 2 * n * d, 3 * guard + 2 * n * d)):
        assert (buf[a:b] == -7.0).all()


# ---- 5. refusals
def test_refusals_return_without_a_launch(hip):
    from trainer.hip_api import GloveHipError, load_factor_library
    lib = load_factor_library()
    row_ptr, col, _ = ref.graph()
    Q_hat_h, alpha, _ = ref.exact_case(0)
    n, d = Q_hat_h.shape
    rp, ci, Q_hat = to_dev(row_ptr, col, Q_hat_h)
    Q_in = Q_hat.clone()
    Q_out = torch.full_like(Q_hat, -7.0)
    rows = torch.arange(5, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    nnz = len(col)

    def call(row_ptr=rp, col_idx=ci, beta=None, n=n, nnz=nnz, rows=rows, n_list=5, Q_hat=Q_hat, Q_in=Q_in, Q_out=Q_out, d=d, alpha=1.0):
        return lib.glove_retrofit_rows_f32(p(row_ptr), p(col_idx), p(beta), n, nnz, p(rows), n_list, p(Q_hat), p(Q_in), p(Q_out),
                                           d, alpha, st)
    BAD = -1
    for change in (dict(row_ptr=None), dict(col_idx=None), dict(Q_hat=None), dict(Q_in=None), dict(Q_out=None), dict(n=0),
                   dict(d=0), dict(d=34), dict(d=1028), dict(n_list=n + 1), dict(rows=None), dict(rows=None, n_list=n - 1),
                   dict(alpha=-0.5), dict(alpha=float("nan")), dict(Q_hat=Q_out)):
        assert call(**change) == BAD, change
    assert call(n_list=0) == 0
    torch.cuda.synchronize()
    assert (Q_out == -7.0).all()                            # nothing ran
    assert call() == 0                                      # (the call they were changes of runs)
    torch.cuda.synchronize()
    assert (Q_out[:5] != -7.0).all() and (Q_out[5:] == -7.0).all()
    # ... and the binding's own checks
    beta = torch.ones(nnz, device=DEV)
    for args in ((rp, ci, beta, rows, Q_hat.double(), Q_in, Q_out, 1.0),
                 (rp, ci, beta, rows, Q_hat, Q_in[:, :d - 4], Q_out, 1.0),
                 (rp, ci, beta, rows, Q_hat, Q_in, Q_out[:, :d - 2], 1.0),
                 (rp[:-1], ci, beta, rows, Q_hat, Q_in, Q_out, 1.0),
                 (rp.int(), ci, beta, rows, Q_hat, Q_in, Q_out, 1.0),
                 (rp, ci.long(), beta, rows, Q_hat, Q_in, Q_out, 1.0),
                 (rp, ci, beta[:-1], rows, Q_hat, Q_in, Q_out, 1.0),
                 (rp, ci, beta, rows.long(), Q_hat, Q_in, Q_out, 1.0),
                 (rp, ci, beta, torch.zeros(n + 1, dtype=torch.int32, device=DEV), Q_hat, Q_in, Q_out, 1.0),
                 (rp, ci, beta, rows, Q_hat, Q_in, Q_out, -1.0),
                 (rp, ci, beta, rows, Q_hat, Q_in, Q_out, float("nan")),
                 (rp.cpu(), ci, beta, rows, Q_hat, Q_in, Q_out, 1.0)):
        with pytest.raises(GloveHipError):
            hip.retrofit_rows(*args)
    with pytest.raises(GloveHipError, match="GLOVE_E_BADARG"):
        hip.retrofit_rows(rp, ci, beta, rows, Q_hat, Q_in, Q_hat, 1.0)


# ---- 6. the driver
def planted_synonyms(n=300, sets=40, size=5, seed=0):
    """A planted table (pca_ref.planted) and `sets` disjoint synonym sets of `size` words each listing the others."""
    W = pca_ref.planted(seed=seed, n=n)[0]
    rng = np.random.default_rng(seed + 1)
    members = rng.permutation(n)[:sets * size].reshape(sets, size)
    lists = {int(i): [int(j) for j in group if j != i] for group in members for i in group}
    lens = np.array([len(lists.get(i, ())) for i in range(n)], np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.array([j for i in range(n) for j in lists.get(i, ())], np.int32)
    return W, row_ptr, col, members


def mean_cosine_inside(Y, members):
    U = Y / np.linalg.norm(Y, axis=1, keepdims=True)
    size = members.shape[1]
    return float(np.mean([(U[g] @ U[g].T)[~np.eye(size, dtype=bool)].mean() for g in members]))


@pytest.mark.parametrize("schedule", ["sequential", "jacobi"])
def test_driver_pulls_planted_synonyms_together(hip, schedule):
    W, row_ptr, col, members = planted_synonyms()
    f64 = retrofit_table(W, row_ptr, col, schedule=schedule, backend=ref.NumpyBackend())
    got = retrofit_table(W, row_ptr, col, schedule=schedule, backend=hip)
    before, after = mean_cosine_inside(W.astype(np.float64), members), mean_cosine_inside(got["Y"].astype(np.float64), members)
    bound = ref.error_bound(4, 1.0, float(np.abs(W).max()))
    err = np.abs(got["Y"].astype(np.float64) - f64["Y"]).max()
    print("%s: mean cosine inside the sets %.3f -> %.3f; largest error %.3g, error / bound %.3g" % (schedule, before, after, err, err / bound))
    assert after > before and err <= bound
    assert got["rows_updated"] == members.size and got["longest_row"] == 4 and got["levels"] == 5      # a clique of five: five levels
    rest = np.setdiff1d(np.arange(len(W)), members)
    assert np.array_equal(ref.bits(got["Y"][rest]), ref.bits(W[rest]))


@pytest.mark.parametrize("schedule", ["sequential", "jacobi"])
@pytest.mark.parametrize("k", [1, 6, 14], ids=[TABLE_IDS[k] for k in (1, 6, 14)])
def test_driver_on_the_exact_table_equals_the_float32_backend(hip, k, schedule):
    dm, stride = ref.TABLES[k]
    row_ptr, col, _ = ref.graph()
    Q_hat, alpha, beta = ref.exact_case(k)
    W = Q_hat[:, :dm]
    settings = dict(iterations=ref.ITERATIONS, alpha=alpha, beta=beta, schedule=schedule)
    want = retrofit_table(W, row_ptr, col, backend=ref.NumpyBackend(float32=True), **settings)
    got = retrofit_table(W, row_ptr, col, backend=hip, **settings)
    same_bits(got["Y"], want["Y"])
    if schedule == "sequential":
        same_bits(got["Y"], ref.exact_sequential(k)[:, :dm])
    for key in ("levels", "largest_level", "longest_row", "rows_updated"):
        assert got[key] == want[key], key
    assert got["longest_row"] == 1100 and got["rows_updated"] == int((np.diff(row_ptr) > 0).sum())
    for key in ("shift_mean", "shift_max"):                 # (float64 norms of the same float32 rows, summed in another order)
        assert abs(got[key] - want[key]) <= 1e-12 * want[key], key


# ---- 7. end to end
def test_cli_end_to_end(hip, tmp_path):
    """`python -m trainer.retrofit` (a child process) on a job directory, then `python -m trainer.wordsim` on its output
    directory."""
    from trainer.config_utils import build_parser, init_params
    from trainer.data_utils import read_vocab
    from trainer.hip_api import DeviceTables
    from trainer.retrofit import read_lexicon
    from trainer.train_utils import CheckpointManager
    vocab = read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))
    V = len(vocab)
    job, P = tmp_path / "job", tmp_path / "P"
    job.mkdir()
    (job / "vocab.txt").write_bytes("\n".join(vocab).encode())
    params = init_params(vars(build_parser().parse_args([
        "--vocab-txt", str(job / "vocab.txt"), "--job-dir", str(job), "--disable-datetime-path", "--embedding-size", "24",
        "--optimizer", "Adagrad"])).copy())
    W = pca_ref.planted(seed=1, n=V)[0]
    tables = DeviceTables(V, 24, "Adagrad", device="cpu", seed=0)
    tables.embeddings("R").copy_(torch.from_numpy(W))
    tables.embeddings("C").zero_()
    CheckpointManager(params["job_dir"]).save(tables)
    words = [w for w in vocab if w != "<UNK>"]
    lexicon = tmp_path / "lexicon.txt"
    lexicon.write_text("".join("%s %s %s notaword\n" % (words[i], words[i + 1], words[(i + 7) % len(words)]) for i in range(0, 40, 2)))

    proc = subprocess.run([sys.executable, "-m", "trainer.retrofit", "--job-dir", str(job), "--lexicon", str(lexicon),
                           "--output-dir", str(P), "--iterations", "5", "--optimizer", "Adagrad"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    blob = torch.load(P / "model.ckpt-0.pt", weights_only=False)["tables"]
    rec = json.loads((P / "retrofit.json").read_text())
    assert int(blob["global_step"]) == 0 and blob["R"].shape == (V, 24) and not blob["C"].any()
    assert (rec["iterations"], rec["schedule"], rec["rows_updated"], rec["longest_row"]) == (5, "sequential", 20, 2)
    assert rec["lexicon_counts"]["neighbours_out_of_vocab"] == 20 and rec["shift_mean"] > 0
    assert json.loads((P / "params.json").read_text())["embedding_size"] == 24
    row_ptr, col, _ = read_lexicon(lexicon, vocab)
    f32 = retrofit_table(W, row_ptr, col, iterations=5, backend=ref.NumpyBackend(float32=True))
    f64 = retrofit_table(W, row_ptr, col, iterations=5, backend=ref.NumpyBackend())
    err = np.abs(blob["R"].numpy().astype(np.float64) - f64["Y"]).max()
    bound = ref.error_bound(2, 1.0, float(np.abs(W).max()))
    print("command line: largest error %.3g, error / bound %.3g; NumPy float32 from float64 %.3g" % (
        err, err / bound, np.abs(f32["Y"] - f64["Y"]).max()))
    assert err <= bound

    pairs = [(words[0], w) for w in words[1:11]]
    pfile = tmp_path / "pairs.tab"
    pfile.write_text("".join("%s\t%s\t%.1f\n" % (a, b, 10 - k_) for k_, (a, b) in enumerate(pairs)))
    proc = subprocess.run([sys.executable, "-m", "trainer.wordsim", "--job-dir", str(P), "--pairs", str(pfile), "--no-lowercase"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    out = json.loads((P / "eval" / "wordsim.json").read_text())
    assert (out["pairs_total"], out["pairs_seen"], out["skipped"], out["global_step"]) == (10, 10, 0, 0)
