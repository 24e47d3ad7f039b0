"""trainer.retrofit on the CPU: the ABI of include/glove_factor_graph_hip.h, the lexicon reader, the level schedule, the
claim the design rests on (the levels, one after the other, ARE the sequential sweep, bit for bit), the semantics of the
update with the NumPy backend of tests/retrofit_ref.py, and the command line's job directory.  The kernel itself:
tests/test_gpu_retrofit.py."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import retrofit_ref as ref
from trainer import retrofit
from trainer.retrofit import level_schedule, read_lexicon, retrofit_table

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "glove_factor_graph_hip.h"
GOLDEN = REPO / "tests" / "golden"
F32, F64 = np.float32, np.float64


# ---- 1. the ABI
@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.FACTOR_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_factor_library()


def declared_functions():
    """name -> number of parameters of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return {name: 0 if args.strip() == "void" else args.count(",") + 1
            for name, args in re.findall(r"\b(glove_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_header_and_the_binding_declare_the_same_two_functions(lib):
    from trainer import hip_api
    declared = declared_functions()
    protos = hip_api.factor_graph_prototypes()
    assert set(declared) == set(protos) == set(hip_api.FACTOR_GRAPH_EXPORTED_SYMBOLS)
    assert set(declared) == {"glove_factor_graph_abi_version", "glove_retrofit_rows_f32"}
    assert declared == {name: len(args) for name, (_, args) in protos.items()}
    assert declared["glove_retrofit_rows_f32"] == 13
    for name in declared:
        assert hasattr(lib, name), name
    every = {k: v for k, v in vars(hip_api).items() if k.endswith("EXPORTED_SYMBOLS")}
    assert len(every) >= 12 and "FACTOR_EXPORTED_SYMBOLS" in every and "EXPORTED_SYMBOLS" in every
    for k, names in every.items():
        if k != "FACTOR_GRAPH_EXPORTED_SYMBOLS":
            assert not set(declared) & set(names), k
    assert not set(protos) & (set(hip_api.factor_prototypes()) | set(hip_api.factor_dense_prototypes()))
    assert lib.glove_factor_graph_abi_version() == hip_api.GLOVE_FACTOR_GRAPH_ABI_VERSION == 1
    assert "#define GLOVE_FACTOR_GRAPH_ABI_VERSION 1" in HEADER.read_text()


def test_argument_errors_come_back_before_any_launch(lib):
    """Null pointers and sizes out of range: the answer is GLOVE_E_BADARG, nothing is enqueued (no device is needed)."""
    call = lib.glove_retrofit_rows_f32
    rp, ci, rows, qh, qi, qo = 16, 32, 48, 64, 80, 96      # (never dereferenced)
    good = dict(row_ptr=rp, col_idx=ci, beta=None, n=10, nnz=5, rows=rows, n_list=3, Q_hat=qh, Q_in=qi, Q_out=qo, d=8, alpha=1.0)

    def rc(**change):
        a = dict(good, **change)
        return call(a["row_ptr"], a["col_idx"], a["beta"], a["n"], a["nnz"], a["rows"], a["n_list"], a["Q_hat"], a["Q_in"],
                    a["Q_out"], a["d"], a["alpha"], None)
    for change in (dict(row_ptr=None), dict(col_idx=None), dict(Q_hat=None), dict(Q_in=None), dict(Q_out=None), dict(n=0),
                   dict(n=-1), dict(nnz=-1), dict(nnz=2 ** 31), dict(d=0), dict(d=34), dict(d=1028), dict(d=-4), dict(n_list=11),
                   dict(n_list=-1), dict(rows=None), dict(rows=None, n_list=0), dict(alpha=-0.5), dict(alpha=float("nan")),
                   dict(alpha=float("inf")), dict(Q_out=qh)):
        assert rc(**change) == -1, change
    assert rc(n_list=0) == 0                                # nothing to do: no launch
    assert rc(n_list=0, Q_out=qi) == 0
    assert rc(n_list=0, nnz=0, col_idx=None) == 0           # (no positions: col_idx may be null)


# ---- 2. the lexicon reader
VOCAB = ["the", "cat", "dog", "Paris", "paris", "feline", "puppy", "hound"]


def write(tmp_path, text):
    p = tmp_path / "lexicon.txt"
    p.write_text(text)
    return p


def rows_of(row_ptr, col_idx):
    return {i: col_idx[a:b].tolist() for i, (a, b) in enumerate(zip(row_ptr[:-1], row_ptr[1:])) if b > a}


def test_read_lexicon_cases(tmp_path):
    text = ("cat feline kitten cat\n"            # a neighbour outside the vocabulary; a self-listing (kept)
            "\n"                                 # an empty line: not a line
            "wolf dog hound\n"                   # a key outside the vocabulary: the line is dropped
            "dog puppy hound puppy\n"            # a duplicate neighbour: the first stays
            "   \t \n"
            "cat the feline\n"                   # a repeated key: merged in file order, `feline` a duplicate across lines
            "Dog cat\n"                          # folded to dog: merged as well
            "hound zebra\n"                      # a key whose neighbours are all outside: a row without positions
            "PARIS the\n")
    row_ptr, col_idx, counts = read_lexicon(write(tmp_path, text), VOCAB)
    assert row_ptr.dtype == np.int64 and col_idx.dtype == np.int32 and row_ptr.shape == (len(VOCAB) + 1,)
    assert rows_of(row_ptr, col_idx) == {1: [5, 1, 0], 2: [6, 7, 1], 4: [0]}      # paris (folded) is id 4, not "Paris"
    assert counts == dict(lines=7, keys_in_vocab=4, keys_out_of_vocab=1, neighbours_kept=7, neighbours_out_of_vocab=2,
                          duplicate_neighbours=2, rows=3)
    # as written: `Dog` and `PARIS` are no words of the vocabulary
    row_ptr, col_idx, counts = read_lexicon(write(tmp_path, text), VOCAB, lowercase=False)
    assert rows_of(row_ptr, col_idx) == {1: [5, 1, 0], 2: [6, 7]}
    assert counts == dict(lines=7, keys_in_vocab=3, keys_out_of_vocab=3, neighbours_kept=5, neighbours_out_of_vocab=2,
                          duplicate_neighbours=2, rows=2)
    row_ptr, col_idx, counts = read_lexicon(write(tmp_path, "Paris paris\n"), VOCAB, lowercase=False)
    assert rows_of(row_ptr, col_idx) == {3: [4]}
    row_ptr, col_idx, counts = read_lexicon(write(tmp_path, "\n\n"), VOCAB)
    assert (row_ptr == 0).all() and len(col_idx) == 0 and counts["lines"] == counts["rows"] == 0


# ---- 3. the level schedule
def random_digraph(rng, n):
    """Asymmetric edges, self loops, empty rows, repeated columns."""
    lens = rng.choice([0, 0, 1, 2, 3, 5], n)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, n, int(row_ptr[-1])).astype(np.int32)
    for i in rng.choice(n, max(1, n // 10), replace=False):
        a, b = row_ptr[i], row_ptr[i + 1]
        if b - a >= 1:
            col[a] = i                                      # a self loop
        if b - a >= 3:
            col[a + 2] = col[a + 1]                         # a repeated column
    return row_ptr, col


def levels_of(rows_by_level, offsets, n):
    level = np.full(n, -1)
    for l, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        level[rows_by_level[a:b]] = l
    return level


@pytest.mark.parametrize("seed", range(12))
def test_level_schedule_constraints_on_random_digraphs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 201))
    row_ptr, col = random_digraph(rng, n)
    rows, offsets = level_schedule(row_ptr, col, n)
    assert rows.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == len(rows) and (np.diff(offsets) > 0).all()
    in_u = np.diff(row_ptr) > 0
    assert sorted(rows.tolist()) == np.flatnonzero(in_u).tolist()                # each row of U once, the others nowhere
    for a, b in zip(offsets[:-1], offsets[1:]):
        assert (np.diff(rows[a:b]) > 0).all()                                    # ascending ids inside a level
    level = levels_of(rows, offsets, n)
    adjacent = np.zeros((n, n), bool)
    for i in range(n):
        for c in col[row_ptr[i]:row_ptr[i + 1]]:
            if c != i and in_u[c]:
                adjacent[i, c] = adjacent[c, i] = True
    for j in np.flatnonzero(in_u):
        below = np.flatnonzero(adjacent[j, :j])
        assert (level[below] < level[j]).all()                                   # level(j) > level(i) for i < j
        assert level[j] == (1 + level[below].max() if len(below) else 0)         # ... and the least such: the longest path


def test_level_schedule_chain_star_and_empty():
    k = 9
    # a chain 0 - 1 - ... - k, each row listing the next one only (the last row lists its predecessor)
    row_ptr = np.arange(k + 2, dtype=np.int64)
    col = np.array(list(range(1, k + 1)) + [k - 1], np.int32)
    rows, offsets = level_schedule(row_ptr, col, k + 1)
    assert len(offsets) - 1 == k + 1 and rows.tolist() == list(range(k + 1))
    # a star: the hub lists every leaf and every leaf the hub; hub first, hub last
    for hub in (0, k):
        leaves = [i for i in range(k + 1) if i != hub]
        lists = {i: [hub] for i in leaves}
        lists[hub] = leaves
        lens = [len(lists[i]) for i in range(k + 1)]
        row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col = np.array([c for i in range(k + 1) for c in lists[i]], np.int32)
        rows, offsets = level_schedule(row_ptr, col, k + 1)
        assert len(offsets) - 1 == 2
        assert ref.lists_of(rows, offsets)[0 if hub == 0 else 1].tolist() == [hub]
    # a star whose leaves list nothing: they are constants and appear nowhere
    row_ptr = np.array([0] + [k] * (k + 1), np.int64)
    rows, offsets = level_schedule(row_ptr, np.arange(1, k + 1, dtype=np.int32), k + 1)
    assert rows.tolist() == [0] and offsets.tolist() == [0, 1]
    # nothing at all; columns out of range count for nothing
    rows, offsets = level_schedule(np.zeros(4, np.int64), np.zeros(0, np.int32), 3)
    assert len(rows) == 0 and offsets.tolist() == [0]
    rows, offsets = level_schedule(np.array([0, 2, 3], np.int64), np.array([-1, 2, 5], np.int32), 2)
    assert rows.tolist() == [0, 1] and offsets.tolist() == [0, 2]
    with pytest.raises(ValueError):
        level_schedule(np.array([0, 2, 1], np.int64), np.zeros(1, np.int32), 2)


# ---- 4. the claim the design rests on
def test_products_of_the_exact_tables_are_exact():
    """What makes a * b + c in NumPy the kernel's fmaf: on every operand the three sweeps meet, beta q and t q^ are float32
    numbers.  Proved on the reference alone, table by table."""
    row_ptr, col, lens = ref.graph()
    assert sorted(set(ref.ROW_LENGTHS)) == sorted(set(lens[list(ref.SPECIAL)].tolist()))
    assert ref.SELF_ROW in col[row_ptr[ref.SELF_ROW]:row_ptr[ref.SELF_ROW + 1]]
    a = row_ptr[ref.REPEAT_ROW]
    assert col[a] == col[a + 1]
    seen = set()
    for k in range(len(ref.TABLES)):
        Q_hat, alpha, beta = ref.exact_case(k)
        seen.add((alpha, beta is None))
        dm, stride = ref.TABLES[k]
        assert (Q_hat[:, dm:] == 0).all() and np.isin(Q_hat[:, :dm], ref.LEVELS).all()
        b32 = np.ones(len(col), F32) if beta is None else beta
        assert np.isin(b32, ref.BETAS).all()
        w = np.array([b32[x:y].astype(F64).sum() for x, y in zip(row_ptr[:-1], row_ptr[1:])])
        assert (w == w.astype(F32)).all() and w.max() <= 2200
        t = alpha * w
        assert (t == t.astype(F32)).all() and ((t + w) == (t + w).astype(F32)).all()
        tq = t[:, None] * Q_hat.astype(F64)
        assert (tq == tq.astype(F32)).all()                                      # t q^: exact
        # beta q on every table a sweep reads or leaves — Q^ and the results of sweeps 1, 2 and 3: a power of two times a
        # float32 number that stays far from the ends of the exponent range
        for Q in (Q_hat, ref.sequential_sweeps(row_ptr, col, beta, Q_hat, alpha, 1), ref.exact_sequential(k)):
            assert np.isfinite(Q).all() and np.abs(Q).max() <= 3 / 8             # convex combinations of Q^'s entries
            assert np.abs(Q[Q != 0]).min() >= 2.0 ** -100
            for bv in ref.BETAS:
                prod = F64(bv) * Q.astype(F64)
                assert (prod == prod.astype(F32)).all()
    assert seen == {(al, nb) for al in ref.ALPHAS for nb in (True, False)}


@pytest.mark.parametrize("k", range(len(ref.TABLES)), ids=["d%d_stride%d" % t for t in ref.TABLES])
def test_levels_in_place_equal_the_sequential_sweep_bit_for_bit(k):
    row_ptr, col, _ = ref.graph()
    Q_hat, alpha, beta = ref.exact_case(k)
    rows, offsets = level_schedule(row_ptr, col, ref.N)
    assert len(offsets) - 1 >= 3
    got = ref.level_sweeps(row_ptr, col, beta, Q_hat, alpha, ref.ITERATIONS, ref.lists_of(rows, offsets))
    want = ref.exact_sequential(k)
    assert got.dtype == want.dtype == F32
    assert np.array_equal(ref.bits(got), ref.bits(want))
    assert not np.array_equal(got, Q_hat)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_levels_equal_the_sequential_sweep_on_normal_data(dtype):
    row_ptr, col, beta, Q_hat, alpha = ref.general_case(36, 36)
    Q_hat, beta = Q_hat.astype(dtype), beta.astype(dtype)
    rows, offsets = level_schedule(row_ptr, col, ref.N)
    got = ref.level_sweeps(row_ptr, col, beta, Q_hat, alpha, 3, ref.lists_of(rows, offsets))
    want = ref.sequential_sweeps(row_ptr, col, beta, Q_hat, alpha, 3)
    assert np.array_equal(ref.bits(got), ref.bits(want))
    # ... and the driver runs exactly these calls
    out = retrofit_table(Q_hat, row_ptr, col, iterations=3, alpha=alpha, beta=beta, backend=ref.NumpyBackend(float32=dtype is F32))
    assert out["Y"].dtype == dtype and np.array_equal(ref.bits(out["Y"]), ref.bits(want))
    # an order that is not the vocabulary's gives other bits: the claim is not empty
    other = ref.level_sweeps(row_ptr, col, beta, Q_hat, alpha, 3, ref.lists_of(rows, offsets)[::-1])
    assert not np.array_equal(other, want)


# ---- 5. semantics
def test_three_word_example_by_hand():
    """cat: [1, 0], feline: [0, 1], dog: [4, 4]; cat lists feline and dog, feline lists cat, dog nothing.  alpha = 1:
    cat <- (2 cat^ + feline + dog) / 4 = [1.5, 1.25]; then feline <- (feline^ + cat) / 2 = [0.75, 1.125] in the
    sequential sweep (the new cat) and [0.5, 0.5] in the Jacobi sweep (the old one)."""
    W = np.array([[1, 0], [0, 1], [4, 4]], F64)
    row_ptr, col = np.array([0, 2, 3, 3], np.int64), np.array([1, 2, 0], np.int32)
    seq = retrofit_table(W, row_ptr, col, iterations=1, backend=ref.NumpyBackend())
    assert seq["Y"].tolist() == [[1.5, 1.25], [0.75, 1.125], [4.0, 4.0]]
    assert (seq["levels"], seq["largest_level"], seq["longest_row"], seq["rows_updated"]) == (2, 1, 2, 2)
    jac = retrofit_table(W, row_ptr, col, iterations=1, schedule="jacobi", backend=ref.NumpyBackend())
    assert jac["Y"].tolist() == [[1.5, 1.25], [0.5, 0.5], [4.0, 4.0]]
    moved = [np.hypot(0.5, 1.25), np.hypot(0.75, 0.125)]
    assert abs(seq["shift_mean"] - np.mean(moved)) <= 1e-15 and abs(seq["shift_max"] - max(moved)) <= 1e-15
    assert {"schedule", "upload", "sweeps", "download"} <= set(seq["seconds"])
    # alpha = 3 and weights: cat <- (3 * 2.5 cat^ + 2 feline + 0.5 dog) / (7.5 + 2.5) = [0.95, 0.4]
    out = retrofit_table(W, row_ptr, col, iterations=1, alpha=3.0, beta=np.array([2.0, 0.5, 1.0]), schedule="jacobi",
                         backend=ref.NumpyBackend())
    np.testing.assert_allclose(out["Y"][0], [0.95, 0.4], rtol=1e-15)


@pytest.mark.parametrize("schedule", retrofit.SCHEDULES)
def test_both_schedules_reach_the_solution_of_the_linear_system(schedule):
    """The fixed point: (t_i + w_i) q_i - sum_j beta_ij q_j = t_i q^_i, t_i = alpha w_i, for the rows with neighbours; the
    others stay.  alpha = 1: the iteration matrix has norm 1 / 2, so 200 sweeps are far beyond float64's precision."""
    rng = np.random.default_rng(5)
    n, d = 30, 4
    row_ptr, col = random_digraph(rng, n)
    beta = rng.uniform(0.5, 2.0, len(col))
    W = rng.standard_normal((n, d))
    B = np.zeros((n, n))
    for i in range(n):
        for p in range(row_ptr[i], row_ptr[i + 1]):
            B[i, col[p]] += beta[p]
    w = B.sum(axis=1)
    A, rhs = np.diag(2 * w) - B, w[:, None] * W
    fixed = w == 0
    A[fixed] = np.eye(n)[fixed]
    rhs[fixed] = W[fixed]
    want = np.linalg.solve(A, rhs)
    out = retrofit_table(W, row_ptr, col, iterations=200, alpha=1.0, beta=beta, schedule=schedule, backend=ref.NumpyBackend())
    assert np.abs(out["Y"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(out["Y"][fixed], W[fixed]) and fixed.sum() >= 3        # rows without neighbours: bit for bit


def test_a_row_without_neighbours_in_the_vocabulary_comes_back_bit_for_bit(tmp_path):
    vocab = ["a", "b", "c", "d"]
    row_ptr, col, counts = read_lexicon(write(tmp_path, "a b\nb a c\nc zebra\nyak d\n"), vocab)
    W = np.random.default_rng(0).standard_normal((4, 6)).astype(F32)
    for schedule in retrofit.SCHEDULES:
        out = retrofit_table(W, row_ptr, col, iterations=4, schedule=schedule, backend=ref.NumpyBackend(float32=True))
        assert np.array_equal(ref.bits(out["Y"][2:]), ref.bits(W[2:])) and out["rows_updated"] == 2
        assert not np.array_equal(out["Y"][:2], W[:2])


def test_driver_refusals():
    W = np.ones((3, 4), F32)
    row_ptr, col = np.array([0, 1, 1, 1], np.int64), np.array([2], np.int32)
    be = ref.NumpyBackend(float32=True)
    for settings in (dict(iterations=0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(schedule="random"),
                     dict(beta=np.ones(2, F32))):
        with pytest.raises(ValueError):
            retrofit_table(W, row_ptr, col, backend=be, **settings)
    with pytest.raises(ValueError, match="nothing to retrofit"):
        retrofit_table(W, np.zeros(4, np.int64), np.zeros(0, np.int32), backend=be)
    with pytest.raises(ValueError, match="table"):
        retrofit_table(np.ones(4, F32), row_ptr, col, backend=be)


# ---- 6. the command line
@pytest.fixture(scope="module")
def source_job(tmp_path_factory):
    """A job directory of trainer.svd's on the golden table, the way tests/test_postprocess.py builds one."""
    import svd_ref
    from trainer import svd
    job = tmp_path_factory.mktemp("retro") / "job"
    argv = ["--train-csv", str(GOLDEN / "text8_cov100_ctx2_interaction.csv"), "--vocab-txt", str(GOLDEN / "text8_cov100_ctx2_vocab.txt"),
            "--job-dir", str(job), "--embedding-size", "8", "--optimizer", "Adagrad"]
    return job, svd.main(argv, backend=svd_ref.NumpyBackend(float32=True))


def lexicon_for(vocab, tmp_path, upper=False):
    words = [w for w in vocab if w != "<UNK>"]
    lines = ["%s %s %s notaword" % (words[0], words[1], words[2]), "%s %s" % (words[1], words[0]),
             "%s %s %s" % (words[5], words[6], words[0]), "notakey %s" % words[3]]
    p = tmp_path / "lexicon.txt"
    p.write_text("\n".join(l.upper() if upper else l for l in lines) + "\n")
    return p, words


def run(argv):
    return retrofit.main(argv, backend=ref.NumpyBackend(float32=True))


def test_command_line_writes_an_ordinary_job_dir(source_job, tmp_path):
    from test_analogy import RefBackend
    from trainer.data_utils import read_vocab
    from trainer.estimator import Estimator
    from trainer.train_utils import CheckpointManager
    job, svd_out = source_job
    vocab = read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))
    lexicon, words = lexicon_for(vocab, tmp_path, upper=True)                    # (folded back by default)
    P = tmp_path / "P"
    out = run(["--job-dir", str(job), "--lexicon", str(lexicon), "--output-dir", str(P), "--optimizer", "Adagrad"])
    V = svd_out["R"].shape[0]
    row_ptr, col, counts = read_lexicon(lexicon, vocab)
    want = retrofit_table(svd_out["R"], row_ptr, col, backend=ref.NumpyBackend(float32=True))
    assert out["Y"].shape == (V, 8) and np.array_equal(ref.bits(out["Y"]), ref.bits(want["Y"]))
    assert {"params.json", "vocab.txt", "model.ckpt-0.pt", "retrofit.json"} <= {p.name for p in P.iterdir()}
    assert Path(CheckpointManager(str(P)).latest()).name == "model.ckpt-0.pt"
    t = torch.load(CheckpointManager(str(P)).latest(), map_location="cpu", weights_only=False)["tables"]
    assert (t["V"], t["d"], int(t["global_step"]), t["optimizer"]) == (V, 8, 0, "Adagrad")
    assert np.array_equal(t["R"].numpy(), out["Y"]) and not t["C"].any() and not t["br"].any() and not t["bc"].any()
    params = json.loads((P / "params.json").read_text())
    assert params["embedding_size"] == 8 and params["job_dir"] == str(P) and Path(params["vocab_txt"]) == P / "vocab.txt"
    assert read_vocab(params["vocab_txt"]) == vocab
    rec = json.loads((P / "retrofit.json").read_text())
    assert rec["source_job_dir"] == str(job) and rec["source_step"] == 0 and rec["embeddings"] == "row"
    assert (rec["iterations"], rec["alpha"], rec["schedule"], rec["lowercase"], rec["restrict_vocab"]) == (10, 1.0, "sequential", True, None)
    assert rec["lexicon"] == str(lexicon) and rec["optimizer"] == "Adagrad" and (rec["vocab_size"], rec["embedding_size"]) == (V, 8)
    assert rec["lexicon_counts"] == counts == dict(lines=4, keys_in_vocab=3, keys_out_of_vocab=1, neighbours_kept=5,
                                                   neighbours_out_of_vocab=1, duplicate_neighbours=0, rows=3)
    assert (rec["levels"], rec["largest_level"], rec["longest_row"], rec["rows_updated"]) == (
        want["levels"], want["largest_level"], 2, 3)
    assert rec["shift_mean"] == want["shift_mean"] > 0 and rec["shift_max"] == want["shift_max"] >= rec["shift_mean"]
    assert {"load", "read_lexicon", "schedule", "upload", "sweeps", "download", "write_job_dir"} <= set(rec["seconds"])
    e = Estimator(params, backend=RefBackend(), device="cpu")
    assert e.vocab_size == V and e.model.tables.global_step == 0
    assert np.array_equal(e._evaluation_table("row", None).numpy()[:, :8], out["Y"])
    # only the lexicon's keys moved
    moved = np.flatnonzero((out["Y"] != svd_out["R"]).any(axis=1))
    assert moved.tolist() == sorted(vocab.index(words[i]) for i in (0, 1, 5))


def test_command_line_options(source_job, tmp_path):
    from trainer.data_utils import read_vocab
    job, svd_out = source_job
    vocab = read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))
    lexicon, words = lexicon_for(vocab, tmp_path)
    P = tmp_path / "P"
    out = run(["--job-dir", str(job), "--lexicon", str(lexicon), "--output-dir", str(P), "--embeddings", "sum", "--iterations", "3",
               "--alpha", "0.5", "--schedule", "jacobi", "--restrict-vocab", "60", "--no-lowercase", "--optimizer", "Adam"])
    row_ptr, col, counts = read_lexicon(lexicon, vocab[:60], lowercase=False)
    want = retrofit_table((svd_out["R"] + svd_out["C"])[:60], row_ptr, col, iterations=3, alpha=0.5, schedule="jacobi",
                          backend=ref.NumpyBackend(float32=True))
    assert out["Y"].shape == (60, 8) and np.array_equal(ref.bits(out["Y"]), ref.bits(want["Y"]))
    rec = json.loads((P / "retrofit.json").read_text())
    assert (rec["iterations"], rec["alpha"], rec["schedule"], rec["lowercase"], rec["restrict_vocab"], rec["embeddings"]) == (
        3, 0.5, "jacobi", False, 60, "sum")
    assert rec["lexicon_counts"] == counts and rec["optimizer"] == "Adam"
    assert read_vocab(json.loads((P / "params.json").read_text())["vocab_txt"]) == vocab[:60]


@pytest.mark.parametrize("extra", [["--iterations", "0"], ["--alpha", "-1"], "same", "empty"])
def test_command_line_refuses_before_any_directory_is_made(source_job, tmp_path, extra):
    from trainer.data_utils import read_vocab
    job, _ = source_job
    P = tmp_path / "P"
    lexicon, _ = lexicon_for(read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt")), tmp_path)
    if extra == "empty":
        lexicon.write_text("notakey notaword\n\n")
    before = sorted(p.name for p in job.iterdir())
    with pytest.raises(ValueError):
        run(["--job-dir", str(job), "--lexicon", str(lexicon), "--output-dir", str(job if extra == "same" else P)]
            + (extra if isinstance(extra, list) else []))
    assert not P.exists() and sorted(p.name for p in job.iterdir()) == before
