"""Spherical k-means without a GPU: the surface of libglove_eval_hip.so's third header
(include/glove_eval_cluster_hip.h), its workspace query and host-side argument checks (they happen before any launch),
the gold-file bookkeeping of trainer.categorize, Estimator.evaluate_categorization / word_classes through a test-only
backend whose kmeans is the float64 reference of tests/kmeans_ref.py, and that reference's own sanity."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import kmeans_ref
from test_analogy import BADARG, FAKE, GRID, VOCAB, WORKSPACE, declared_functions, grid_table

REPO = Path(__file__).resolve().parent.parent
HEADERS = {name: REPO / "include" / name for name in ("glove_hip.h", "glove_eval_hip.h", "glove_eval_sim_hip.h",
                                                      "glove_eval_cluster_hip.h")}
N_MAX = 65535 * 128


@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.EVAL_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_eval_library()


# ---- library surface
def test_cluster_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADERS["glove_eval_cluster_hip.h"])
    assert set(names) == set(hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS) and len(names) == len(hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS) == 4
    for n in names:
        assert hasattr(lib, n), n
    others = set(hip_api.EXPORTED_SYMBOLS) | set(hip_api.EVAL_EXPORTED_SYMBOLS) | set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS)
    assert not set(names) & others
    train = hip_api.load_library()
    for n in names:
        assert not hasattr(train, n), n                      # the new object is no part of libglove_hip.so
    assert lib.glove_eval_cluster_abi_version() == hip_api.GLOVE_EVAL_CLUSTER_ABI_VERSION == 1
    assert "GLOVE_EVAL_CLUSTER_ABI_VERSION 1" in HEADERS["glove_eval_cluster_hip.h"].read_text()


def test_the_other_headers_keep_their_versions(lib):
    from trainer import hip_api
    assert "#define GLOVE_ABI_VERSION 15" in HEADERS["glove_hip.h"].read_text() and hip_api.GLOVE_ABI_VERSION == 15
    assert "GLOVE_EVAL_ABI_VERSION 1" in HEADERS["glove_eval_hip.h"].read_text() and lib.glove_eval_abi_version() == 1
    assert "GLOVE_EVAL_SIM_ABI_VERSION 1" in HEADERS["glove_eval_sim_hip.h"].read_text() and lib.glove_eval_sim_abi_version() == 1
    assert set(declared_functions(HEADERS["glove_eval_hip.h"])) == set(hip_api.EVAL_EXPORTED_SYMBOLS)
    assert set(declared_functions(HEADERS["glove_eval_sim_hip.h"])) == set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS)
    assert len(declared_functions(HEADERS["glove_hip.h"])) == 42


def layout(n, d, K):
    """The header's: pinv[n] | cinv[K] | hist[T K] | starts[5 (K + 1)] | sorted[n] | sums_a[R1 d] | sums_b[R2 d]."""
    up = lambda words: (4 * words + 255) // 256 * 256
    T, R1 = (n + 2047) // 2048, n // 64 + K
    R2 = R1 // 64 + K
    return up(n) + up(K) + up(T * K) + up(5 * (K + 1)) + up(n) + up(R1 * d) + up(R2 * d)


def test_workspace_query_is_the_stated_layout(lib):
    ws = lib.glove_kmeans_workspace_bytes
    for n, V, d, K in ((5000, 5000, 64, 40), (0, 10, 8, 1), (1, 1, 4, 1), (2049, 3000, 300, 1000), (400000, 400000, 320, 4096),
                       (N_MAX, 5, 1024, 4096), (777, 1000, 52, 33)):
        assert ws(n, V, d, K) == layout(n, d, K), (n, V, d, K)
    base = ws(5000, 5000, 64, 40)
    assert ws(5064, 5000, 64, 40) > base and ws(5000, 5000, 68, 40) > base and ws(5000, 5000, 64, 41) > base
    assert ws(5000, 9000, 64, 40) == base                    # V does not enter it
    assert ws(0, 5000, 64, 40) > 0


@pytest.mark.parametrize("bad", [(-1, 5000, 64, 40), (N_MAX + 1, 5000, 64, 40), (100, 0, 64, 40), (100, -3, 64, 40),
                                 (100, 5000, 0, 40), (100, 5000, 62, 40), (100, 5000, 1028, 40), (100, 5000, 64, 0),
                                 (100, 5000, 64, 4097)])
def test_every_bad_size_is_refused(lib, bad):
    n, V, d, K = bad
    assert lib.glove_kmeans_workspace_bytes(*bad) == 0
    assert lib.glove_kmeans_assign_f32(FAKE, V, d, FAKE, n, FAKE, K, FAKE, FAKE, FAKE, 1 << 40, None) == BADARG
    assert lib.glove_kmeans_update_f32(FAKE, V, d, FAKE, n, FAKE, FAKE, K, FAKE + 64, FAKE, FAKE, 1 << 40, None) == BADARG


def assign_call(lib, V=100, d=8, n=4, K=5, W=FAKE, ids=FAKE, C=FAKE, assign=FAKE, cos=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.glove_kmeans_workspace_bytes(max(n, 0), V, d, K)
    return lib.glove_kmeans_assign_f32(W, V, d, ids, n, C, K, assign, cos, ws, ws_bytes, None)


def update_call(lib, V=100, d=8, n=4, K=5, W=FAKE, ids=FAKE, assign=FAKE, C_in=FAKE, C_out=2 * FAKE, counts=FAKE, ws=FAKE,
                ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.glove_kmeans_workspace_bytes(max(n, 0), V, d, K)
    return lib.glove_kmeans_update_f32(W, V, d, ids, n, assign, C_in, K, C_out, counts, ws, ws_bytes, None)


def test_argument_errors_are_reported_on_the_host(lib):
    for name in ("W", "ids", "C", "assign", "cos", "ws"):
        assert assign_call(lib, **{name: None}) == BADARG, name
    for name in ("W", "ids", "assign", "C_in", "C_out", "counts", "ws"):
        assert update_call(lib, **{name: None}) == BADARG, name
    assert update_call(lib, C_out=FAKE) == BADARG                        # C_out == C_in
    need = lib.glove_kmeans_workspace_bytes(4, 100, 8, 5)
    assert assign_call(lib, ws_bytes=need - 1) == WORKSPACE and update_call(lib, ws_bytes=need - 1) == WORKSPACE
    assert assign_call(lib, n=0) == 0 and update_call(lib, n=0) == 0    # nothing to do: no launch
    assert assign_call(lib, n=0, ids=None, assign=None, cos=None, ws=None, ws_bytes=0) == 0
    assert update_call(lib, n=0, K=0) == BADARG and assign_call(lib, n=0, d=10, ws_bytes=1 << 30) == BADARG    # sizes come first


# ---- the gold file: parser, lookup, purity
CATEGORIES = """# AP-style: word category
w00 fruit
W01 fruit

w10 tool
missing tool
# a comment in the middle
<UNK> tool
w00 tool
Berlin city
x0 city
x1\tcity
w11 tool
"""


def write_categories(tmp_path, text=CATEGORIES, name="categories.txt"):
    path = tmp_path / name
    path.write_text(text)
    return path


def test_parser_skips_comments_and_blank_lines(tmp_path):
    from trainer import categorize
    rows = categorize.parse_categories(write_categories(tmp_path))
    assert [r[0] for r in rows] == [2, 3, 5, 6, 8, 9, 10, 11, 12, 13]    # line numbers
    assert rows[1][1:] == ("w01", "fruit") and rows[6][1:] == ("berlin", "city")
    assert [r[1:] for r in rows] == kmeans_ref.parse(write_categories(tmp_path))
    rows = categorize.parse_categories(write_categories(tmp_path), lowercase=False)
    assert rows[1][1] == "W01" and rows[6][1] == "Berlin"
    assert categorize.parse_categories(write_categories(tmp_path, "# x\n\n")) == []
    with pytest.raises(ValueError, match="line 3"):
        categorize.parse_categories(write_categories(tmp_path, "a fruit\n# c\nb\n"))


def test_column_options(tmp_path):
    from trainer import categorize
    bless = "fruit,apple,0.5\ntool,New Hammer ,1\n"
    rows = categorize.parse_categories(write_categories(tmp_path, bless), delimiter=",", word_column=2, category_column=1)
    assert [r[1:] for r in rows] == [("apple", "fruit"), ("new hammer", "tool")]         # a delimiter keeps inner blanks
    assert [r[1:] for r in rows] == kmeans_ref.parse(write_categories(tmp_path, bless), delimiter=",", word_column=2, category_column=1)
    rows = categorize.parse_categories(write_categories(tmp_path, "a x fruit\nb y tool\n"), category_column=3)
    assert [r[1:] for r in rows] == [("a", "fruit"), ("b", "tool")]
    with pytest.raises(ValueError, match="line 2"):
        categorize.parse_categories(write_categories(tmp_path, "a x fruit\nb y\n"), category_column=3)
    for wc, cc in ((1, 1), (0, 2), (2, 0)):
        with pytest.raises(ValueError, match="column"):
            categorize.parse_categories(write_categories(tmp_path, bless), word_column=wc, category_column=cc)


def test_lookup_counts_what_it_skips_and_the_duplicates(tmp_path):
    from trainer import categorize
    rows = categorize.parse_categories(write_categories(tmp_path))
    # "missing", <UNK> and "berlin" (the vocabulary holds "Berlin") are skipped; the second w00 is a duplicate
    assert categorize.lookup_words(rows, VOCAB) == ([1, 2, 5, 18, 19, 6], ["fruit", "fruit", "tool", "city", "city", "tool"], 3, 1)
    assert categorize.lookup_words(rows, VOCAB) == kmeans_ref.lookup(kmeans_ref.parse(write_categories(tmp_path)), VOCAB)
    rows = categorize.parse_categories(write_categories(tmp_path), lowercase=False)
    ids, gold, skipped, duplicates = categorize.lookup_words(rows, VOCAB)
    assert ids == [1, 5, 17, 18, 19, 6] and (skipped, duplicates) == (3, 1)              # W01 is no word as written, Berlin is
    ids, gold, skipped, duplicates = categorize.lookup_words(categorize.parse_categories(write_categories(tmp_path)), VOCAB, limit=18)
    assert ids == [1, 2, 5, 6] and gold == ["fruit", "fruit", "tool", "tool"] and (skipped, duplicates) == (5, 1)
    assert (ids, gold, skipped, duplicates) == kmeans_ref.lookup(kmeans_ref.parse(write_categories(tmp_path)), VOCAB, restrict=18)


def test_purity_on_hand_computed_cases():
    from trainer import categorize
    gold = ["a", "a", "a", "b", "b", "c"]
    for f in (categorize.purity, kmeans_ref.purity):
        assert f([0, 0, 0, 1, 1, 2], gold) == 1.0                                        # the gold partition
        assert f([5, 5, 5, 1, 1, 0], gold) == 1.0                                        # cluster names do not matter
        assert f([0, 0, 0, 0, 0, 0], gold) == 3 / 6                                      # one cluster: the largest category
        assert f([0, 1, 2, 3, 4, 5], gold) == 1.0                                        # all singletons
        assert f([0, 0, 1, 1, 2, 2], gold) == (2 + 1 + 1) / 6                            # ties inside a cluster: a b | b c
        assert f([0, 1, 0, 1, 0, 1], gold) == (2 + 1) / 6
        assert f(np.array([1, 1], np.int32), ["x", "y"]) == 0.5
        assert f([], []) is None
    with pytest.raises(ValueError):
        categorize.purity([0, 1], ["a"])
    rng = np.random.default_rng(3)
    for _ in range(20):
        a, g = rng.integers(0, 5, 40), [str(x) for x in rng.integers(0, 4, 40)]
        assert categorize.purity(a, g) == kmeans_ref.purity(a, g)


# ---- the Estimator through a reference backend
class RefBackend:
    """kmeans by the float64 reference; remembers what it was handed."""

    def kmeans(self, W, ids, K, seed=0, restarts=1, iterations=100, init=None):
        assert ids.dtype == torch.int32 and ids.dim() == 1 and init is None
        self.W, self.ids, self.options = W.clone(), ids.clone(), dict(K=K, seed=seed, restarts=restarts, iterations=iterations)
        res = kmeans_ref.kmeans(W.numpy(), ids.numpy(), K, seed, restarts, iterations)
        return SimpleNamespace(assign=torch.from_numpy(res.assign), cos=torch.from_numpy(res.cos.astype(np.float32)),
                               centroids=torch.from_numpy(res.centroids.astype(np.float32)), iterations=res.iterations,
                               converged=res.converged, objective=res.objective, objectives=res.objectives,
                               assignments=[torch.from_numpy(a) for a in res.assignments])


@pytest.fixture()
def est(tmp_path):
    from trainer.config_utils import parse_args
    from trainer.estimator import Estimator
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(VOCAB))
    params = parse_args(["--train-csv", str(tmp_path / "none.csv"), "--vocab-txt", str(vocab), "--job-dir", str(tmp_path / "job"),
                         "--disable-datetime-path", "--embedding-size", str(2 * GRID), "--optimizer", "Adagrad", "--seed", "1"])
    e = Estimator(params, backend=RefBackend(), device="cpu")
    e.model.tables.R = torch.from_numpy(grid_table(0))
    e.model.tables.C = torch.from_numpy(grid_table(1)[::-1].copy())
    return e


KEYS = {"global_step", "embeddings", "categories_file", "words_total", "words_seen", "skipped", "duplicates", "categories",
        "clusters", "restarts", "seed", "iterations", "converged", "objective", "purity", "purity_mean", "purity_min",
        "purity_max", "sizes"}


def test_categorization_record_and_json(est, tmp_path):
    p = write_categories(tmp_path)
    rec = est.evaluate_categorization(str(p), restarts=4, seed=2)
    assert set(rec) == KEYS
    assert (rec["categories_file"], rec["words_total"], rec["words_seen"], rec["skipped"], rec["duplicates"]) == \
        ("categories.txt", 10, 6, 3, 1)
    assert (rec["categories"], rec["clusters"], rec["restarts"], rec["seed"], rec["embeddings"], rec["global_step"]) == \
        (3, 3, 4, 2, "row", 0)
    assert est.backend.ids.tolist() == [1, 2, 5, 18, 19, 6] and est.backend.options == dict(K=3, seed=2, restarts=4, iterations=100)
    assert rec == kmeans_ref.score_file(str(p), VOCAB, est.model.tables.R.numpy(), restarts=4, seed=2)
    assert rec["purity_min"] <= rec["purity_mean"] <= rec["purity_max"] and rec["purity_min"] <= rec["purity"] <= rec["purity_max"]
    assert sum(rec["sizes"]) == 6 and len(rec["sizes"]) == 3 and 1 / 3 < rec["purity"] <= 1.0
    assert json.loads((Path(est.params["job_dir"]) / "eval" / "categorization.json").read_text()) == rec


@pytest.mark.parametrize("which", ["row", "col", "sum"])
def test_categorization_options_reach_the_table_and_the_lookup(est, tmp_path, which):
    p = write_categories(tmp_path)
    t = est.model.tables
    table = {"row": t.R, "col": t.C, "sum": t.R + t.C}[which]
    rec = est.evaluate_categorization(str(p), embeddings=which, restrict_vocab=18, lowercase=False, clusters=3, restarts=2,
                                      iterations=7)
    assert torch.equal(est.backend.W, table[:18]) and rec["embeddings"] == which
    assert est.backend.ids.tolist() == [1, 5, 17, 6] and est.backend.options == dict(K=3, seed=0, restarts=2, iterations=7)
    assert (rec["words_seen"], rec["skipped"], rec["duplicates"], rec["categories"], rec["clusters"]) == (4, 5, 1, 3, 3)
    assert rec == kmeans_ref.score_file(str(p), VOCAB, table.numpy(), restrict=18, lowercase=False, clusters=3, restarts=2,
                                        iterations=7, embeddings=which)
    with pytest.raises(ValueError, match="embeddings"):
        est.evaluate_categorization(str(p), embeddings="both")
    with pytest.raises(ValueError, match="restrict-vocab"):
        est.evaluate_categorization(str(p), restrict_vocab=len(VOCAB) + 1)
    with pytest.raises(ValueError, match="clusters"):
        est.evaluate_categorization(str(p), clusters=7)                  # six words kept
    with pytest.raises(ValueError, match="clusters"):
        est.evaluate_categorization(str(write_categories(tmp_path, "# nothing\n")))
    with pytest.raises(ValueError, match="restarts"):
        est.evaluate_categorization(str(p), restarts=0)


def test_word_classes_files(est):
    rec = est.word_classes(4, iterations=5, restarts=2, seed=3)
    assert set(rec) == {"global_step", "embeddings", "words", "classes", "iterations", "converged", "objective", "empty",
                        "largest", "smallest"}
    job = Path(est.params["job_dir"])
    lines = (job / "classes.txt").read_text().split("\n")
    assert lines[-1] == "" and [x.split(" ")[0] for x in lines[:-1]] == VOCAB[1:]        # vocabulary order, <UNK> left out
    want_lines, want = kmeans_ref.classes_file(VOCAB, est.model.tables.R.numpy(), 4, iterations=5, restarts=2, seed=3)
    assert lines[:-1] == want_lines and rec == want
    assert est.backend.ids.tolist() == list(range(1, len(VOCAB))) and est.backend.options == dict(K=4, seed=3, restarts=2, iterations=5)
    assert (rec["words"], rec["classes"]) == (len(VOCAB) - 1, 4) and rec["smallest"] <= rec["largest"] and rec["iterations"] <= 5
    assert json.loads((job / "eval" / "classes.json").read_text()) == rec
    t = est.model.tables
    rec = est.word_classes(3, embeddings="sum", restrict_vocab=10)
    assert torch.equal(est.backend.W, (t.R + t.C)[:10]) and est.backend.ids.tolist() == list(range(1, 10)) and rec["words"] == 9
    assert (job / "classes.txt").read_text().split("\n")[:-1] == \
        kmeans_ref.classes_file(VOCAB, (t.R + t.C).numpy(), 3, restrict=10, embeddings="sum")[0]
    for bad in (0, None, len(VOCAB)):
        with pytest.raises(ValueError, match="classes"):
            est.word_classes(bad)


def test_mains_only_parse_arguments(est, monkeypatch):
    """main() of trainer.categorize and trainer.classes hand their flags to the Estimator of the job's params."""
    from trainer import categorize, classes, estimator
    seen = {}

    class Fake:
        def __init__(self, params):
            seen["params"] = params

        def evaluate_categorization(self, categories, **options):
            seen.update(categories=categories, **options)
            return "rec"

        def word_classes(self, k, **options):
            seen.update(k=k, **options)
            return "classes"
    monkeypatch.setattr(estimator, "Estimator", Fake)
    job = est.params["job_dir"]
    assert categorize.main(job_dir=job, categories="c.txt", embeddings="sum", restrict_vocab=9, no_lowercase=True, delimiter=",",
                           word_column=2, category_column=1, clusters=6, restarts=3, iterations=20, seed=5) == "rec"
    assert seen["params"]["job_dir"] == job and seen["categories"] == "c.txt"
    keys = ("embeddings", "restrict_vocab", "lowercase", "delimiter", "word_column", "category_column", "clusters", "restarts",
            "iterations", "seed")
    assert {k: seen[k] for k in keys} == dict(embeddings="sum", restrict_vocab=9, lowercase=False, delimiter=",", word_column=2,
                                              category_column=1, clusters=6, restarts=3, iterations=20, seed=5)
    categorize.main(job_dir=job, categories="c.txt")
    assert {k: seen[k] for k in keys} == dict(embeddings="row", restrict_vocab=None, lowercase=True, delimiter=None, word_column=1,
                                              category_column=2, clusters=None, restarts=10, iterations=100, seed=0)
    assert classes.main(job_dir=job, classes=8) == "classes"
    assert (seen["k"], seen["iterations"], seen["restarts"], seen["seed"], seen["embeddings"]) == (8, 10, 1, 0, "row")


# ---- the reference's own sanity
def test_reference_recovers_a_planted_partition():
    W, gold, init = kmeans_ref.planted()                     # 24 centres x 90 points, d = 64, noise 0.35, seed 77
    ids = np.arange(len(W), dtype=np.int32)
    res = kmeans_ref.kmeans(W, ids, 24, init=init)
    print("planted data: %d passes, minimum margin %.4f" % (res.iterations, res.min_margin))
    assert res.converged and res.iterations <= 3
    assert res.assign.tolist() == gold.tolist() and kmeans_ref.purity(res.assign, gold.tolist()) == 1.0
    # far from any tie (0.41 measured), so that the float32 kernels may be asked for the same partition exactly
    assert res.min_margin >= 0.1
    assert all(y >= x - 1e-9 for x, y in zip(res.trace, res.trace[1:]))
    # update: unit rows, the counts, an empty cluster keeps its row
    C = np.vstack([init, np.full((1, 64), 3.0, np.float32)])
    new, counts = kmeans_ref.update(W, ids, res.assign, C)
    assert counts.tolist() == [90] * 24 + [0] and np.array_equal(new[24], C[24])
    np.testing.assert_allclose(np.linalg.norm(new[:24], axis=1), 1.0, rtol=1e-12)
    # random restarts reach it too, and the winner is the arg-max of the objectives
    res = kmeans_ref.kmeans(W, ids, 24, seed=1, restarts=3)
    assert res.objective == max(res.objectives) and len(res.assignments) == 3
    a, cos, margin = kmeans_ref.assign(np.zeros((2, 4), np.float32), np.array([0, 1], np.int32), np.ones((3, 4), np.float32))
    assert a.tolist() == [0, 0] and cos.tolist() == [0.0, 0.0] and margin.tolist() == [0.0, 0.0]      # a zero row: cluster 0
