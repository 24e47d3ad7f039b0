"""Word-similarity evaluation without a GPU: the pairs-file format and the statistics of trainer.wordsim, and
Estimator.evaluate_word_pairs through a test-only backend whose pair_cosine is the float64 reference."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import cosmul_ref
import wordsim_ref
from test_analogy import GRID, VOCAB, grid_table


class RefBackend:
    """pair_cosine by the float64 reference; remembers the table and the pairs it was handed."""

    def pair_cosine(self, W, pairs):
        self.W, self.pairs = W.clone(), pairs.clone()
        assert pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2
        return torch.from_numpy(cosmul_ref.pair_cosine(W.numpy(), pairs.numpy()).astype(np.float32))


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


# ids: 0 <UNK>, 1 .. 16 the grid words w00 .. w33, 17 Berlin, 18 .. 21 x0 .. x3
PAIRS = """# WordSim-style: a comment, then a header
Word 1\tWord 2\tHuman (mean)
w00\tw01\t7.5
W00\tw11\t2.25

w00\tmissing\t9
# a comment in the middle
<UNK>\tw01\t1
w12\tw13\t6.5
Berlin\tw00\t3
x0\tx1\t5.0
w22 w33 1.5
"""


def write_pairs(tmp_path, text=PAIRS, name="pairs.tab"):
    path = tmp_path / name
    path.write_text(text)
    return path


# ---- the file format
def test_parser_skips_comments_blank_lines_and_one_header(tmp_path):
    from trainer import wordsim
    rows = wordsim.parse_pairs(write_pairs(tmp_path))
    assert [r[0] for r in rows] == [3, 4, 6, 8, 9, 10, 11, 12]          # line numbers
    assert rows[1][1:] == ("w00", "w11", 2.25) and rows[5][1:] == ("berlin", "w00", 3.0)
    assert [r[1:] for r in rows] == wordsim_ref.parse(write_pairs(tmp_path))
    rows = wordsim.parse_pairs(write_pairs(tmp_path), lowercase=False)
    assert rows[1][1] == "W00" and rows[5][1] == "Berlin"
    # no header: the first line is a pair
    assert len(wordsim.parse_pairs(write_pairs(tmp_path, "a b 1\nc d 2\n"))) == 2
    # only ONE header line
    with pytest.raises(ValueError, match="line 2"):
        wordsim.parse_pairs(write_pairs(tmp_path, "w1 w2 score\nw1 w2 score\na b 1\n"))
    assert wordsim.parse_pairs(write_pairs(tmp_path, "")) == [] and wordsim.parse_pairs(write_pairs(tmp_path, "# x\n\nw1 w2 sim\n")) == []


def test_delimiter_and_score_column(tmp_path):
    from trainer import wordsim
    simlex = "word1\tword2\tPOS\tSimLex999\tconc\nold\tnew\tA\t1.58\t2.7\nsmart\tintelligent\tA\t9.2\t1.75\n"
    rows = wordsim.parse_pairs(write_pairs(tmp_path, simlex), score_column=4)
    assert [r[1:] for r in rows] == [("old", "new", 1.58), ("smart", "intelligent", 9.2)]
    assert [r[1:] for r in rows] == wordsim_ref.parse(write_pairs(tmp_path, simlex), score_column=4)
    csv = "a,b,score\nnew york,city,3.5\nx , y ,1\n"
    rows = wordsim.parse_pairs(write_pairs(tmp_path, csv), delimiter=",")
    assert [r[1:] for r in rows] == [("new york", "city", 3.5), ("x", "y", 1.0)]       # a delimiter keeps inner blanks
    assert [r[1:] for r in rows] == wordsim_ref.parse(write_pairs(tmp_path, csv), delimiter=",")
    with pytest.raises(ValueError, match="score-column"):
        wordsim.parse_pairs(write_pairs(tmp_path, csv), score_column=2)


def test_malformed_line_names_its_line(tmp_path):
    from trainer import wordsim
    with pytest.raises(ValueError, match="line 4"):
        wordsim.parse_pairs(write_pairs(tmp_path, "w1 w2 score\na b 1\n\nc d\n"))
    with pytest.raises(ValueError, match="line 3"):
        wordsim.parse_pairs(write_pairs(tmp_path, "a b 1\n# c\nc d high\n"))
    with pytest.raises(ValueError, match="line 2"):
        wordsim.parse_pairs(write_pairs(tmp_path, "a b 1\nc d nan\n"))
    with pytest.raises(ValueError, match="line 3"):
        wordsim.parse_pairs(write_pairs(tmp_path, "h1\th2\th3\th4\na\tb\tN\t1\nc\td\t2\n"), score_column=4)


def test_lookup_counts_what_it_skips(tmp_path):
    from trainer import wordsim
    rows = wordsim.parse_pairs(write_pairs(tmp_path))
    ids, human, skipped = wordsim.lookup_pairs(rows, VOCAB)
    # "missing" and <UNK> are skipped, and "berlin": the vocabulary holds "Berlin" only
    assert ids == [(1, 2), (1, 6), (7, 8), (18, 19), (11, 16)] and human == [7.5, 2.25, 6.5, 5.0, 1.5] and skipped == 3
    ids, human, skipped = wordsim.lookup_pairs(wordsim.parse_pairs(write_pairs(tmp_path), lowercase=False), VOCAB)
    assert ids == [(1, 2), (7, 8), (17, 1), (18, 19), (11, 16)] and skipped == 3          # W00 is no word as written, Berlin is
    ids, human, skipped = wordsim.lookup_pairs(rows, VOCAB, limit=16)
    assert ids == [(1, 2), (1, 6), (7, 8)] and skipped == 5                                # w33 has id 16, x0 / x1 ids >= 18


# ---- the statistics
def test_spearman_on_hand_computed_cases():
    from trainer import wordsim
    assert wordsim.spearman([1, 2, 3, 4, 5], [10, 20, 30, 40, 50]) == pytest.approx(1.0, abs=1e-15)
    assert wordsim.spearman([1, 2, 3, 4, 5], [5, 4, 3, 2, 1]) == pytest.approx(-1.0, abs=1e-15)
    assert wordsim.spearman([0.1, 0.5, 0.2], [1, 100, 10]) == pytest.approx(1.0, abs=1e-15)       # monotone, not linear
    assert wordsim.pearson([0.1, 0.5, 0.2], [1, 100, 10]) < 0.99
    # ties: x = 1 2 2 4 has ranks 1 2.5 2.5 4; y = 1 3 2 2 has ranks 1 4 2.5 2.5; both means 2.5
    # deviations -1.5 0 0 1.5 and -1.5 1.5 0 0: covariance sum 2.25, both sums of squares 4.5 -> rho = 2.25 / 4.5
    assert wordsim.average_ranks([1, 2, 2, 4]).tolist() == [1, 2.5, 2.5, 4]
    assert wordsim.average_ranks([1, 3, 2, 2]).tolist() == [1, 4, 2.5, 2.5]
    assert wordsim.average_ranks([7, 7, 7]).tolist() == [2, 2, 2] and wordsim.average_ranks([]).tolist() == []
    assert wordsim.spearman([1, 2, 2, 4], [1, 3, 2, 2]) == pytest.approx(0.5, abs=1e-15)
    # no ties, n = 4, d = rank differences 1 -1 1 -1: rho = 1 - 6 sum d^2 / (n (n^2 - 1)) = 1 - 24 / 60
    assert wordsim.spearman([1, 2, 3, 4], [2, 1, 4, 3]) == pytest.approx(0.6, abs=1e-15)
    # Pearson by hand: x = 1 2 3, y = 1 2 4: dx = -1 0 1, dy = -4/3 -1/3 5/3, sxy = 3, sxx = 2, syy = 42/9
    assert wordsim.pearson([1, 2, 3], [1, 2, 4]) == pytest.approx(3 / np.sqrt(2 * 42 / 9), abs=1e-15)


def test_statistics_are_none_where_they_do_not_exist():
    from trainer import wordsim
    for f in (wordsim.spearman, wordsim.pearson):
        assert f([], []) is None and f([1.0], [2.0]) is None
        assert f([1, 2, 3], [4, 4, 4]) is None and f([5, 5, 5], [1, 2, 3]) is None
        assert f([1, 2], [2, 1]) == pytest.approx(-1.0)
        with pytest.raises(ValueError):
            f([1, 2], [1])


def test_statistics_against_the_reference_and_scipy():
    from trainer import wordsim
    rng = np.random.default_rng(21)
    for n in (2, 3, 10, 200):
        x = rng.integers(0, 8, n).astype(float) if n > 3 else rng.standard_normal(n)      # many ties
        y = rng.standard_normal(n) + x
        assert wordsim.spearman(x, y) == pytest.approx(wordsim_ref.spearman(x.tolist(), y.tolist()), abs=1e-13)
        assert wordsim.pearson(x, y) == pytest.approx(wordsim_ref.pearson(x.tolist(), y.tolist()), abs=1e-13)
        assert wordsim.average_ranks(x).tolist() == wordsim_ref.ranks(x.tolist())
    try:
        from scipy import stats
    except ImportError:
        return                                               # (only this cross-check is left out without scipy)
    x = rng.integers(0, 8, 200).astype(float)
    y = rng.standard_normal(200) + x
    assert wordsim.spearman(x, y) == pytest.approx(stats.spearmanr(x, y)[0], abs=1e-12)
    assert wordsim.pearson(x, y) == pytest.approx(stats.pearsonr(x, y)[0], abs=1e-12)


# ---- the Estimator through a reference backend
def test_record_and_json(est, tmp_path):
    p = write_pairs(tmp_path)
    rec = est.evaluate_word_pairs(str(p))
    assert set(rec) == {"global_step", "embeddings", "pairs_file", "pairs_total", "pairs_seen", "skipped", "spearman", "pearson"}
    assert (rec["pairs_file"], rec["pairs_total"], rec["pairs_seen"], rec["skipped"]) == ("pairs.tab", 8, 5, 3)
    assert rec["embeddings"] == "row" and rec["global_step"] == 0
    assert est.backend.pairs.tolist() == [[1, 2], [1, 6], [7, 8], [18, 19], [11, 16]]
    want = wordsim_ref.score_file(str(p), VOCAB, est.model.tables.R.numpy())
    for key in rec:
        assert rec[key] == (pytest.approx(want[key], abs=1e-6) if key in ("spearman", "pearson") else want[key]), key
    assert -1 <= rec["pearson"] <= 1 and rec["spearman"] is not None
    assert json.loads((Path(est.params["job_dir"]) / "eval" / "wordsim.json").read_text()) == rec


@pytest.mark.parametrize("which", ["row", "col", "sum"])
def test_options_reach_the_table_and_the_lookup(est, tmp_path, which):
    p = write_pairs(tmp_path)
    t = est.model.tables
    table = {"row": t.R, "col": t.C, "sum": t.R + t.C}[which]
    rec = est.evaluate_word_pairs(str(p), embeddings=which, restrict_vocab=18, lowercase=False)
    assert torch.equal(est.backend.W, table[:18]) and rec["embeddings"] == which
    assert (rec["pairs_seen"], rec["skipped"]) == (4, 4)
    want = wordsim_ref.score_file(str(p), VOCAB, table.numpy(), restrict=18, lowercase=False, embeddings=which)
    assert rec["spearman"] == pytest.approx(want["spearman"], abs=1e-6) and rec["pearson"] == pytest.approx(want["pearson"], abs=1e-6)
    with pytest.raises(ValueError, match="embeddings"):
        est.evaluate_word_pairs(str(p), embeddings="both")
    with pytest.raises(ValueError, match="restrict-vocab"):
        est.evaluate_word_pairs(str(p), restrict_vocab=len(VOCAB) + 1)


def test_too_few_pairs_give_none(est, tmp_path):
    rec = est.evaluate_word_pairs(str(write_pairs(tmp_path, "w00 w01 3\nnope w01 4\n")))
    assert (rec["pairs_total"], rec["pairs_seen"], rec["skipped"], rec["spearman"], rec["pearson"]) == (2, 1, 1, None, None)
    rec = est.evaluate_word_pairs(str(write_pairs(tmp_path, "# nothing\n")))
    assert (rec["pairs_total"], rec["pairs_seen"], rec["spearman"]) == (0, 0, None)
    rec = est.evaluate_word_pairs(str(write_pairs(tmp_path, "w00 w01 3\nw02 w13 3\nw11 w30 3\n")))      # a constant column
    assert rec["pairs_seen"] == 3 and rec["spearman"] is None and rec["pearson"] is None


def test_main_only_parses_arguments(est, monkeypatch):
    """`python -m trainer.wordsim`'s main() hands its flags to Estimator.evaluate_word_pairs of the job's params."""
    from trainer import estimator, wordsim
    seen = {}

    class Fake:
        def __init__(self, params):
            seen["params"] = params

        def evaluate_word_pairs(self, pairs, **options):
            seen.update(pairs=pairs, **options)
            return "rec"
    monkeypatch.setattr(estimator, "Estimator", Fake)
    job = est.params["job_dir"]
    assert wordsim.main(job_dir=job, pairs="p.tab", embeddings="sum", restrict_vocab=9, no_lowercase=True, delimiter=",",
                        score_column=4) == "rec"
    assert seen["params"]["job_dir"] == job and seen["pairs"] == "p.tab"
    assert {k: seen[k] for k in ("embeddings", "restrict_vocab", "lowercase", "delimiter", "score_column")} == \
        {"embeddings": "sum", "restrict_vocab": 9, "lowercase": False, "delimiter": ",", "score_column": 4}
    wordsim.main(job_dir=job, pairs="p.tab")
    assert {k: seen[k] for k in ("embeddings", "restrict_vocab", "lowercase", "delimiter", "score_column")} == \
        {"embeddings": "row", "restrict_vocab": None, "lowercase": True, "delimiter": None, "score_column": 3}
