"""Word-analogy evaluation without a GPU: the surface of libglove_eval_hip.so (include/glove_eval_hip.h), its host-side
argument checks (they happen before any launch), and the question-file bookkeeping of trainer.analogy /
Estimator.evaluate_analogies through a test-only backend whose analogy_topk is the float64 reference."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import analogy_ref

REPO = Path(__file__).resolve().parent.parent
EVAL_HEADER = REPO / "include" / "glove_eval_hip.h"
TRAIN_HEADER = REPO / "include" / "glove_hip.h"
BADARG, WORKSPACE = -1, -2
FAKE = 0x10000              # a non-null "device pointer": the calls below return before anything would read it


def declared_functions(header):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(glove_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.EVAL_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_eval_library()


# ---- library surface
def test_eval_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(EVAL_HEADER)
    assert set(names) == set(hip_api.EVAL_EXPORTED_SYMBOLS) and len(names) <= 3
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_eval_abi_version() == hip_api.GLOVE_EVAL_ABI_VERSION == 1
    assert "GLOVE_EVAL_ABI_VERSION 1" in EVAL_HEADER.read_text()


def test_training_header_is_untouched():
    from trainer import hip_api
    names = declared_functions(TRAIN_HEADER)
    assert len(names) == 42 and set(names) == set(hip_api.EXPORTED_SYMBOLS)
    assert hip_api.GLOVE_ABI_VERSION == 15
    assert not set(names) & set(hip_api.EVAL_EXPORTED_SYMBOLS)      # the new object is no part of libglove_hip.so


def test_missing_eval_library_is_an_error_not_a_fallback(tmp_path):
    from trainer import hip_api
    with pytest.raises(hip_api.GloveHipError, match="no CPU fallback"):
        hip_api.load_eval_library(tmp_path / "libglove_eval_hip.so")


def test_workspace_query_is_a_pure_host_function(lib):
    ws = lib.glove_analogy_workspace_bytes
    base = ws(100, 5000, 64, 10)
    # inv_norm[V] | Q[n d] | q_inv[n] | sims[n V] | 2 x (values + ids of ceil(V / 4096) k winners per question), 256-B aligned
    up = lambda x: (x + 255) // 256 * 256
    assert base == up(5000 * 4) + up(100 * 64 * 4) + up(100 * 4) + up(100 * 5000 * 4) + 4 * up(100 * 2 * 10 * 4)
    assert ws(101, 5000, 64, 10) > base and ws(100, 5001, 64, 10) > base
    assert ws(100, 5000, 68, 10) > base and ws(100, 5000, 64, 11) > base
    assert ws(0, 5000, 64, 10) > 0
    for bad in ((-1, 5000, 64, 10), (100, 0, 64, 10), (100, 5000, 0, 10), (100, 5000, 62, 10), (100, 5000, 64, 0),
                (100, 5000, 64, 1025), (100, 12, 64, 10), (65535 * 128 + 1, 5000, 64, 10), (100, 5000, 1028, 10)):
        assert ws(*bad) == 0, bad
    assert ws(1, 13, 64, 10) > 0 and ws(65535 * 128, 5000, 64, 10) > 0 and ws(100, 5000, 1024, 1024) > 0


def call(lib, V=100, d=8, n=4, k=5, W=FAKE, abc=FAKE, sims=FAKE, idx=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.glove_analogy_workspace_bytes(max(n, 0), V, d, k)
    return lib.glove_analogy_topk_f32(W, V, d, abc, n, k, sims, idx, ws, ws_bytes, None)


def test_argument_errors_are_reported_on_the_host(lib):
    assert call(lib, V=100, k=98, ws_bytes=1 << 30) == BADARG           # k = V - 2: an excluded id could reach the output
    assert call(lib, V=5000, k=1025, ws_bytes=1 << 30) == BADARG
    assert call(lib, d=10, ws_bytes=1 << 30) == BADARG                  # d % 4 != 0
    assert call(lib, n=-1, ws_bytes=1 << 30) == BADARG
    assert call(lib, k=0, ws_bytes=1 << 30) == BADARG
    for name in ("W", "abc", "sims", "idx", "ws"):
        assert call(lib, **{name: None}) == BADARG, name
    need = lib.glove_analogy_workspace_bytes(4, 100, 8, 5)
    assert call(lib, ws_bytes=need - 1) == WORKSPACE
    assert call(lib, n=0) == 0                                          # nothing to do: no launch
    assert call(lib, n=0, abc=None, sims=None, idx=None) == 0
    assert call(lib, n=0, k=98) == BADARG                               # (sizes are checked before the early return)


# ---- parser and bookkeeping
class RefBackend:
    """analogy_topk by the float64 reference; remembers the table it was handed."""

    def analogy_topk(self, W, abc, k, batch=1024):
        self.W, self.batch = W.clone(), batch
        sims, idx = analogy_ref.topk(W.numpy(), abc.numpy(), k)
        return torch.from_numpy(sims.astype(np.float32)), torch.from_numpy(idx)


GRID = 4
# ids: 0 <UNK>, 1 .. 16 the grid words w00 .. w33, 17 Berlin (capitalised in the vocabulary), 18 .. 21 late words
VOCAB = ["<UNK>"] + ["w%d%d" % (i, j) for i in range(GRID) for j in range(GRID)] + ["Berlin", "x0", "x1", "x2", "x3"]


def grid_table(seed):
    """Rows e_i + f_j for the grid words (so that wi1j1 : wi1j2 :: wi2j1 : wi2j2 holds exactly) plus a little noise."""
    rng = np.random.default_rng(seed)
    W = 0.01 * rng.standard_normal((len(VOCAB), 2 * GRID)).astype(np.float32)
    for i in range(GRID):
        for j in range(GRID):
            W[1 + i * GRID + j, i] += 1.0
            W[1 + i * GRID + j, GRID + j] += 1.0
    W[18:] += rng.standard_normal((4, 2 * GRID)).astype(np.float32)
    return W


@pytest.fixture()
def est(tmp_path):
    from trainer.config_utils import parse_args
    from trainer.estimator import Estimator
    vocab = tmp_path / "vocab.txt"
    vocab.write_text("\n".join(VOCAB))
    params = parse_args(["--train-csv", str(tmp_path / "none.csv"), "--vocab-txt", str(vocab), "--job-dir", str(tmp_path / "job"),
                         "--disable-datetime-path", "--embedding-size", str(2 * GRID), "--optimizer", "Adagrad", "--seed", "1"])
    e = Estimator(params, backend=RefBackend(), device="cpu")
    t = e.model.tables
    t.R = torch.from_numpy(grid_table(0))
    t.C = torch.from_numpy(grid_table(1)[::-1].copy())         # another table altogether: other answers
    return e


QUESTIONS = """: capital-common-countries
w00 w01 w10 w11
W00 w02 w20 w22
w00 w01 w10 w33
w00 w01 missing w11
w00 <UNK> w10 w11
: gram1-plural
w11 w12 w21 w22
Berlin w01 w10 w11
w00 w01 x0 x1

w33 w30 w03 w00
"""


def write_questions(tmp_path, text=QUESTIONS):
    path = tmp_path / "questions.txt"
    path.write_text(text)
    return path


def test_sections_counts_and_json(est, tmp_path):
    q = write_questions(tmp_path)
    rec = est.evaluate_analogies(str(q))
    assert set(rec) == {"global_step", "embeddings", "top_k", "sections", "semantic", "syntactic", "total",
                        "questions_seen", "questions_total"}
    assert [s["name"] for s in rec["sections"]] == ["capital-common-countries", "gram1-plural"]
    for s in rec["sections"] + [rec["semantic"], rec["syntactic"], rec["total"]]:
        assert set(s) - {"name"} == {"correct", "total", "skipped", "accuracy"}
    cap, gram = rec["sections"]
    # lowercased by default: W00 is found; "missing" and <UNK> are skipped; the third question names a wrong answer
    assert (cap["correct"], cap["total"], cap["skipped"]) == (2, 3, 2) and cap["accuracy"] == 2 / 3
    # "Berlin" is lowercased and the vocabulary holds "Berlin" only: skipped; x0 : x1 is no analogy of the table
    assert (gram["total"], gram["skipped"]) == (3, 1)
    assert rec["semantic"] == {k: cap[k] for k in ("correct", "total", "skipped", "accuracy")}
    assert rec["syntactic"] == {k: gram[k] for k in ("correct", "total", "skipped", "accuracy")}
    for key in ("correct", "total", "skipped"):
        assert rec["semantic"][key] + rec["syntactic"][key] == rec["total"][key]
    assert rec["questions_seen"] == 6 and rec["questions_total"] == 9 and rec["top_k"] == 1 and rec["embeddings"] == "row"
    assert rec["global_step"] == 0
    assert json.loads((Path(est.params["job_dir"]) / "eval" / "analogy.json").read_text()) == rec
    want = analogy_ref.score_file(str(q), VOCAB, est.model.tables.R.numpy())
    assert rec == want


def test_lowercasing_can_be_switched_off(est, tmp_path):
    q = write_questions(tmp_path)
    rec = est.evaluate_analogies(str(q), lowercase=False)
    cap, gram = rec["sections"]
    assert (cap["total"], cap["skipped"]) == (2, 3)          # W00 is no vocabulary word as written
    assert (gram["total"], gram["skipped"]) == (4, 0)        # Berlin is
    assert rec == analogy_ref.score_file(str(q), VOCAB, est.model.tables.R.numpy(), lowercase=False)


def test_restrict_vocab_limits_table_candidates_and_questions(est, tmp_path):
    q = write_questions(tmp_path)
    rec = est.evaluate_analogies(str(q), restrict_vocab=17)
    assert est.backend.W.shape == (17, 2 * GRID) and torch.equal(est.backend.W, est.model.tables.R[:17])
    cap, gram = rec["sections"]
    assert (gram["total"], gram["skipped"]) == (2, 2)        # x0 / x1 have ids >= 17
    assert rec == analogy_ref.score_file(str(q), VOCAB, est.model.tables.R.numpy(), restrict=17)
    with pytest.raises(ValueError, match="restrict-vocab"):
        est.evaluate_analogies(str(q), restrict_vocab=len(VOCAB) + 1)
    with pytest.raises(ValueError, match="top-k"):
        est.evaluate_analogies(str(q), restrict_vocab=5, top_k=3)


def test_top_k_counts_a_hit_at_rank_three(est, tmp_path):
    R = est.model.tables.R.numpy()
    a, b, c = 1, 2, 5                                        # w00 : w01 :: w10 : ?
    third = int(analogy_ref.topk(R, [[a, b, c]], 5)[1][0][2])
    q = write_questions(tmp_path, ": s\nw00 w01 w10 %s\n" % VOCAB[third])
    assert est.evaluate_analogies(str(q), top_k=1)["total"]["correct"] == 0
    assert est.evaluate_analogies(str(q), top_k=2)["total"]["correct"] == 0
    rec = est.evaluate_analogies(str(q), top_k=5)
    assert rec["total"]["correct"] == 1 and rec["top_k"] == 5


def test_malformed_line_names_its_line(est, tmp_path):
    q = write_questions(tmp_path, ": s\nw00 w01 w10 w11\n\nw00 w01 w10\n")
    with pytest.raises(ValueError, match="line 4"):
        est.evaluate_analogies(str(q))
    q = write_questions(tmp_path, ": s\nw00 w01 w10 w11 w12\n")
    with pytest.raises(ValueError, match="line 2"):
        est.evaluate_analogies(str(q))


@pytest.mark.parametrize("which", ["row", "col", "sum"])
def test_embeddings_choice_selects_the_table(est, tmp_path, which):
    q = write_questions(tmp_path)
    t = est.model.tables
    want = {"row": t.R, "col": t.C, "sum": t.R + t.C}[which]
    rec = est.evaluate_analogies(str(q), embeddings=which, batch_size=3)
    assert torch.equal(est.backend.W, want) and est.backend.batch == 3 and rec["embeddings"] == which
    assert rec == analogy_ref.score_file(str(q), VOCAB, want.numpy(), embeddings=which)
    with pytest.raises(ValueError, match="embeddings"):
        est.evaluate_analogies(str(q), embeddings="both")


def test_questions_before_any_section_and_an_empty_file(est, tmp_path):
    rec = est.evaluate_analogies(str(write_questions(tmp_path, "w00 w01 w10 w11\n")))
    assert [s["name"] for s in rec["sections"]] == [""] and rec["total"]["correct"] == 1
    rec = est.evaluate_analogies(str(write_questions(tmp_path, ": only\n")))
    assert rec["total"] == {"correct": 0, "total": 0, "skipped": 0, "accuracy": None} and rec["questions_total"] == 0


def test_main_only_parses_arguments(est, tmp_path, monkeypatch):
    """`python -m trainer.analogy`'s main() hands its flags to Estimator.evaluate_analogies of the job's params."""
    from trainer import analogy, estimator
    seen = {}

    class Fake:
        def __init__(self, params):
            seen["params"] = params

        def evaluate_analogies(self, questions, **options):
            seen.update(questions=questions, **options)
            return "rec"
    monkeypatch.setattr(estimator, "Estimator", Fake)
    job = est.params["job_dir"]
    assert analogy.main(job_dir=job, questions="q.txt", embeddings="sum", top_k=3, batch_size=7, restrict_vocab=9, no_lowercase=True) == "rec"
    assert seen["params"]["job_dir"] == job and seen["questions"] == "q.txt"
    assert {k: seen[k] for k in ("embeddings", "top_k", "batch_size", "restrict_vocab", "lowercase")} == \
        {"embeddings": "sum", "top_k": 3, "batch_size": 7, "restrict_vocab": 9, "lowercase": False}
