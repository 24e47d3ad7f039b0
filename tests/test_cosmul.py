"""3CosMul analogies and the pair cosine without a GPU: the surface of include/glove_eval_sim_hip.h (the second header of
libglove_eval_hip.so), its host-side argument checks (they happen before any launch), and Estimator.evaluate_analogies
with method="3cosmul" through a test-only backend whose analogy_cosmul_topk is the float64 reference."""
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import analogy_ref
import cosmul_ref
from test_analogy import FAKE, QUESTIONS, VOCAB, GRID, RefBackend, declared_functions, grid_table, write_questions

REPO = Path(__file__).resolve().parent.parent
SIM_HEADER = REPO / "include" / "glove_eval_sim_hip.h"
EVAL_HEADER = REPO / "include" / "glove_eval_hip.h"
BADARG, WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.EVAL_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_eval_library()


# ---- library surface
def test_sim_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(SIM_HEADER)
    assert set(names) == set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS) and len(names) == 4
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_eval_sim_abi_version() == hip_api.GLOVE_EVAL_SIM_ABI_VERSION == 1
    assert "GLOVE_EVAL_SIM_ABI_VERSION 1" in SIM_HEADER.read_text()
    # the first header keeps its three functions and its version; no name is declared twice
    assert set(declared_functions(EVAL_HEADER)) == set(hip_api.EVAL_EXPORTED_SYMBOLS) and len(hip_api.EVAL_EXPORTED_SYMBOLS) == 3
    assert not set(names) & set(hip_api.EVAL_EXPORTED_SYMBOLS) and not set(names) & set(hip_api.EXPORTED_SYMBOLS)
    assert lib.glove_eval_abi_version() == 1


def test_new_symbols_are_no_part_of_the_training_library():
    from trainer import hip_api
    train = hip_api.load_library()
    for n in hip_api.EVAL_SIM_EXPORTED_SYMBOLS:
        assert not hasattr(train, n), n


def test_workspace_query_is_the_stated_layout(lib):
    ws = lib.glove_cosmul_workspace_bytes
    up = lambda x: (x + 255) // 256 * 256
    # inv_norm[V] | scores[n V] | 2 x (values + ids of ceil(V / 4096) k winners per question), each piece 256-B aligned
    layout = lambda n, V, k: up(V * 4) + up(n * V * 4) + 4 * up(n * ((V + 4095) // 4096) * k * 4)
    for n, V, d, k in ((100, 5000, 64, 10), (1, 13, 64, 10), (0, 5000, 64, 10), (301, 40003, 52, 20), (7, 4096, 8, 1024),
                       (7, 4097, 8, 1024)):
        assert ws(n, V, d, k) == layout(n, V, k), (n, V, d, k)
    base = ws(100, 5000, 64, 10)
    assert ws(101, 5000, 64, 10) > base and ws(100, 5001, 64, 10) > base and ws(100, 5000, 64, 11) > base
    assert ws(100, 5000, 68, 10) == base                     # no piece holds query rows: d sizes nothing
    assert ws(0, 5000, 64, 10) > 0
    # no 3n x V matrix: smaller than three score matrices, and than the 3CosAdd workspace (which also holds Q and q_inv)
    assert base < 3 * 100 * 5000 * 4 and base < lib.glove_analogy_workspace_bytes(100, 5000, 64, 10)
    for bad in ((-1, 5000, 64, 10), (100, 0, 64, 10), (100, 5000, 0, 10), (100, 5000, 62, 10), (100, 5000, 64, 0),
                (100, 5000, 64, 1025), (100, 12, 64, 10), (65535 * 128 + 1, 5000, 64, 10), (100, 5000, 1028, 10)):
        assert ws(*bad) == 0, bad
    assert ws(1, 13, 64, 10) > 0 and ws(65535 * 128, 5000, 64, 10) > 0 and ws(100, 5000, 1024, 1024) > 0


def call(lib, V=100, d=8, n=4, k=5, eps=1e-3, W=FAKE, abc=FAKE, sims=FAKE, idx=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.glove_cosmul_workspace_bytes(max(n, 0), V, d, k)
    return lib.glove_cosmul_topk_f32(W, V, d, abc, n, k, eps, sims, idx, ws, ws_bytes, None)


def test_cosmul_argument_errors_are_reported_on_the_host(lib):
    assert call(lib, V=100, k=98, ws_bytes=1 << 30) == BADARG           # k = V - 2: an excluded id could reach the output
    assert call(lib, V=5000, k=1025, ws_bytes=1 << 30) == BADARG
    assert call(lib, d=10, ws_bytes=1 << 30) == BADARG                  # d % 4 != 0
    assert call(lib, n=-1, ws_bytes=1 << 30) == BADARG
    assert call(lib, k=0, ws_bytes=1 << 30) == BADARG
    for eps in (0.0, -1e-3, math.nan, 1.0 + 1e-6, 2.0, math.inf, -math.inf):
        assert call(lib, eps=eps) == BADARG, eps
    for name in ("W", "abc", "sims", "idx", "ws"):
        assert call(lib, **{name: None}) == BADARG, name
    need = lib.glove_cosmul_workspace_bytes(4, 100, 8, 5)
    assert call(lib, ws_bytes=need - 1) == WORKSPACE
    assert call(lib, n=0) == 0                                          # nothing to do: no launch
    assert call(lib, n=0, eps=1.0) == 0 and call(lib, n=0, eps=1e-6) == 0
    assert call(lib, n=0, abc=None, sims=None, idx=None) == 0
    assert call(lib, n=0, k=98) == BADARG                               # (sizes are checked before the early return)
    assert call(lib, n=0, eps=0.0) == BADARG                            # (eps too)


def test_pair_cosine_argument_errors_are_reported_on_the_host(lib):
    f = lib.glove_pair_cosine_f32
    assert f(FAKE, 100, 8, FAKE, 0, FAKE, None) == 0                    # nothing to do: no launch
    assert f(FAKE, 100, 8, None, 0, None, None) == 0
    for args in ((None, 100, 8, FAKE, 4, FAKE), (FAKE, 100, 8, None, 4, FAKE), (FAKE, 100, 8, FAKE, 4, None),
                 (FAKE, 100, 10, FAKE, 4, FAKE), (FAKE, 100, 0, FAKE, 4, FAKE), (FAKE, 100, 1028, FAKE, 4, FAKE),
                 (FAKE, 0, 8, FAKE, 4, FAKE), (FAKE, 100, 8, FAKE, -1, FAKE), (FAKE, 100, 10, FAKE, 0, FAKE)):
        assert f(*args, None) == BADARG, args


# ---- the Estimator through a reference backend
class BothBackend(RefBackend):
    """analogy_topk of test_analogy.RefBackend plus analogy_cosmul_topk by the float64 reference; remembers its calls."""

    def __init__(self):
        self.calls = []

    def analogy_topk(self, W, abc, k, batch=1024):
        self.calls.append(("3cosadd", None, batch))
        return super().analogy_topk(W, abc, k, batch)

    def analogy_cosmul_topk(self, W, abc, k, eps=1e-3, batch=1024):
        self.calls.append(("3cosmul", eps, batch))
        self.W = W.clone()
        sims, idx = cosmul_ref.topk(W.numpy(), abc.numpy(), k, eps)
        return torch.from_numpy(sims.astype(np.float32)), torch.from_numpy(idx)


def make_estimator(tmp_path, vocab, R, C=None):
    from trainer.config_utils import parse_args
    from trainer.estimator import Estimator
    path = tmp_path / "vocab.txt"
    path.write_text("\n".join(vocab))
    params = parse_args(["--train-csv", str(tmp_path / "none.csv"), "--vocab-txt", str(path), "--job-dir", str(tmp_path / "job"),
                         "--disable-datetime-path", "--embedding-size", str(R.shape[1]), "--optimizer", "Adagrad", "--seed", "1"])
    e = Estimator(params, backend=BothBackend(), device="cpu")
    e.model.tables.R = torch.from_numpy(R)
    e.model.tables.C = torch.from_numpy(R[::-1].copy() if C is None else C)
    return e


@pytest.fixture()
def est(tmp_path):
    return make_estimator(tmp_path, VOCAB, grid_table(0), grid_table(1)[::-1].copy())


def test_cosmul_record_file_and_backend_call(est, tmp_path):
    q = write_questions(tmp_path)
    rec = est.evaluate_analogies(str(q), method="3cosmul", epsilon=1e-4, batch_size=5)
    assert est.backend.calls == [("3cosmul", 1e-4, 5)]
    assert rec == cosmul_ref.score_file(str(q), VOCAB, est.model.tables.R.numpy(), eps=1e-4)
    assert rec["method"] == "3cosmul" and rec["epsilon"] == 1e-4 and rec["questions_seen"] == 6
    eval_dir = Path(est.params["job_dir"]) / "eval"
    assert json.loads((eval_dir / "analogy_3cosmul.json").read_text()) == rec
    assert not (eval_dir / "analogy.json").exists()                     # the two methods never overwrite each other
    assert est.evaluate_analogies(str(q), method="3cosmul")["epsilon"] == 1e-3 and est.backend.calls[-1] == ("3cosmul", 1e-3, 1024)
    rec = est.evaluate_analogies(str(q), method="3cosmul", embeddings="sum", restrict_vocab=17, top_k=2, lowercase=False)
    t = est.model.tables
    assert rec == cosmul_ref.score_file(str(q), VOCAB, (t.R + t.C).numpy(), top_k=2, restrict=17, lowercase=False, embeddings="sum")
    assert est.backend.W.shape == (17, 2 * GRID)


def test_default_call_is_what_it_was(est, tmp_path):
    q = write_questions(tmp_path)
    est.evaluate_analogies(str(q), method="3cosmul")
    cosmul_file = Path(est.params["job_dir"]) / "eval" / "analogy_3cosmul.json"
    before = cosmul_file.read_text()
    rec = est.evaluate_analogies(str(q))
    assert est.backend.calls[-1] == ("3cosadd", None, 1024)
    assert set(rec) == {"global_step", "embeddings", "top_k", "sections", "semantic", "syntactic", "total",
                        "questions_seen", "questions_total"}
    assert rec == analogy_ref.score_file(str(q), VOCAB, est.model.tables.R.numpy())
    assert rec == est.evaluate_analogies(str(q), method="3cosadd", epsilon=0.5)      # epsilon plays no part in 3cosadd
    assert json.loads((Path(est.params["job_dir"]) / "eval" / "analogy.json").read_text()) == rec
    assert cosmul_file.read_text() == before


def test_unknown_method_and_bad_epsilon_raise(est, tmp_path):
    q = write_questions(tmp_path)
    with pytest.raises(ValueError, match="--method"):
        est.evaluate_analogies(str(q), method="3cosdiv")
    for eps in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="--epsilon"):
            est.evaluate_analogies(str(q), method="3cosmul", epsilon=eps)
    assert est.backend.calls == []


def test_the_two_methods_can_name_different_first_answers(tmp_path):
    """A small random table and the first question on which the references disagree, both with a clear margin."""
    rng = np.random.default_rng(11)
    V, d = 40, 4
    W = rng.standard_normal((V, d)).astype(np.float32)
    vocab = ["t%d" % i for i in range(V)]
    found = None
    for a, b, c in (rng.choice(V, 3, replace=False) for _ in range(200)):
        sa, ia = analogy_ref.topk(W, [[a, b, c]], 2)
        sm, im = cosmul_ref.topk(W, [[a, b, c]], 2, 1e-3)
        if ia[0, 0] != im[0, 0] and sa[0, 0] - sa[0, 1] > 1e-3 and sm[0, 0] - sm[0, 1] > 1e-3 * sm[0, 0]:
            found = (int(a), int(b), int(c), int(ia[0, 0]), int(im[0, 0]))
            break
    assert found is not None
    a, b, c, by_add, by_mul = found
    assert by_add != by_mul
    e = make_estimator(tmp_path, vocab, W)
    for want, name in ((by_add, "add"), (by_mul, "mul")):
        q = tmp_path / ("q_%s.txt" % name)
        q.write_text(": s\n%s %s %s %s\n" % (vocab[a], vocab[b], vocab[c], vocab[want]))
        assert e.evaluate_analogies(str(q))["total"]["correct"] == int(name == "add")
        assert e.evaluate_analogies(str(q), method="3cosmul")["total"]["correct"] == int(name == "mul")


def test_analogy_main_forwards_method_and_epsilon(est, monkeypatch):
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
    assert analogy.main(job_dir=job, questions="q.txt", method="3cosmul", epsilon=1e-6) == "rec"
    assert seen["method"] == "3cosmul" and seen["epsilon"] == 1e-6 and seen["questions"] == "q.txt"
    analogy.main(job_dir=job, questions="q.txt")
    assert seen["method"] == "3cosadd" and seen["epsilon"] == 1e-3
    assert "gensim uses 1e-6" in Path(analogy.__file__).read_text()


def test_the_product_backend_forwards_the_new_calls():
    """The Estimator reaches the binding through trainer.stepper.HipBackend: it has to offer what the test backends do."""
    from trainer.hip_api import GloveHip
    from trainer.stepper import HipBackend
    for name in ("analogy_topk", "analogy_cosmul_topk", "pair_cosine"):
        assert callable(getattr(HipBackend, name, None)) and callable(getattr(GloveHip, name, None)), name
