"""Word-analogy top-k (3CosAdd) on the GPU: glove_analogy_topk_f32 of libglove_eval_hip.so against the float64 reference
of tests/analogy_ref.py, and `python -m trainer.analogy` end to end.

The shapes are the smallest that cross the boundaries of the GEMM and the selection: a query tile of 128, a vocabulary
tile of 128, a k-slab of 32 and a top-k segment of 4,096 candidates.  Of the seven row shapes of the lane-group kernels
their widths (8 .. 300) reach three, 16 x 1, 32 x 1 and 32 x 3: tests/test_gpu_eval_row_shapes.py runs every shape at its
first and its last width, tests/test_gpu_topk_order.py pins the selection's order on exact ties.

Tolerances.  Scores: rtol 1e-5, atol 1e-6, the figures of test_topk_cosine (the same GEMM, one more rounding per query
element); the same formula in float32 NumPy deviates from float64 by 2.8e-7 at most over the six parity cases (the kernel: 2.9e-7 on an MI355X).  Ids
are compared at every (question, rank) whose float64 score is at least 1e-5 away from both neighbours in the reference's
ranking; the reference alone leaves out 1.31 % of the positions at most (the (64, 8, 61, 5) case, whose ranking holds the
whole vocabulary), the cap is 2 %."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import analogy_ref
from helpers import to_dev

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
RTOL, ATOL, GAP, LEFT_OUT_MAX = 1e-5, 1e-6, 1e-5, 0.02

CASES = [(64, 8, 16, 40), (64, 8, 61, 5), (500, 64, 20, 200), (1000, 300, 5, 257), (3000, 128, 33, 300), (40003, 52, 20, 301)]


def questions(rng, V, n):
    """Three distinct random ids per question; the first rows are forced onto the edges of the tiles and segments."""
    abc = np.stack([rng.choice(V, 3, replace=False) for _ in range(n)]).astype(np.int32)
    edges = [0, 127, 128, V - 1] + [e for s in range(4096, V, 4096) for e in (s - 1, s)]
    for i, e in enumerate([e for e in dict.fromkeys(edges) if 0 <= e < V][:n]):
        others = [x for x in rng.choice(V, 3, replace=False) if x != e][:2]
        abc[i] = np.roll([e] + others, i % 3)
    assert all(len(set(q)) == 3 for q in abc.tolist())
    return abc


@functools.lru_cache(maxsize=None)
def case(V, d, k, n):
    """(W, abc, reference sims [n, k + 1], reference idx [n, k + 1]): computed once, shared, never written to."""
    rng = np.random.default_rng(1000 + V + d)
    W = rng.standard_normal((V, d)).astype(np.float32)
    abc = questions(rng, V, n)
    sims, idx = analogy_ref.topk(W, abc, k, extra=1)
    for a in (sims, idx):
        a.setflags(write=False)
    return W, abc, sims, idx


def check_parity(got_s, got_i, want_s_ext, want_i_ext, abc, k, what=""):
    """The three parity checks of a result [n, k] against the reference's [n, k + 1]; returns the share of positions left
    out of the id comparison."""
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    want_s, want_i = want_s_ext[:, :k], want_i_ext[:, :k]
    print("%s: largest score deviation %.3g" % (what, np.abs(got_s - want_s).max()))
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=ATOL, err_msg=what)
    clear = analogy_ref.separated(want_s_ext, k, GAP)
    left_out = 1.0 - clear.mean()
    print("%s: %.2f %% of the positions left out of the id comparison" % (what, 100 * left_out))
    assert left_out <= LEFT_OUT_MAX, what
    assert (got_i[clear] == want_i[clear]).all(), (what, np.argwhere(clear & (got_i != want_i))[:5])
    assert not (got_i[:, :, None] == np.asarray(abc)[:, None, :]).any(), what        # a, b and c are no answers
    assert ((got_i >= 0) & np.isfinite(got_s)).all(), what
    return left_out


@pytest.mark.parametrize("V,d,k,n", CASES)
def test_parity_with_the_float64_reference(hip, V, d, k, n):
    W, abc, want_s, want_i = case(V, d, k, n)
    sims, idx = hip.analogy_topk(*to_dev(W, abc), k)
    assert sims.shape == idx.shape == (n, k) and sims.dtype == torch.float32 and idx.dtype == torch.int32
    check_parity(sims, idx, want_s, want_i, abc, k, "V=%d d=%d k=%d n=%d" % (V, d, k, n))
    got = sims.cpu().numpy()
    assert (got[:, :-1] >= got[:, 1:]).all()                 # descending


def test_planted_answers_come_out_first(hip):
    V0, d, n = 936, 64, 64
    rng = np.random.default_rng(3)
    W = rng.standard_normal((V0 + n, d))
    abc = np.stack([rng.choice(V0, 3, replace=False) for _ in range(n)]).astype(np.int32)
    unit = W / np.linalg.norm(W, axis=1, keepdims=True)
    W[V0:] = unit[abc[:, 1]] - unit[abc[:, 0]] + unit[abc[:, 2]] + 1e-3 * rng.standard_normal((n, d))
    sims, idx = hip.analogy_topk(*to_dev(W.astype(np.float32), abc), 1)
    assert idx[:, 0].cpu().tolist() == list(range(V0, V0 + n))
    assert (sims[:, 0].cpu() - 1).abs().max() < 1e-4


def test_degenerate_questions_and_rows(hip):
    V, d = 200, 16
    k = V - 3                                                # the whole ranking
    rng = np.random.default_rng(4)
    W = rng.standard_normal((V, d)).astype(np.float32)
    W[11] = 0.0                                              # a row the clamp has to hold
    W[7] = W[3]                                              # two identical candidates
    abc = np.array([[5, 5, 9],                               # a == b: the query is c's direction
                    [20, 30, 20],                            # a == c: the query is b's direction
                    [40, 50, 50],                            # b == c
                    [60, 60, 60],                            # all the same word
                    [11, 2, 13],                             # the zero row as a
                    [21, 11, 23], [31, 32, 11],              # ... as b, as c
                    [70, 80, 90]], np.int32)
    sims, idx = hip.analogy_topk(*to_dev(W, abc), k)
    want_s, want_i = analogy_ref.topk(W, abc, k, extra=1)
    check_parity(sims, idx, want_s, want_i, abc, k, "degenerate")
    got_s, got_i = sims.cpu().numpy(), idx.cpu().numpy()
    assert np.isfinite(got_s).all()
    # a == b: the answer is c's nearest neighbour other than c (and other than a, which is no candidate)
    unit = W.astype(np.float64) / np.sqrt(np.maximum((W.astype(np.float64) ** 2).sum(1, keepdims=True), 1e-12))
    near = unit @ unit[9]
    near[[5, 9]] = -np.inf
    order = np.argsort(-near, kind="stable")
    assert near[order[0]] - near[order[1]] > GAP and got_i[0, 0] == order[0]
    # identical rows: adjacent, the lower id first, in every ranking
    for q, row in enumerate(got_i.tolist()):
        assert row.index(7) == row.index(3) + 1
        assert len(set(row)) == k and not set(row) & set(abc[q].tolist())


def test_padded_row_stride(hip):
    V, dm, d, k, n = 300, 10, 12, 9, 150
    rng = np.random.default_rng(5)
    W = np.zeros((V, d), np.float32)
    W[:, :dm] = rng.standard_normal((V, dm))
    abc = questions(rng, V, n)
    Wd, qd = to_dev(W, abc)
    first = hip.analogy_topk(Wd, qd, k)
    second = hip.analogy_topk(Wd, qd, k)
    np.testing.assert_allclose(first[0].cpu().numpy(), second[0].cpu().numpy(), rtol=1e-6, atol=1e-7)
    assert torch.equal(first[1], second[1])
    want_s, want_i = analogy_ref.topk(W[:, :dm], abc, k, extra=1)                 # the table without its padding
    check_parity(*first, want_s, want_i, abc, k, "padded stride")


def test_repeatable_and_batched_calls_are_bitwise_equal(hip):
    V, d, k, n = 40003, 52, 20, 301
    W, abc, _, _ = case(V, d, k, n)
    Wd, qd = to_dev(W, abc)
    one = hip.analogy_topk(Wd, qd, k)
    again = hip.analogy_topk(Wd, qd, k)
    batched = hip.analogy_topk(Wd, qd, k, batch=128)         # 128 + 128 + 45 through one workspace
    for other in (again, batched):
        assert torch.equal(one[0], other[0]) and torch.equal(one[1], other[1])
    empty = hip.analogy_topk(Wd, qd[:0], k)
    assert empty[0].shape == (0, k) and empty[1].shape == (0, k)


def test_captured_call_replays_like_the_eager_one(hip):
    V, d, k, n = 3000, 128, 33, 300
    W, abc, _, _ = case(V, d, k, n)
    Wd, qd = to_dev(W, abc)
    eager = hip.analogy_topk(Wd, qd, k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.analogy_topk(Wd, qd, k)                          # warm the launch paths outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sims, idx = hip.analogy_topk(Wd, qd, k)
    for _ in range(2):
        sims.fill_(float("nan"))
        idx.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sims, eager[0]) and torch.equal(idx, eager[1])


def test_predict_path_is_unchanged_by_an_analogy_call(hip):
    rng = np.random.default_rng(6)
    R, q = to_dev(rng.standard_normal((500, 64)).astype(np.float32), np.array([0, 3, 127, 128, 499], np.int32))
    before = hip.topk_cosine(R, q, 20)
    W, abc, _, _ = case(500, 64, 20, 200)
    hip.analogy_topk(*to_dev(W, abc), 20)
    after = hip.topk_cosine(R, q, 20)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert before[1][:, 0].cpu().tolist() == [0, 3, 127, 128, 499]


def test_argument_errors_raise(hip):
    from trainer.hip_api import GloveHipError
    W, abc = to_dev(np.ones((10, 8), np.float32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(GloveHipError, match="BADARG"):
        hip.analogy_topk(W, abc, 8)                          # k = V - 2
    with pytest.raises(GloveHipError):
        hip.analogy_topk(W, abc.long(), 3)


def test_cli_end_to_end(hip, tmp_path):
    """Train a tiny job, ask `python -m trainer.analogy` (a child process) about a question file made from its
    vocabulary, and compare analogy.json with the reference scorer on the checkpoint's tables."""
    from trainer import estimator
    csv, vocab_txt = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    job = tmp_path / "job"
    estimator.main(["--train-csv", str(csv), "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path",
                    "--embedding-size", "50", "--optimizer", "Adagrad", "--learning-rate", "0.05", "--batch-size", "64",
                    "--train-steps", "60", "--log-every", "20", "--seed", "7", "--skip-eval"])
    blob = torch.load(job / "model.ckpt-60.pt", weights_only=False)["tables"]
    vocab = vocab_txt.read_text().split("\n")
    words = [w for w in vocab if w != "<UNK>"]
    rng = np.random.default_rng(8)
    tables = {"row": blob["R"].numpy(), "sum": (blob["R"] + blob["C"]).numpy()}
    for which, W in tables.items():
        # half of the questions ask for what the reference finds, the rest for a random word
        lines, close, asked, sure = [": capital-test"], 0, 0, 0
        for i in range(80):
            if i == 40:
                lines.append(": gram1-test")
            a, b, c = rng.choice(len(words), 3, replace=False)
            ids = [vocab.index(words[j]) for j in (a, b, c)]
            s, top = analogy_ref.topk(W, [ids], 2)
            close += int(s[0, 0] - s[0, 1] < GAP)
            asked += 1
            best = [vocab[v] for v in top[0] if vocab[v] != "<UNK>"][0]       # (<UNK> has a row and can rank first; asking for it would skip the question)
            sure += int(i % 2 == 0 and best == vocab[top[0, 0]])
            answer = best if i % 2 == 0 else words[rng.integers(len(words))]
            lines.append(" ".join([words[a], words[b], words[c], answer]))
        lines.insert(5, "the of zzz-not-a-word the")
        assert close <= LEFT_OUT_MAX * asked                 # the reference's own near-ties, capped first
        qfile = tmp_path / ("questions_%s.txt" % which)
        qfile.write_text("\n".join(lines) + "\n")
        proc = subprocess.run([sys.executable, "-m", "trainer.analogy", "--job-dir", str(job), "--questions", str(qfile),
                               "--embeddings", which], cwd=str(REPO), capture_output=True, text=True, timeout=240)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        got = json.loads((job / "eval" / "analogy.json").read_text())
        want = analogy_ref.score_file(str(qfile), vocab, W, embeddings=which, global_step=60)
        assert [s["name"] for s in got["sections"]] == ["capital-test", "gram1-test"]
        assert got["sections"][0]["skipped"] == 1 and got["questions_total"] == 81 and got["questions_seen"] == 80
        for key in ("global_step", "embeddings", "top_k", "questions_seen", "questions_total"):
            assert got[key] == want[key], key
        for g, w in zip(got["sections"] + [got["semantic"], got["syntactic"], got["total"]],
                        want["sections"] + [want["semantic"], want["syntactic"], want["total"]]):
            assert (g["total"], g["skipped"]) == (w["total"], w["skipped"])
            assert abs(g["correct"] - w["correct"]) <= close
        assert sure >= 30 and got["total"]["correct"] >= sure - close      # the questions that ask for the reference's first answer
        assert "analogies, gram1-test" in proc.stderr
