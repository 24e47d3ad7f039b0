"""3CosMul word-analogy top-k on the GPU: glove_cosmul_topk_f32 of libglove_eval_hip.so against the float64 reference of
tests/cosmul_ref.py, and `python -m trainer.analogy --method 3cosmul` end to end.

The shapes and the question generator are those of tests/test_gpu_analogy.py: they cross a vocabulary tile of 128, a
k-slab of 32 (d below it, and no multiple of it), a top-k segment of 4,096 candidates, and question counts that are no
multiple of 32, 64 or 128 (the question tile is 64).  The row shapes of the lane-group kernels beyond the three these
widths reach are run by tests/test_gpu_eval_row_shapes.py.

Tolerances.  Scores: rtol 1e-5, atol 1e-6, the project's figures for this GEMM.  The same formula in float32 NumPy
deviates from float64 by 8.3e-7 relative at most (4.8e-6 absolute, at scores up to 7.5) over the six parity cases with
this file's questions and both eps values; four times that stays below the tolerance, which therefore stands as it is.
The kernel on an MI355X: 8.4e-7 relative at most (5.5e-6 absolute) over the same eight runs.  Ids are compared at every (question, rank) whose float64 score s is at least
1e-5 max(1, |s|) away from both neighbours in the reference's ranking; the reference alone leaves out 0.88 % of the
positions at most (the (3000, 128, 33, 300) case), the cap is 2 % and is asserted first."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import analogy_ref
import cosmul_ref
from helpers import to_dev
from test_gpu_analogy import CASES, questions

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
RTOL, ATOL, GAP, LEFT_OUT_MAX = 1e-5, 1e-6, 1e-5, 0.02
EPS_CASES = [(c, 1e-3) for c in CASES] + [((64, 8, 61, 5), 1e-6), ((40003, 52, 20, 301), 1e-6)]


@functools.lru_cache(maxsize=None)
def table(V, d, n):
    """(W, abc): computed once, shared, never written to."""
    rng = np.random.default_rng(1000 + V + d)
    W = rng.standard_normal((V, d)).astype(np.float32)
    abc = questions(rng, V, n)
    for a in (W, abc):
        a.setflags(write=False)
    return W, abc


@functools.lru_cache(maxsize=None)
def case(V, d, k, n, eps):
    """(W, abc, reference scores [n, k + 1], reference idx [n, k + 1])."""
    W, abc = table(V, d, n)
    sims, idx = cosmul_ref.topk(W, abc, k, eps, extra=1)
    for a in (sims, idx):
        a.setflags(write=False)
    return W, abc, sims, idx


def check_parity(got_s, got_i, want_s_ext, want_i_ext, abc, k, what=""):
    """The parity checks of a result [n, k] against the reference's [n, k + 1]."""
    got_s, got_i = np.asarray(got_s.cpu()), np.asarray(got_i.cpu())
    want_s, want_i = want_s_ext[:, :k], want_i_ext[:, :k]
    dev = np.abs(got_s - want_s)
    print("%s: largest score deviation %.3g absolute, %.3g relative, largest score %.3g"
          % (what, dev.max(), (dev / np.maximum(np.abs(want_s), 1e-30)).max(), want_s.max()))
    assert np.isfinite(got_s).all() and (got_i >= 0).all(), what
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=ATOL, err_msg=what)
    clear = cosmul_ref.separated(want_s_ext, k, GAP)
    left_out = 1.0 - clear.mean()
    print("%s: %.2f %% of the positions left out of the id comparison" % (what, 100 * left_out))
    assert left_out <= LEFT_OUT_MAX, what
    assert (got_i[clear] == want_i[clear]).all(), (what, np.argwhere(clear & (got_i != want_i))[:5])
    assert not (got_i[:, :, None] == np.asarray(abc)[:, None, :]).any(), what        # a, b and c are no answers
    assert (got_s[:, :-1] >= got_s[:, 1:]).all(), what                               # descending


@pytest.mark.parametrize("shape,eps", EPS_CASES)
def test_parity_with_the_float64_reference(hip, shape, eps):
    V, d, k, n = shape
    W, abc, want_s, want_i = case(V, d, k, n, eps)
    sims, idx = hip.analogy_cosmul_topk(*to_dev(W, abc), k, eps)
    assert sims.shape == idx.shape == (n, k) and sims.dtype == torch.float32 and idx.dtype == torch.int32
    check_parity(sims, idx, want_s, want_i, abc, k, "V=%d d=%d k=%d n=%d eps=%g" % (V, d, k, n, eps))


def degenerate_table():
    V, d = 200, 16
    rng = np.random.default_rng(4)
    W = rng.standard_normal((V, d)).astype(np.float32)
    W[11] = 0.0                                              # a row the clamp has to hold
    W[7] = W[3]                                              # two identical candidates
    # a row and its negative whose cosine is -1 in any arithmetic: |W[70]|^2 = 16 and the inverse norm 1/4 are exact, so
    # s(a, 71) = 0 and the denominator is eps itself.  (With a generic row a float32 cosine may stop an ulp short of -1:
    # 3e-8 in the denominator, 3e-5 of eps = 1e-3, which no float32 arithmetic brings under rtol 1e-5.)
    W[70] = 0.0
    W[70, :4] = 2.0
    W[71] = -W[70]
    abc = np.array([[5, 5, 9],                               # a == b
                    [20, 30, 20],                            # a == c
                    [40, 50, 50],                            # b == c
                    [60, 60, 60],                            # all the same word
                    [11, 2, 13],                             # the zero row as a
                    [21, 11, 23], [31, 32, 11],              # ... as b, as c
                    [70, 80, 90]], np.int32)                 # -W[a] is a candidate
    return W, abc


def test_degenerate_questions_and_rows(hip):
    W, abc = degenerate_table()
    V, eps = len(W), 1e-3
    k = V - 3                                                # the whole ranking
    sims, idx = hip.analogy_cosmul_topk(*to_dev(W, abc), k, eps)
    want_s, want_i = cosmul_ref.topk(W, abc, k, eps, extra=1)
    check_parity(sims, idx, want_s, want_i, abc, k, "degenerate")
    got_s, got_i = sims.cpu().numpy(), idx.cpu().numpy()
    # identical rows: adjacent, the lower id first, in every ranking
    for q, row in enumerate(got_i.tolist()):
        assert row.index(7) == row.index(3) + 1
        assert len(set(row)) == k and not set(row) & set(abc[q].tolist())
    # the candidate -W[a]: s(a, v) = 0, the score is s(b, v) s(c, v) / eps, finite
    unit = cosmul_ref.unit_rows(W)
    want = (1 + unit[80] @ unit[71]) / 2 * (1 + unit[90] @ unit[71]) / 2 / eps
    at = got_i[7].tolist().index(71)
    assert np.isfinite(got_s[7, at]) and got_s[7, at] == pytest.approx(want, rel=RTOL)
    assert want_s[7, want_i[7].tolist().index(71)] == pytest.approx(want, rel=1e-12)


def test_padded_row_stride(hip):
    V, dm, d, k, n = 300, 10, 12, 9, 150
    rng = np.random.default_rng(5)
    W = np.zeros((V, d), np.float32)
    W[:, :dm] = rng.standard_normal((V, dm))
    abc = questions(rng, V, n)
    got = hip.analogy_cosmul_topk(*to_dev(W, abc), k)
    want_s, want_i = cosmul_ref.topk(W[:, :dm], abc, k, 1e-3, extra=1)              # the table without its padding
    check_parity(*got, want_s, want_i, abc, k, "padded stride")


def test_repeatable_and_batched_calls_are_bitwise_equal(hip):
    V, d, k, n = 40003, 52, 20, 301
    W, abc = table(V, d, n)
    Wd, qd = to_dev(W, abc)
    one = hip.analogy_cosmul_topk(Wd, qd, k)
    again = hip.analogy_cosmul_topk(Wd, qd, k)
    batched = hip.analogy_cosmul_topk(Wd, qd, k, batch=128)  # 128 + 128 + 45 through one workspace
    odd = hip.analogy_cosmul_topk(Wd, qd, k, batch=33)       # no question keeps its place in a tile
    for other in (again, batched, odd):
        assert torch.equal(one[0], other[0]) and torch.equal(one[1], other[1])
    empty = hip.analogy_cosmul_topk(Wd, qd[:0], k)
    assert empty[0].shape == (0, k) and empty[1].shape == (0, k)


def test_captured_call_replays_like_the_eager_one(hip):
    V, d, k, n = 3000, 128, 33, 300
    W, abc = table(V, d, n)
    Wd, qd = to_dev(W, abc)
    eager = hip.analogy_cosmul_topk(Wd, qd, k)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.analogy_cosmul_topk(Wd, qd, k)                   # warm the launch paths outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sims, idx = hip.analogy_cosmul_topk(Wd, qd, k)
    for _ in range(2):
        sims.fill_(float("nan"))
        idx.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(sims, eager[0]) and torch.equal(idx, eager[1])


def test_the_other_top_k_paths_are_unchanged_by_a_cosmul_call(hip):
    rng = np.random.default_rng(6)
    R, q = to_dev(rng.standard_normal((500, 64)).astype(np.float32), np.array([0, 3, 127, 128, 499], np.int32))
    W, abc = table(500, 64, 200)
    Wd, qd = to_dev(W, abc)
    before = hip.topk_cosine(R, q, 20), hip.analogy_topk(Wd, qd, 20)
    hip.analogy_cosmul_topk(Wd, qd, 20)
    after = hip.topk_cosine(R, q, 20), hip.analogy_topk(Wd, qd, 20)
    for b, a in zip(before, after):
        assert torch.equal(b[0], a[0]) and torch.equal(b[1], a[1])
    assert before[0][1][:, 0].cpu().tolist() == [0, 3, 127, 128, 499]
    want_s, want_i = analogy_ref.topk(W, abc, 20)
    np.testing.assert_allclose(after[1][0].cpu().numpy(), want_s, rtol=RTOL, atol=ATOL)


def test_argument_errors_raise(hip):
    from trainer.hip_api import GloveHipError
    W, abc = to_dev(np.ones((10, 8), np.float32), np.array([[0, 1, 2]], np.int32))
    with pytest.raises(GloveHipError, match="BADARG"):
        hip.analogy_cosmul_topk(W, abc, 8)                   # k = V - 2
    with pytest.raises(GloveHipError, match="BADARG"):
        hip.analogy_cosmul_topk(W, abc, 3, eps=0.0)
    with pytest.raises(GloveHipError):
        hip.analogy_cosmul_topk(W, abc.long(), 3)
    with pytest.raises(GloveHipError):
        hip.analogy_cosmul_topk(W, abc, 3, batch=0)


def test_cli_end_to_end(hip, tmp_path):
    """Train a tiny job, ask `python -m trainer.analogy --method 3cosmul` (a child process) about a question file made
    from its vocabulary, and compare analogy_3cosmul.json with the reference scorer on the checkpoint's table."""
    from trainer import estimator
    csv, vocab_txt = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    job = tmp_path / "job"
    estimator.main(["--train-csv", str(csv), "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path",
                    "--embedding-size", "50", "--optimizer", "Adagrad", "--learning-rate", "0.05", "--batch-size", "64",
                    "--train-steps", "60", "--log-every", "20", "--seed", "7", "--skip-eval"])
    W = torch.load(job / "model.ckpt-60.pt", weights_only=False)["tables"]["R"].numpy()
    vocab = vocab_txt.read_text().split("\n")
    words = [w for w in vocab if w != "<UNK>"]
    rng = np.random.default_rng(9)
    eps = 1e-3
    # half of the questions ask for what the reference finds, the rest for a random word
    lines, close, asked, sure = [": capital-test"], 0, 0, 0
    for i in range(80):
        if i == 40:
            lines.append(": gram1-test")
        a, b, c = rng.choice(len(words), 3, replace=False)
        ids = [vocab.index(words[j]) for j in (a, b, c)]
        s, top = cosmul_ref.topk(W, [ids], 2, eps)
        close += int(s[0, 0] - s[0, 1] < GAP * max(1.0, s[0, 0]))
        asked += 1
        best = [vocab[v] for v in top[0] if vocab[v] != "<UNK>"][0]       # (<UNK> has a row and can rank first; asking for it would skip the question)
        sure += int(i % 2 == 0 and best == vocab[top[0, 0]])
        answer = best if i % 2 == 0 else words[rng.integers(len(words))]
        lines.append(" ".join([words[a], words[b], words[c], answer]))
    lines.insert(5, "the of zzz-not-a-word the")
    assert close <= LEFT_OUT_MAX * asked                     # the reference's own near-ties, capped first
    qfile = tmp_path / "questions.txt"
    qfile.write_text("\n".join(lines) + "\n")
    proc = subprocess.run([sys.executable, "-m", "trainer.analogy", "--job-dir", str(job), "--questions", str(qfile),
                           "--method", "3cosmul"], cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert not (job / "eval" / "analogy.json").exists()
    got = json.loads((job / "eval" / "analogy_3cosmul.json").read_text())
    want = cosmul_ref.score_file(str(qfile), vocab, W, eps=eps, global_step=60)
    assert [s["name"] for s in got["sections"]] == ["capital-test", "gram1-test"]
    assert got["sections"][0]["skipped"] == 1 and got["questions_total"] == 81 and got["questions_seen"] == 80
    for key in ("global_step", "embeddings", "top_k", "method", "epsilon", "questions_seen", "questions_total"):
        assert got[key] == want[key], key
    assert set(got) == set(want)
    for g, w in zip(got["sections"] + [got["semantic"], got["syntactic"], got["total"]],
                    want["sections"] + [want["semantic"], want["syntactic"], want["total"]]):
        assert (g["total"], g["skipped"]) == (w["total"], w["skipped"])
        assert abs(g["correct"] - w["correct"]) <= close
    assert sure >= 30 and got["total"]["correct"] >= sure - close      # the questions that ask for the reference's first answer
    assert "analogies, gram1-test" in proc.stderr
