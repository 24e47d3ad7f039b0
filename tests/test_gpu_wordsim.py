"""The pair cosine on the GPU: glove_pair_cosine_f32 of libglove_eval_hip.so against the float64 reference of
tests/cosmul_ref.py, and `python -m trainer.wordsim` end to end against tests/wordsim_ref.py.

Tolerance of a cosine: rtol 1e-5, atol 1e-6, the figures of the similarity GEMM's tests; the same formula in float32
NumPy deviates from float64 by 2.4e-7 at most on these tables, the kernel on an MI355X by 1.2e-7."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cosmul_ref
import wordsim_ref
from helpers import to_dev
from test_gpu_analogy import CASES

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
RTOL, ATOL = 1e-5, 1e-6
TABLES = sorted({(V, d) for V, d, _, _ in CASES})


def pairs_case(V, d, n=300):
    rng = np.random.default_rng(2000 + V + d)
    W = rng.standard_normal((V, d)).astype(np.float32)
    zero = V // 2
    W[zero] = 0.0
    pairs = rng.integers(0, V, (n, 2)).astype(np.int32)
    edges = [e for e in (0, 127, 128, V - 1) if e < V]
    for i, e in enumerate(edges):
        pairs[2 * i] = (e, e)                                # i == j
        pairs[2 * i + 1] = (e, int(rng.integers(V)))
    pairs[20], pairs[21], pairs[22] = (zero, 3), (5, zero), (zero, zero)
    return W, pairs, edges


@pytest.mark.parametrize("V,d", TABLES)
def test_pair_cosine_parity_with_the_float64_reference(hip, V, d):
    W, pairs, edges = pairs_case(V, d)
    Wd, pd = to_dev(W, pairs)
    got = hip.pair_cosine(Wd, pd)
    assert got.shape == (300,) and got.dtype == torch.float32
    want = cosmul_ref.pair_cosine(W, pairs)
    g = got.cpu().numpy()
    print("V=%d d=%d: largest deviation %.3g" % (V, d, np.abs(g - want).max()))
    np.testing.assert_allclose(g, want, rtol=RTOL, atol=ATOL)
    assert (np.abs(g) <= 1.0).all()                          # the clamp
    np.testing.assert_allclose(g[0:2 * len(edges):2], 1.0, rtol=RTOL, atol=ATOL)    # i == j
    assert (g[20:23] == 0.0).all()                           # a zero row: the clamped norm, cosine 0
    assert torch.equal(got, hip.pair_cosine(Wd, pd))         # bitwise repeatable
    # whatever the grid: a pair's cosine does not depend on its place in the call
    assert torch.equal(got[37:111], hip.pair_cosine(Wd, pd[37:111].contiguous()))


def test_padded_row_stride_and_empty_call(hip):
    V, dm, d = 300, 10, 12
    rng = np.random.default_rng(5)
    W = np.zeros((V, d), np.float32)
    W[:, :dm] = rng.standard_normal((V, dm))
    pairs = rng.integers(0, V, (150, 2)).astype(np.int32)
    Wd, pd = to_dev(W, pairs)
    np.testing.assert_allclose(hip.pair_cosine(Wd, pd).cpu().numpy(), cosmul_ref.pair_cosine(W[:, :dm], pairs), rtol=RTOL, atol=ATOL)
    assert hip.pair_cosine(Wd, pd[:0]).shape == (0,)
    from trainer.hip_api import GloveHipError
    with pytest.raises(GloveHipError):
        hip.pair_cosine(Wd, pd.long())
    with pytest.raises(GloveHipError):
        hip.pair_cosine(Wd, pd[:, :1])


def test_cli_end_to_end(hip, tmp_path):
    """Train a tiny job, ask `python -m trainer.wordsim` (a child process) about a pairs file made from its vocabulary,
    and compare wordsim.json with the reference on the checkpoint's tables."""
    from trainer import estimator
    csv, vocab_txt = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    job = tmp_path / "job"
    estimator.main(["--train-csv", str(csv), "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path",
                    "--embedding-size", "50", "--optimizer", "Adagrad", "--learning-rate", "0.05", "--batch-size", "64",
                    "--train-steps", "60", "--log-every", "20", "--seed", "7", "--skip-eval"])
    blob = torch.load(job / "model.ckpt-60.pt", weights_only=False)["tables"]
    W = (blob["R"] + blob["C"]).numpy()
    vocab = vocab_txt.read_text().split("\n")
    words = [w for w in vocab if w != "<UNK>"]
    rng = np.random.default_rng(10)
    every = [(i, j) for i in range(len(words)) for j in range(i + 1, len(words))]      # (the vocabulary is small: no pair twice)
    assert len(every) >= 200
    ids = np.array([every[p] for p in rng.choice(len(every), 200, replace=False)])
    ids = np.array([[vocab.index(words[i]), vocab.index(words[j])] for i, j in ids])
    cos = cosmul_ref.pair_cosine(W, ids)
    # pairs whose reference cosine lies within 1e-5 of another pair's are left out of the file: the ranks of the float32
    # cosines are then those of the float64 ones
    order = np.argsort(cos)
    near = np.zeros(len(cos), bool)
    tight = np.diff(cos[order]) < 1e-5
    near[order[:-1]] |= tight
    near[order[1:]] |= tight
    ids, cos = ids[~near], cos[~near]
    assert len(ids) >= 150
    # a noisy function of the cosine (noise of half the signal's spread), rounded: with ties
    human = np.round(5 + 4 * cos + 2 * cos.std() * rng.standard_normal(len(cos)), 2)
    lines = ["word1\tword2\thuman"] + ["%s\t%s\t%.2f" % (vocab[i], vocab[j], h) for (i, j), h in zip(ids.tolist(), human)]
    lines.insert(3, "the\tzzz-not-a-word\t5.0")
    lines.insert(7, "<UNK>\tthe\t2.0")
    lines.insert(9, "# a comment")
    pfile = tmp_path / "pairs.tab"
    pfile.write_text("\n".join(lines) + "\n")
    proc = subprocess.run([sys.executable, "-m", "trainer.wordsim", "--job-dir", str(job), "--pairs", str(pfile),
                           "--embeddings", "sum"], cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    got = json.loads((job / "eval" / "wordsim.json").read_text())
    want = wordsim_ref.score_file(str(pfile), vocab, W, embeddings="sum", global_step=60)
    assert set(got) == set(want)
    for key in ("global_step", "embeddings", "pairs_file", "pairs_total", "pairs_seen", "skipped"):
        assert got[key] == want[key], key
    assert (got["pairs_total"], got["pairs_seen"], got["skipped"]) == (len(ids) + 2, len(ids), 2)
    print("spearman %.9f (reference %.9f), pearson %.9f (reference %.9f)" % (got["spearman"], want["spearman"], got["pearson"], want["pearson"]))
    assert abs(got["spearman"] - want["spearman"]) <= 1e-6 and abs(got["pearson"] - want["pearson"]) <= 1e-6
    assert 0.5 < got["spearman"] < 1.0                       # the human scores follow the cosines, noisily
    assert "word similarity, pairs.tab" in proc.stderr
