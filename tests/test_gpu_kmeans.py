"""Spherical k-means on the GPU: glove_kmeans_assign_f32 / glove_kmeans_update_f32 of libglove_eval_hip.so and the driver
GloveHip.kmeans against the float64 reference of tests/kmeans_ref.py, and `python -m trainer.categorize` /
`python -m trainer.classes` end to end.

The shapes are the smallest at which the kernels can go wrong: one centroid and two; point counts that are no multiple of
the point tile (128) or of a sort tile (2048) and that cross several of both; K below, at and beyond a centroid tile
(128) up to the limit 4096; d below a k-slab (8), no multiple of it (52, 300) and the widest (1024); a cluster of many
chunks of 64, empty clusters and singletons.

Tolerances.  Cosines and centroids: rtol 1e-5, atol 1e-6, the project's figures for the similarity GEMM.  A point whose
float64 margin (best minus second-best score) is below 2.5e-5 — twice the tolerance at |cos| <= 1, rounded up — is
undecided: there the GPU may pick any centroid within 2.5e-5 of the best; everywhere else the assignment is exact.  The
float64 reference alone leaves at most 0.06 % of a case's points undecided at that threshold with the seeds below (the
(5000, 64, 5000, 129) case; 0.055 % at (20000, 64, 20000, 4096), none in the others); the cap, asserted first, is 0.5 %.
The widths here reach three of the seven row shapes; tests/test_gpu_factor_row_shapes.py runs assign and update at all of them."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import kmeans_ref
from helpers import to_dev

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
RTOL, ATOL, UNDECIDED, UNDECIDED_MAX = 1e-5, 1e-6, 2.5e-5, 0.005
CASES = [(300, 8, 300, 1), (300, 8, 257, 2), (1000, 52, 777, 33), (5000, 64, 5000, 129), (3000, 300, 2049, 1000),
         (600, 1024, 130, 31), (20000, 64, 20000, 4096)]


@functools.lru_cache(maxsize=None)
def case(V, d, n, K):
    """(W, ids, C, reference scores [n, K]): computed once, shared, never written to."""
    rng = np.random.default_rng(3000 + V + d + K)
    W = rng.standard_normal((V, d)).astype(np.float32)
    ids = (rng.permutation(V) if n == V else rng.integers(0, V, n)).astype(np.int32)
    C = (W[rng.choice(V, K, replace=False)] + 0.5 * rng.standard_normal((K, d))).astype(np.float32)
    S = kmeans_ref.scores(W, ids, C)
    for a in (W, ids, C, S):
        a.setflags(write=False)
    return W, ids, C, S


def check_assign(got_a, got_cos, S, what="", tied=()):
    """The parity checks of an assignment against the reference's score matrix S [n, K].  `tied`: points whose best
    score is shared on purpose (they are undecided by construction and stay out of the cap on the undecided share)."""
    got_a, got_cos = got_a.cpu().numpy(), got_cos.cpu().numpy()
    n, K = S.shape
    want_a = S.argmax(axis=1)
    best = S[np.arange(n), want_a]
    if K > 1:
        second = np.partition(S, K - 2, axis=1)[:, K - 2]
        undecided = best - second < UNDECIDED
    else:
        undecided = np.zeros(n, bool)
    print("%s: %.3f %% of the points undecided, largest cosine deviation %.3g"
          % (what, 100 * undecided.mean(), np.abs(got_cos - np.clip(best, -1, 1)).max()))
    assert np.delete(undecided, list(tied)).mean() <= UNDECIDED_MAX, what
    assert ((got_a >= 0) & (got_a < K)).all(), what
    np.testing.assert_allclose(got_cos, np.clip(best, -1.0, 1.0), rtol=RTOL, atol=ATOL, err_msg=what)
    assert (np.abs(got_cos) <= 1.0).all(), what
    assert (got_a[~undecided] == want_a[~undecided]).all(), (what, np.flatnonzero(~undecided & (got_a != want_a))[:5])
    assert (S[np.arange(n), got_a][undecided] >= best[undecided] - UNDECIDED).all(), what


@pytest.mark.parametrize("shape", CASES)
def test_assign_parity_with_the_float64_reference(hip, shape):
    V, d, n, K = shape
    W, ids, C, S = case(*shape)
    Wd, idsd, Cd = to_dev(W, ids, C)
    a, cos = hip.kmeans_assign(Wd, idsd, Cd)
    assert a.shape == cos.shape == (n,) and a.dtype == torch.int32 and cos.dtype == torch.float32
    check_assign(a, cos, S, "V=%d d=%d n=%d K=%d" % shape)
    again = hip.kmeans_assign(Wd, idsd, Cd)
    assert torch.equal(a, again[0]) and torch.equal(cos, again[1])               # bitwise repeatable
    if n >= 111:                                                                 # a point's result does not depend on its place
        part = hip.kmeans_assign(Wd, idsd[37:111].contiguous(), Cd)
        assert torch.equal(a[37:111], part[0]) and torch.equal(cos[37:111], part[1])


def test_assign_edge_rows(hip):
    V, d, n, K = 500, 52, 400, 150
    rng = np.random.default_rng(11)
    W = rng.standard_normal((V, d)).astype(np.float32)
    W[7] = 0.0                                               # a zero point row
    ids = rng.integers(0, V, n).astype(np.int32)
    ids[[0, 129, 399]] = 7
    ids[2], ids[4] = 11, 12
    C = (W[rng.choice(V, K, replace=False)] + 0.5 * rng.standard_normal((K, d))).astype(np.float32)
    C[3], C[19] = W[11], W[12]                               # the centroids of points 2 and 4, cosine 1 ...
    C[140] = C[3]                                            # ... and their bit-identical twins: in another tile,
    C[20] = C[19]                                            # and next to it
    C[77] = 0.0                                              # a zero centroid row
    a, cos = hip.kmeans_assign(*to_dev(W, ids, C))
    S = kmeans_ref.scores(W, ids, C)
    # tied on purpose: the zero rows, and every point closest to a centroid that has a twin
    check_assign(a, cos, S, "edge rows", tied=np.flatnonzero((ids == 7) | np.isin(S.argmax(axis=1), [3, 19])))
    a, cos = a.cpu().numpy(), cos.cpu().numpy()
    assert not np.isin(a, [140, 20]).any() and (a[2], a[4]) == (3, 19)           # the higher id never wins
    assert (a[[0, 129, 399]] == 0).all() and (cos[[0, 129, 399]] == 0.0).all()   # a zero row: cluster 0, cosine 0
    # a zero centroid scores 0: against centroids that are all further than a right angle away, it wins with cosine 0
    x = W[ids[1]]
    far = np.stack([-x, -x + 0.1 * rng.standard_normal(d).astype(np.float32), np.zeros(d, np.float32), -2 * x])
    a, cos = hip.kmeans_assign(*to_dev(W, ids[1:2].copy(), far))
    assert a.tolist() == [2] and cos.tolist() == [0.0]
    # everything a zero row: cluster 0
    a, cos = hip.kmeans_assign(*to_dev(np.zeros((4, 8), np.float32), np.array([0, 3, 3], np.int32), C[:5, :8].copy()))
    assert a.tolist() == [0, 0, 0] and cos.tolist() == [0.0, 0.0, 0.0]


def test_padded_row_stride(hip):
    V, dm, d, n, K = 300, 10, 12, 150, 9
    rng = np.random.default_rng(5)
    W = np.zeros((V, d), np.float32)
    W[:, :dm] = rng.standard_normal((V, dm))
    C = np.zeros((K, d), np.float32)
    C[:, :dm] = rng.standard_normal((K, dm))
    ids = rng.integers(0, V, n).astype(np.int32)
    Wd, idsd, Cd = to_dev(W, ids, C)
    a, cos = hip.kmeans_assign(Wd, idsd, Cd)
    check_assign(a, cos, kmeans_ref.scores(W[:, :dm], ids, C[:, :dm]), "padded stride")
    new, counts = hip.kmeans_update(Wd, idsd, a, Cd)
    want, want_counts = kmeans_ref.update(W[:, :dm], ids, a.cpu().numpy(), C[:, :dm])
    np.testing.assert_allclose(new.cpu().numpy()[:, :dm], want, rtol=RTOL, atol=ATOL)
    assert (new.cpu().numpy()[:, dm:] == 0.0).all() and counts.cpu().tolist() == want_counts.tolist()


# ---- update
def check_update(hip, W, ids, a, C, what=""):
    Wd, idsd, ad, Cd = to_dev(W, ids, a, C)
    new, counts = hip.kmeans_update(Wd, idsd, ad, Cd)
    assert new.shape == C.shape and counts.shape == (len(C),) and counts.dtype == torch.int32
    want, want_counts = kmeans_ref.update(W, ids, a, C)
    assert counts.cpu().tolist() == want_counts.tolist(), what                   # exact
    got = new.cpu().numpy()
    print("%s: largest centroid deviation %.3g" % (what, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)
    empty = want_counts == 0
    assert np.array_equal(got[empty].view(np.uint32), C[empty].view(np.uint32)), what        # bit for bit
    again = hip.kmeans_update(Wd, idsd, ad, Cd)
    assert torch.equal(new, again[0]) and torch.equal(counts, again[1])          # bitwise repeatable
    # seven more centroids that attract nothing: the first K rows keep their bits
    if len(C) + 7 <= 4096:
        more = torch.cat([Cd, Cd[:1].repeat(7, 1) * 2.0 + 1.0]).contiguous()
        wider = hip.kmeans_update(Wd, idsd, ad, more)
        assert torch.equal(wider[0][:len(C)], new) and torch.equal(wider[0][len(C):], more[len(C):])
        assert torch.equal(wider[1][:len(C)], counts) and (wider[1][len(C):] == 0).all()
    return got, want_counts


def test_update_a_cluster_of_many_chunks_empty_clusters_and_singletons(hip):
    V, d, n, K = 5000, 64, 5000, 40
    W, ids, _, _ = case(5000, 64, 5000, 129)
    rng = np.random.default_rng(12)
    C = rng.standard_normal((K, d)).astype(np.float32)
    a = rng.choice(np.arange(9, K), n).astype(np.int32)       # clusters 9 .. 39 share what is left
    spots = rng.permutation(n)
    a[spots[:3000]] = 0                                       # cluster 0: 3000 points, 47 chunks of 64
    for c in (1, 2, 3):                                       # three singletons
        a[spots[3000 + c]] = c
    for c in (4, 5, 6, 7, 8):                                 # five empty clusters
        assert not (a == c).any()
    got, counts = check_update(hip, W, ids, a, C, "many chunks")
    assert counts[0] == 3000 and counts[1:4].tolist() == [1, 1, 1] and (counts[4:9] == 0).all()
    for c in (1, 2, 3):
        np.testing.assert_allclose(got[c], kmeans_ref.unit_points(W, ids[spots[3000 + c]][None])[0], rtol=RTOL, atol=ATOL)


def test_update_with_the_assignment_of_the_assign_case(hip):
    shape = (3000, 300, 2049, 1000)
    W, ids, C, S = case(*shape)
    a, _ = hip.kmeans_assign(*to_dev(W, ids, C))
    check_update(hip, W, ids, a.cpu().numpy(), C, "V=%d d=%d n=%d K=%d" % shape)


def test_update_across_sort_tiles_and_summation_levels(hip):
    """20 000 points in 3 clusters: ten sort tiles, one cluster of 12 000 points (188 chunks, three summation levels)."""
    W, ids, _, _ = case(20000, 64, 20000, 4096)
    rng = np.random.default_rng(13)
    a = rng.choice(3, len(ids), p=[0.6, 0.3999, 0.0001]).astype(np.int32)
    C = rng.standard_normal((3, 64)).astype(np.float32)
    check_update(hip, W, ids, a, C, "three levels")
    a4096 = rng.integers(0, 4096, len(ids)).astype(np.int32)
    check_update(hip, W, ids, a4096, np.asarray(case(20000, 64, 20000, 4096)[2]), "K = 4096")


def test_empty_calls(hip):
    W, ids, C, _ = case(300, 8, 257, 2)
    Wd, idsd, Cd = to_dev(W, ids, C)
    a, cos = hip.kmeans_assign(Wd, idsd[:0], Cd)
    assert a.shape == (0,) and cos.shape == (0,)
    # n == 0: the library launches nothing and leaves its outputs as they are
    from trainer.hip_api import load_eval_library
    lib = load_eval_library()
    out = torch.full_like(Cd, 7.0)
    counts = torch.full((2,), 7, dtype=torch.int32, device="cuda:0")
    ws = hip.kmeans_workspace(0, 300, 8, 2, "cuda:0")
    rc = lib.glove_kmeans_update_f32(Wd.data_ptr(), 300, 8, idsd.data_ptr(), 0, a.data_ptr(), Cd.data_ptr(), 2, out.data_ptr(),
                                     counts.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and (out == 7.0).all() and (counts == 7).all()
    # the binding answers for it: every cluster is empty
    new, counts = hip.kmeans_update(Wd, idsd[:0], a, Cd)
    assert torch.equal(new, Cd) and counts.tolist() == [0, 0]
    from trainer.hip_api import GloveHipError
    with pytest.raises(GloveHipError):
        hip.kmeans_assign(Wd, idsd.long(), Cd)
    with pytest.raises(GloveHipError):
        hip.kmeans_assign(Wd, idsd, Cd[:, :4].contiguous())
    with pytest.raises(GloveHipError):
        hip.kmeans_update(Wd, idsd, a, Cd)                   # assign [0] for 257 points


# ---- the driver
def own_loop(hip, Wd, idsd, init, iterations):
    """The driver's loop from kmeans_assign and kmeans_update; also every pass's objective."""
    cents, previous, t, trace = init, None, 0, []
    while True:
        t += 1
        a, cos = hip.kmeans_assign(Wd, idsd, cents)
        trace.append(float(cos.cpu().numpy().astype(np.float64).sum()))
        converged = previous is not None and torch.equal(a, previous)
        if converged or t == iterations:
            return a, cos, cents, t, converged, trace
        cents, _ = hip.kmeans_update(Wd, idsd, a, cents)
        previous = a


@pytest.mark.parametrize("iterations", [1, 4, 100])
def test_driver_equals_a_loop_of_assign_and_update(hip, iterations):
    W, ids, C, _ = case(1000, 52, 777, 33)
    Wd, idsd, Cd = to_dev(W, ids, C)
    res = hip.kmeans(Wd, idsd, 33, iterations=iterations, init=Cd)
    a, cos, cents, t, converged, trace = own_loop(hip, Wd, idsd, Cd, iterations)
    assert torch.equal(res.assign, a) and torch.equal(res.cos, cos) and torch.equal(res.centroids, cents)
    assert (res.iterations, res.converged) == (t, converged) and res.objective == trace[-1] == res.objectives[0]
    assert t <= iterations and (converged or t == iterations) and (iterations > 1 or not converged)
    drops = [x - y for x, y in zip(trace, trace[1:])]
    print("objective per pass:", trace)
    assert all(x <= 1e-6 * len(ids) for x in drops)          # J never drops by more than 1e-6 n


def test_planted_partition_is_recovered_exactly(hip):
    W, gold, init = kmeans_ref.planted()
    ids = np.arange(len(W), dtype=np.int32)
    res = hip.kmeans(*to_dev(W, ids), 24, init=to_dev(init)[0])
    assert res.converged and res.iterations <= 3
    assert kmeans_ref.purity(res.assign.cpu().numpy(), gold.tolist()) == 1.0
    assert res.assign.cpu().tolist() == gold.tolist()         # init row c is a member of centre c
    want = kmeans_ref.kmeans(W, ids, 24, init=init)
    assert res.assign.cpu().tolist() == want.assign.tolist() and res.iterations == want.iterations
    np.testing.assert_allclose(res.cos.cpu().numpy(), want.cos, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(res.centroids.cpu().numpy(), want.centroids, rtol=RTOL, atol=ATOL)


def test_seeded_runs_repeat_and_the_best_restart_wins(hip):
    W, ids, _, _ = case(1000, 52, 777, 33)
    Wd, idsd = to_dev(W, ids)
    one = hip.kmeans(Wd, idsd, 12, seed=3, restarts=4, iterations=6)
    two = hip.kmeans(Wd, idsd, 12, seed=3, restarts=4, iterations=6)
    for x, y in zip(one[:3], two[:3]):
        assert torch.equal(x, y)
    assert one[3:6] == two[3:6] and one.objectives == two.objectives
    assert len(one.objectives) == len(one.assignments) == 4
    best = int(np.argmax(one.objectives))                     # the first of equal objectives
    assert one.objective == one.objectives[best] and torch.equal(one.assign, one.assignments[best])
    # run r starts from the sorted rows numpy draws for [seed, r]
    rows = kmeans_ref.initial_rows(len(ids), 12, 3, best)
    X = Wd[idsd[torch.from_numpy(rows).cuda()].long()]
    init = (X * torch.rsqrt(torch.clamp((X * X).sum(dim=1, keepdim=True), min=1e-12))).contiguous()
    alone = hip.kmeans(Wd, idsd, 12, iterations=6, init=init)
    assert torch.equal(alone.assign, one.assign) and torch.equal(alone.centroids, one.centroids)
    other = hip.kmeans(Wd, idsd, 12, seed=4, restarts=1, iterations=6)
    assert not torch.equal(other.assign, one.assignments[0])
    from trainer.hip_api import GloveHipError
    with pytest.raises(GloveHipError):
        hip.kmeans(Wd, idsd, 778)
    with pytest.raises(GloveHipError):
        hip.kmeans(Wd, idsd, 12, iterations=0)


def test_captured_iteration_replays_like_the_eager_one(hip):
    shape = (5000, 64, 5000, 129)
    W, ids, C, _ = case(*shape)
    Wd, idsd, Cd = to_dev(W, ids, C)
    ws = hip.kmeans_workspace(5000, 5000, 64, 129, "cuda:0")
    a0, cos0 = hip.kmeans_assign(Wd, idsd, Cd, ws)
    new0, counts0 = hip.kmeans_update(Wd, idsd, a0, Cd, ws)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm the launch paths outside the capture
        hip.kmeans_update(Wd, idsd, hip.kmeans_assign(Wd, idsd, Cd, ws)[0], Cd, ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a, cos = hip.kmeans_assign(Wd, idsd, Cd, ws)
        new, counts = hip.kmeans_update(Wd, idsd, a, Cd, ws)
    a.fill_(-7); cos.fill_(float("nan")); new.fill_(float("nan")); counts.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, a0) and torch.equal(cos, cos0) and torch.equal(new, new0) and torch.equal(counts, counts0)


# ---- end to end
def test_cli_end_to_end(hip, tmp_path):
    """Train a tiny job, run `python -m trainer.categorize` and `python -m trainer.classes` (child processes) on it, and
    compare what they write with the bookkeeping of the reference and with GloveHip.kmeans in this process."""
    from trainer import estimator
    from trainer.hip_api import row_width
    csv, vocab_txt = GOLDEN / "text8_cov90_ctx5_interaction.csv", GOLDEN / "text8_cov90_ctx5_vocab.txt"
    job = tmp_path / "job"
    estimator.main(["--train-csv", str(csv), "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path",
                    "--embedding-size", "50", "--optimizer", "Adagrad", "--learning-rate", "0.05", "--batch-size", "64",
                    "--train-steps", "60", "--log-every", "20", "--seed", "7", "--skip-eval"])
    blob = torch.load(job / "model.ckpt-60.pt", weights_only=False)["tables"]
    vocab = vocab_txt.read_text().split("\n")
    Wd = torch.zeros(len(vocab), row_width(len(vocab), 50), device="cuda:0")
    Wd[:, :50] = (blob["R"] + blob["C"]).to("cuda:0")[:, :50]
    words = [w for w in vocab if w != "<UNK>"]
    rng = np.random.default_rng(9)
    chosen = [words[i] for i in rng.choice(len(words), 30, replace=False)]
    lines = ["# word category"] + ["%s cat%d" % (w.upper() if i % 7 == 0 else w, i % 5) for i, w in enumerate(chosen)]
    lines.insert(4, "zzz-not-a-word cat1")
    lines.insert(9, "<UNK> cat2")
    lines.insert(20, "%s cat4" % chosen[0])                  # a duplicate, under another category
    lines.insert(25, "")
    cfile = tmp_path / "categories.txt"
    cfile.write_text("\n".join(lines) + "\n")
    proc = subprocess.run([sys.executable, "-m", "trainer.categorize", "--job-dir", str(job), "--categories", str(cfile),
                           "--embeddings", "sum", "--restarts", "3"], cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    got = json.loads((job / "eval" / "categorization.json").read_text())
    pairs = kmeans_ref.parse(str(cfile))
    ids, gold, skipped, duplicates = kmeans_ref.lookup(pairs, vocab)
    assert (got["words_total"], got["words_seen"], got["skipped"], got["duplicates"]) == (33, 30, 2, 1) \
        == (len(pairs), len(ids), skipped, duplicates)
    assert (got["categories"], got["clusters"], got["restarts"], got["seed"]) == (5, 5, 3, 0)
    assert (got["global_step"], got["embeddings"], got["categories_file"]) == (60, "sum", "categories.txt")
    res = hip.kmeans(Wd, torch.tensor(ids, dtype=torch.int32, device="cuda:0"), 5, seed=0, restarts=3, iterations=100)
    assert got["purity"] == kmeans_ref.purity(res.assign.cpu().numpy(), gold)
    purities = [kmeans_ref.purity(a.cpu().numpy(), gold) for a in res.assignments]
    assert (got["purity_min"], got["purity_max"]) == (min(purities), max(purities)) and got["purity_mean"] == pytest.approx(np.mean(purities))
    assert (got["iterations"], got["converged"], got["objective"]) == (res.iterations, res.converged, res.objective)
    assert got["sizes"] == np.bincount(res.assign.cpu().numpy(), minlength=5).tolist() and sum(got["sizes"]) == 30
    assert "categorization, categories.txt" in proc.stderr

    proc = subprocess.run([sys.executable, "-m", "trainer.classes", "--job-dir", str(job), "--classes", "8", "--embeddings", "sum"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    out = [line.split(" ") for line in (job / "classes.txt").read_text().split("\n")[:-1]]
    assert [t for t, _ in out] == words                       # vocabulary order, <UNK> left out
    classes = [int(c) for _, c in out]
    assert all(0 <= c < 8 for c in classes)
    all_ids = torch.tensor([i for i, w in enumerate(vocab) if w != "<UNK>"], dtype=torch.int32, device="cuda:0")
    res = hip.kmeans(Wd, all_ids, 8, seed=0, restarts=1, iterations=10)
    assert classes == res.assign.cpu().tolist()
    rec = json.loads((job / "eval" / "classes.json").read_text())
    sizes = np.bincount(classes, minlength=8)
    assert rec == {"global_step": 60, "embeddings": "sum", "words": len(words), "classes": 8, "iterations": res.iterations,
                   "converged": res.converged, "objective": res.objective, "empty": int((sizes == 0).sum()),
                   "largest": int(sizes.max()), "smallest": int(sizes.min())}
