"""trainer.align on the CPU: the ABI of include/glove_eval_cross_hip.h and include/glove_factor_align_hip.h (the surface,
the size queries, every refusal the host makes before a launch), then the driver (orthogonal Procrustes, CSLS retrieval,
refinement) and the two command lines with the NumPy backend of tests/align_ref.py.  The kernels themselves:
tests/test_gpu_align.py."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import align_ref as ref
from trainer import align
from trainer.align import align_tables, read_dictionary, shared_vocab_pairs, translation_precision

REPO = Path(__file__).resolve().parent.parent
CROSS_HEADER = REPO / "include" / "glove_eval_cross_hip.h"
ALIGN_HEADER = REPO / "include" / "glove_factor_align_hip.h"
BAD, WS = -1, -2
BIG = 1 << 40


# ---- 1. the ABI
@pytest.fixture(scope="module")
def libs():
    from trainer import hip_api
    if not hip_api.FACTOR_LIB_PATH.exists() or not hip_api.EVAL_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_eval_library(), hip_api.load_factor_library()


def declared_functions(header):
    """name -> number of parameters of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return {name: 0 if args.strip() == "void" else args.count(",") + 1
            for name, args in re.findall(r"\b(glove_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_headers_and_the_binding_declare_the_same_functions(libs):
    from trainer import hip_api
    ev, fa = libs
    for header, protos, symbols, lib, want in (
            (CROSS_HEADER, hip_api.eval_cross_prototypes(), hip_api.EVAL_CROSS_EXPORTED_SYMBOLS, ev,
             {"glove_eval_cross_abi_version", "glove_cross_topk_workspace_bytes", "glove_cross_topk_f32", "glove_topk_mean_f32"}),
            (ALIGN_HEADER, hip_api.factor_align_prototypes(), hip_api.FACTOR_ALIGN_EXPORTED_SYMBOLS, fa,
             {"glove_factor_align_abi_version", "glove_cross_gram_workspace_bytes", "glove_cross_gram_f64"})):
        declared = declared_functions(header)
        assert set(declared) == set(protos) == set(symbols) == want
        assert declared == {name: len(args) for name, (_, args) in protos.items()}
        for name in declared:
            assert hasattr(lib, name), name
    others = (hip_api.EXPORTED_SYMBOLS + hip_api.EVAL_EXPORTED_SYMBOLS + hip_api.EVAL_SIM_EXPORTED_SYMBOLS
              + hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS + hip_api.PREP_EXPORTED_SYMBOLS + hip_api.TEXT_EXPORTED_SYMBOLS
              + hip_api.VECTORS_EXPORTED_SYMBOLS + hip_api.COOC_OPTIONS_EXPORTED_SYMBOLS + hip_api.PHRASES_EXPORTED_SYMBOLS
              + hip_api.FACTOR_EXPORTED_SYMBOLS + hip_api.FACTOR_DENSE_EXPORTED_SYMBOLS + hip_api.FACTOR_GRAPH_EXPORTED_SYMBOLS)
    assert not (set(hip_api.EVAL_CROSS_EXPORTED_SYMBOLS) | set(hip_api.FACTOR_ALIGN_EXPORTED_SYMBOLS)) & set(others)
    assert not set(hip_api.EVAL_CROSS_EXPORTED_SYMBOLS) & set(hip_api.FACTOR_ALIGN_EXPORTED_SYMBOLS)


def test_the_new_versions_are_1_and_the_older_ones_unchanged(libs):
    from trainer import hip_api
    ev, fa = libs
    assert ev.glove_eval_cross_abi_version() == hip_api.GLOVE_EVAL_CROSS_ABI_VERSION == 1
    assert fa.glove_factor_align_abi_version() == hip_api.GLOVE_FACTOR_ALIGN_ABI_VERSION == 1
    assert "#define GLOVE_EVAL_CROSS_ABI_VERSION 1" in CROSS_HEADER.read_text()
    assert "#define GLOVE_FACTOR_ALIGN_ABI_VERSION 1" in ALIGN_HEADER.read_text()
    assert (ev.glove_eval_abi_version(), ev.glove_eval_sim_abi_version(), ev.glove_eval_cluster_abi_version()) == (1, 1, 1)
    assert (fa.glove_factor_abi_version(), fa.glove_factor_dense_abi_version(), fa.glove_factor_graph_abi_version()) == (1, 1, 1)
    for name, macro in (("glove_eval_hip.h", "GLOVE_EVAL_ABI_VERSION"), ("glove_eval_sim_hip.h", "GLOVE_EVAL_SIM_ABI_VERSION"),
                        ("glove_eval_cluster_hip.h", "GLOVE_EVAL_CLUSTER_ABI_VERSION"), ("glove_factor_hip.h", "GLOVE_FACTOR_ABI_VERSION"),
                        ("glove_factor_dense_hip.h", "GLOVE_FACTOR_DENSE_ABI_VERSION"),
                        ("glove_factor_graph_hip.h", "GLOVE_FACTOR_GRAPH_ABI_VERSION")):
        assert "#define %s 1" % macro in (REPO / "include" / name).read_text()
    # the chunk and the slice are the dense header's: the new one includes it and defines neither
    text = ALIGN_HEADER.read_text()
    assert '#include "glove_factor_dense_hip.h"' in text and "#define GLOVE_GRAM_CHUNK" not in text


def up256(nbytes):
    return (nbytes + 255) // 256 * 256


def test_the_size_queries_are_pure_host_functions(libs):
    from trainer.hip_api import GRAM_SLICE as S
    ev, fa = libs
    q = fa.glove_cross_gram_workspace_bytes
    assert q(1, 4) == 256                                    # one slot of 16 doubles: never less than 256 B
    for n, d in ((1, 304), (S, 304), (S + 1, 304), (2 * S + 7, 64), (200000, 304), (2 ** 31 - 1, 1024)):
        assert q(n, d) == max(256, up256(math.ceil(n / S) * d * d * 8)), (n, d)
        assert q(n, d) == fa.glove_gram_workspace_bytes(n, d)
    for n, d in ((0, 8), (-1, 8), (2 ** 31, 8), (10, 0), (10, 6), (10, 1028), (10, -4), (10, 2)):
        assert q(n, d) == 0, (n, d)
    q = ev.glove_cross_topk_workspace_bytes
    for n, Vt, d, k in ((1, 1, 4, 1), (40, 64, 8, 5), (129, 129, 36, 10), (257, 4097, 64, 10), (130, 40003, 52, 20), (0, 64, 8, 5),
                        (1024, 200000, 304, 10)):
        segs = math.ceil(Vt / 4096)                          # the winners the first top-k stage leaves: values and ids, twice
        want = up256(4 * n) + up256(4 * Vt) + up256(4 * n * Vt) + 2 * (up256(4 * n * segs * k) + up256(4 * n * segs * k))
        assert q(n, Vt, d, k) == want, (n, Vt, d, k)
    for n, Vt, d, k in ((-1, 64, 8, 5), (65535 * 128 + 1, 64, 8, 5), (4, 0, 8, 1), (4, 64, 0, 5), (4, 64, 6, 5), (4, 64, 1028, 5),
                        (4, 64, 8, 0), (4, 64, 8, 65), (4, 4096, 8, 1025)):
        assert q(n, Vt, d, k) == 0, (n, Vt, d, k)
    assert q(4, 4096, 8, 1024) > 0 and q(65535 * 128, 1, 4, 1) > 0


def test_argument_errors_come_back_before_any_launch(libs):
    """Null pointers, sizes out of range, a short workspace, one penalty array without the other: the answer is a
    GLOVE_E_* code, nothing is enqueued (no device is needed; 16, 32, ... stand for pointers nothing dereferences)."""
    ev, fa = libs
    topk, mean, gram = ev.glove_cross_topk_f32, ev.glove_topk_mean_f32, fa.glove_cross_gram_f64
    good = dict(Q=16, Vq=9, qid=32, n=4, T=48, Vt=64, d=8, k=5, q_pen=None, t_pen=None, sims=64, idx=80, ws=96, ws_bytes=BIG)

    def call(**change):
        a = dict(good, **change)
        return topk(a["Q"], a["Vq"], a["qid"], a["n"], a["T"], a["Vt"], a["d"], a["k"], a["q_pen"], a["t_pen"], a["sims"],
                    a["idx"], a["ws"], a["ws_bytes"], None)
    for name in ("Q", "qid", "T", "sims", "idx", "ws"):
        assert call(**{name: None}) == BAD, name
    for change in (dict(d=6), dict(d=0), dict(d=1028), dict(k=0), dict(k=65), dict(Vt=4096, k=1025), dict(n=-1),
                   dict(n=65535 * 128 + 1), dict(Vt=0), dict(Vq=0), dict(q_pen=112), dict(t_pen=112)):
        assert call(**change) == BAD, change
    assert call(ws_bytes=ev.glove_cross_topk_workspace_bytes(4, 64, 8, 5) - 1) == WS
    # n == 0 returns 0 without a launch, whatever the pointers — but after the size checks
    assert call(n=0, Q=None, qid=None, T=None, sims=None, idx=None, ws=None, ws_bytes=0) == 0
    assert call(n=0, d=6) == BAD and call(n=0, k=65) == BAD and call(n=0, q_pen=112) == BAD
    assert mean(None, 4, 5, 16, None) == BAD and mean(16, 4, 5, None, None) == BAD
    assert mean(16, -1, 5, 32, None) == BAD and mean(16, 4, 0, 32, None) == BAD
    assert mean(None, 0, 5, None, None) == 0

    good = dict(X=16, Vx=7, Y=32, Vy=9, d=8, xid=48, yid=64, n=10, M=80, ws=96, ws_bytes=BIG)

    def call(**change):
        a = dict(good, **change)
        return gram(a["X"], a["Vx"], a["Y"], a["Vy"], a["d"], a["xid"], a["yid"], a["n"], None, None, a["M"], a["ws"],
                    a["ws_bytes"], None)
    for name in ("X", "Y", "xid", "yid", "M", "ws"):
        assert call(**{name: None}) == BAD, name
    for change in (dict(n=0), dict(n=2 ** 31), dict(d=6), dict(d=0), dict(d=1028), dict(Vx=0), dict(Vy=0)):
        assert call(**change) == BAD, change
    assert call(ws_bytes=255) == WS and call(n=20000, ws_bytes=2 * 8 * 8 * 8 - 1) == WS


def test_missing_libraries_are_an_error_not_a_fallback(tmp_path):
    from trainer import hip_api
    with pytest.raises(hip_api.GloveHipError, match="no CPU fallback"):
        hip_api.load_eval_library(tmp_path / "libglove_eval_hip.so")


# ---- 2. the driver on planted cases (the NumPy backend)
def identity_pairs(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)


def test_a_planted_rotation_is_recovered():
    X, Y, Q = ref.planted_rotation()                         # V = 500, d = 20
    out = align_tables(X, Y, identity_pairs(200), backend=ref.NumpyBackend())
    W = out["W"]
    # float64 rounding level: the singular vectors of a 20 x 20 matrix of condition number below 2 (200 unit-length anchors
    # of an isotropic cloud) come back to a few d u, u = 2^-53; 1e-13 leaves two orders of magnitude
    assert W.dtype == np.float64 and np.abs(W - Q).max() <= 1e-13
    assert out["orthogonality_defect"] <= 1e-13
    assert np.abs(out["Y"] - Y).max() <= 1e-12 and out["Y"].shape == (500, 20)
    assert abs(out["anchor_cosine_after"] - 1.0) <= 1e-13 and out["anchor_cosine_before"] < 0.5
    assert out["singular_values"].shape == (20,) and (np.diff(out["singular_values"]) <= 0).all()
    assert out["dictionary_sizes"] == [] and {"cross_gram", "svd", "rows_transform"} <= set(out["seconds"])
    # W is the map of the definitions, spelled out without the driver
    assert np.abs(W - ref.procrustes_map(X, np.arange(200), Y, np.arange(200))).max() <= 1e-13
    # anchors in any order and repeated: the same map
    rng = np.random.default_rng(1)
    ids = rng.choice(200, 300)
    again = align_tables(X, Y, np.stack([ids, ids], axis=1), backend=ref.NumpyBackend())
    assert np.abs(again["W"] - Q).max() <= 1e-13


@pytest.mark.parametrize("normalize", align.NORMALIZE)
def test_with_noise_the_map_stays_orthogonal_and_the_anchors_come_closer(normalize):
    X, Y, Q = ref.planted_rotation(seed=2, noise=0.3)
    out = align_tables(X, Y, identity_pairs(200), normalize=normalize, backend=ref.NumpyBackend())
    assert out["orthogonality_defect"] <= 1e-13
    assert 0.01 < np.abs(out["W"] - Q).max() < 0.2           # near the planted rotation, not on it
    if normalize == "unit":                                  # what this W maximises over the orthogonal maps is that mean
        assert out["anchor_cosine_after"] >= out["anchor_cosine_before"]
        a = X[:200] * ref.inv_norms(X[:200])[:, None]
        b = Y[:200] * ref.inv_norms(Y[:200])[:, None]
        want = ((a @ out["W"].T) * b).sum(axis=1).mean()
        assert abs(out["anchor_cosine_after"] - want) <= 1e-12
        assert want >= ((a @ Q.T) * b).sum(axis=1).mean() - 1e-12      # no worse than the planted rotation itself
    # the source rows are mapped unscaled
    assert np.abs(out["Y"] - X @ out["W"].T).max() <= 1e-12


def test_the_float32_backend_stays_at_float32_rounding():
    """The figure the GPU test's bound is built from (the device is allowed 8 times it)."""
    X, Y, _ = ref.planted_rotation(noise=0.1)
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    f64 = align_tables(X, Y, identity_pairs(200), backend=ref.NumpyBackend())
    f32 = align_tables(X, Y, identity_pairs(200), backend=ref.NumpyBackend(float32=True))
    assert f32["W"].dtype == np.float32 and f32["Y"].dtype == np.float32
    e = np.abs(f32["W"] - f64["W"]).max()
    print("NumPy float32 from float64: W %.3g" % e)
    assert 0 < e <= 64 * 2.0 ** -24                          # entries below 1, a well-conditioned M
    assert f32["orthogonality_defect"] <= 64 * 2.0 ** -24


def test_driver_refusals():
    X, Y, _ = ref.planted_rotation(V=50, d=8)
    be = ref.NumpyBackend()
    with pytest.raises(ValueError, match="embedding size"):
        align_tables(X, Y[:, :4], identity_pairs(10), backend=be)
    with pytest.raises(ValueError, match="fewer than one anchor"):
        align_tables(X, Y, np.zeros((0, 2), np.int32), backend=be)
    with pytest.raises(ValueError, match="outside"):
        align_tables(X, Y, [[0, 50]], backend=be)
    for settings in (dict(normalize="l1"), dict(refine=-1), dict(refine_vocab=0), dict(knn=0), dict(refine=1, knn=51)):
        with pytest.raises(ValueError):
            align_tables(X, Y, identity_pairs(10), backend=be, **settings)
    with pytest.raises(ValueError):
        translation_precision(X, Y, identity_pairs(10), method="mnn", backend=be)
    with pytest.raises(ValueError):
        translation_precision(X, Y, identity_pairs(10), top_k=(0,), backend=be)
    with pytest.raises(ValueError):
        translation_precision(X, Y, identity_pairs(10), top_k=(51,), backend=be)
    with pytest.raises(ValueError):
        translation_precision(X, Y, np.zeros((0, 2), np.int32), backend=be)


# ---- 3. the dictionary and the scoring
def test_the_dictionary_reader_skips_counts_and_keeps_the_file_order(tmp_path):
    src = ["<UNK>", "cat", "dog", "house", "dog"]            # the second `dog` is never an id
    tgt = ["chat", "chien", "maison", "<UNK>", "matou"]
    f = tmp_path / "en-fr.txt"
    f.write_text("dog chien\ncat\tchat\n\ncat matou\nbird oiseau\ndog chien\nhouse   maison\ncat oiseau\n<UNK> chat\ncat <UNK>\n")
    pairs, counts = read_dictionary(f, src, tgt)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[2, 1], [1, 0], [1, 4], [3, 2]]
    assert counts == {"lines": 9, "pairs": 4, "skipped": 4, "duplicates": 1}
    pairs, counts = read_dictionary(f, src, tgt, target_limit=3)        # matou lies beyond the candidates
    assert pairs.tolist() == [[2, 1], [1, 0], [3, 2]] and counts["skipped"] == 5
    f.write_text("dog chien le\n")
    with pytest.raises(ValueError, match="line 1"):
        read_dictionary(f, src, tgt)
    pairs, counts = shared_vocab_pairs(["a", "<UNK>", "b", "c", "d"], ["d", "b", "<UNK>", "a"])
    assert pairs.tolist() == [[0, 3], [2, 1], [4, 0]] and counts["shared"] == 3
    assert shared_vocab_pairs(["a", "b", "c", "d"], ["d", "b", "a"], anchors=2)[0].tolist() == [[0, 2], [1, 1]]


def test_precision_at_k_with_several_gold_targets():
    """Targets on a circle, queries just beside some of them: the ranking of every query is known by construction."""
    ang = np.deg2rad(np.arange(12) * 30.0)
    T = np.stack([np.cos(ang), np.sin(ang), np.zeros(12), np.zeros(12)], axis=1)
    q_ang = np.deg2rad(np.array([1.0, 91.0, 181.0, 271.0]))      # nearest: 0, 3, 6, 9; then 1, 4, 7, 10; then 11, 2, 5, 8
    A = np.stack([np.cos(q_ang), np.sin(q_ang), np.zeros(4), np.zeros(4)], axis=1) * np.array([[1.0], [2.0], [0.5], [3.0]])
    pairs = [[0, 0],                 # hit at 1
             [1, 4], [1, 7],         # two gold targets, the better one second: hit at 2
             [2, 5], [2, 0],         # 5 is third (6, 7, 5, 8): hit at 3
             [3, 3], [3, 0]]         # never among the first four (9, 10, 8, 11)
    out = translation_precision(A, T, pairs, method="nn", top_k=(1, 2, 3, 4), backend=ref.NumpyBackend())
    assert out["precision"] == {1: 0.25, 2: 0.5, 3: 0.75, 4: 0.75} and (out["queries"], out["pairs"]) == (4, 7)
    assert out["precision"] == ref.precision_at(A, T, pairs, (1, 2, 3, 4), "nn")


def test_csls_answers_the_partner_where_nearest_neighbours_answer_the_hub():
    A, T, pairs = ref.hub_case()
    hub = len(T) - 1
    # the reference itself first: the case is one where CSLS helps
    nn, csls = ref.precision_at(A, T, pairs, (1,), "nn"), ref.precision_at(A, T, pairs, (1,), "csls", knn=10)
    assert csls[1] >= 0.9 > 0.1 >= nn[1]
    nn_top = ref.topk(A, np.arange(len(A)), T, 1)[1][:, 0]
    assert (nn_top == hub).mean() >= 0.9                     # nearest neighbours: the hub, for most queries
    pens = ref.csls_penalty(A, np.arange(len(A)), T, 10), ref.csls_penalty(T, np.arange(len(T)), A, 10)
    assert pens[1][hub] == pens[1].max()                     # ... which is what its penalty says
    csls_top = ref.topk(A, np.arange(len(A)), T, 1, *pens)[1][:, 0]
    assert (csls_top == hub).mean() <= 0.1
    be = ref.NumpyBackend()
    assert translation_precision(A, T, pairs, method="nn", top_k=(1,), backend=be)["precision"] == nn
    assert translation_precision(A, T, pairs, method="csls", knn=10, top_k=(1,), backend=be)["precision"] == csls
    # the target-side penalty against fewer source rows: another figure, the reference's
    few = translation_precision(A, T, pairs, method="csls", knn=10, top_k=(1, 5), backend=be, penalty_rows=15)
    assert few["precision"] == ref.precision_at(A, T, pairs, (1, 5), "csls", knn=10, penalty_rows=15)


def planted_permutation(n=300, d=20, seed=3):
    X, _, Q = ref.planted_rotation(seed=seed, V=n, d=d)
    perm = np.random.default_rng(seed + 2).permutation(n)
    Y = np.empty_like(X)
    Y[perm] = X @ Q.T                                        # source row s is target row perm[s]
    return X, Y, Q, perm


def test_refinement_on_a_planted_permutation_grows_the_dictionary_to_all_rows():
    X, Y, Q, perm = planted_permutation()
    rng = np.random.default_rng(0)
    seed_pairs = np.stack([np.arange(12), perm[:12]], axis=1)
    seed_pairs[:4, 1] = rng.permutation(seed_pairs[:4, 1])   # a third of the 12 seed pairs are wrong: fewer right ones than d
    first = align_tables(X, Y, seed_pairs, backend=ref.NumpyBackend())
    assert np.abs(first["W"] - Q).max() > 0.05               # the seed alone does not determine the rotation
    out = align_tables(X, Y, seed_pairs, refine=3, refine_vocab=300, backend=ref.NumpyBackend())
    sizes = out["dictionary_sizes"]
    print("dictionary sizes per round:", sizes)
    assert len(sizes) == 3 and sizes[-1] == 300 and sizes == sorted(sizes) and sizes[0] < 300
    assert np.abs(out["W"] - Q).max() <= 1e-12
    full = np.stack([np.arange(300), perm], axis=1)
    assert translation_precision(out["Y"], Y, full, method="csls", top_k=(1,), backend=ref.NumpyBackend())["precision"][1] == 1.0
    # --refine-vocab looks at the first rows of both sides only
    out = align_tables(X, Y, np.stack([np.arange(40), perm[:40]], axis=1), refine=1, refine_vocab=100, backend=ref.NumpyBackend())
    assert out["dictionary_sizes"][0] <= 100


# ---- 4. the command lines
VOCAB_S = ["<UNK>"] + ["s%03d" % i for i in range(1, 120)]          # s_i has id i
VOCAB_T = ["t%03d" % i for i in range(139)] + ["<UNK>"]


@pytest.fixture(scope="module")
def job_dirs(tmp_path_factory):
    """Two job directories at step 0 around a planted rotation with noise: source word s_i is target word t_perm[i]."""
    from trainer.postprocess import write_step0_job_dir
    root = tmp_path_factory.mktemp("align")
    rng = np.random.default_rng(11)
    X, _, Q = ref.planted_rotation(seed=4, V=120, d=12)
    perm = rng.permutation(139)[:120]
    Y = rng.standard_normal((140, 12))
    Y[perm] = X @ Q.T + 0.05 * rng.standard_normal((120, 12))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    write_step0_job_dir(root / "S", VOCAB_S, X, "Adagrad", {})
    write_step0_job_dir(root / "T", VOCAB_T, Y, "Adagrad", {})
    train = "".join("%s %s\n" % (VOCAB_S[i], VOCAB_T[perm[i]]) for i in range(1, 60)) + "s001 t%03d\nnobody t000\ns002 nothing\n" % perm[1]
    test = "".join("%s %s\n" % (VOCAB_S[i], VOCAB_T[perm[i]]) for i in range(60, 120)) + "s060 %s\nnobody t000\n" % VOCAB_T[perm[61]]
    (root / "train.txt").write_text(train)
    (root / "test.txt").write_text(test)
    return root, X, Y, perm


def run(argv):
    return align.main(argv, backend=ref.NumpyBackend(float32=True))


def job_tables(job):
    from trainer.train_utils import CheckpointManager
    return torch.load(CheckpointManager(str(job)).latest(), map_location="cpu", weights_only=False)["tables"]


def test_fit_then_eval_command_lines(job_dirs, tmp_path):
    from trainer import vectors
    from trainer.data_utils import read_vocab
    root, X, Y, perm = job_dirs
    A = tmp_path / "A"
    out = run(["fit", "--source-dir", str(root / "S"), "--target-dir", str(root / "T"), "--output-dir", str(A),
               "--dictionary", str(root / "train.txt"), "--optimizer", "Adagrad"])
    pairs = np.stack([np.arange(1, 60), perm[1:60]], axis=1)
    want = align_tables(X, Y, pairs, backend=ref.NumpyBackend(float32=True))
    assert np.array_equal(out["Y"], want["Y"]) and out["Y"].shape == (120, 12)
    t = job_tables(A)
    assert (t["V"], t["d"], int(t["global_step"]), t["optimizer"]) == (120, 12, 0, "Adagrad")
    assert np.array_equal(t["R"].numpy(), out["Y"]) and not t["C"].any() and not t["br"].any()
    params = json.loads((A / "params.json").read_text())
    assert params["embedding_size"] == 12 and params["job_dir"] == str(A) and read_vocab(params["vocab_txt"]) == VOCAB_S
    rec = json.loads((A / "align.json").read_text())
    assert (rec["source_job_dir"], rec["target_job_dir"], rec["source_step"], rec["target_step"]) == (str(root / "S"), str(root / "T"), 0, 0)
    assert (rec["anchors_used"], rec["anchors_skipped"], rec["anchor_counts"]["duplicates"]) == (59, 2, 1)
    assert (rec["normalize"], rec["refine"], rec["refine_vocab"], rec["knn"], rec["embeddings"]) == ("unit", 0, 15000, 10, "row")
    assert rec["top_singular_values"] == [float(x) for x in want["singular_values"]] and len(rec["top_singular_values"]) == 12
    assert rec["orthogonality_defect"] == want["orthogonality_defect"] <= 64 * 2.0 ** -24
    assert rec["anchor_cosine_after"] == want["anchor_cosine_after"] > 0.95 > rec["anchor_cosine_before"] == want["anchor_cosine_before"]
    assert rec["dictionary_sizes"] == [] and {"load", "anchors", "cross_gram", "svd", "rows_transform", "write_job_dir"} <= set(rec["seconds"])

    # eval: the held-out words, by both methods, against the reference scorer on the tables as written
    test_pairs = [[i, perm[i]] for i in range(60, 120)] + [[60, perm[61]]]
    for method, extra in (("nn", []), ("csls", ["--knn", "7"]), ("csls", ["--restrict-vocab", "130"])):
        got = run(["eval", "--source-dir", str(A), "--target-dir", str(root / "T"), "--dictionary", str(root / "test.txt"),
                   "--method", method, "--top-k", "1", "5"] + extra)
        bli = json.loads((A / "eval" / "bli.json").read_text())
        knn = 7 if "--knn" in extra else 10
        limit = 130 if "--restrict-vocab" in extra else None
        kept = [p for p in test_pairs if limit is None or p[1] < limit]
        want_p = ref.precision_at(out["Y"], Y[:limit], kept, (1, 5), method, knn=knn, penalty_rows=limit)
        assert bli["precision"] == {str(k): v for k, v in want_p.items()} == {str(k): v for k, v in got["precision"].items()}
        assert bli["queries"] == len({p[0] for p in kept}) and bli["pairs"] == len(kept)
        assert bli["pairs_skipped"] == 1 + len(test_pairs) - len(kept)
        assert (bli["method"], bli["knn"], bli["restrict_vocab"], bli["top_k"]) == (method, knn, limit, [1, 5])
        assert bli["precision"]["1"] >= 0.9                  # the planted partner, nearly always
    # trainer.vectors export opens the output
    import vectors_ref
    vec = tmp_path / "A.txt"
    vectors.main(["export", "--job-dir", str(A), "--output", str(vec)], backend=vectors_ref.NumpyVectorsBackend())
    assert vec.read_bytes() == vectors_ref.write_vectors(VOCAB_S[1:], out["Y"][1:], "glove", 6)       # <UNK> left out


def test_fit_with_shared_vocabulary_and_refinement(job_dirs, tmp_path):
    root, X, Y, perm = job_dirs
    # the source against itself rotated: every word is shared
    from trainer.postprocess import write_step0_job_dir
    Q = np.linalg.qr(np.random.default_rng(9).standard_normal((12, 12)))[0]
    write_step0_job_dir(tmp_path / "S2", VOCAB_S, (X @ Q.T).astype(np.float32), "Adam", {})
    A = tmp_path / "A"
    out = run(["fit", "--source-dir", str(root / "S"), "--target-dir", str(tmp_path / "S2"), "--output-dir", str(A), "--shared-vocab",
               "--anchors", "30", "--normalize", "none", "--refine", "1", "--refine-vocab", "100", "--knn", "5", "--optimizer", "Adam"])
    rec = json.loads((A / "align.json").read_text())
    assert (rec["anchors_used"], rec["anchors_skipped"], rec["shared_vocab"], rec["anchors"], rec["dictionary"]) == (30, 0, True, 30, None)
    assert rec["anchor_counts"]["shared"] == 119 and rec["dictionary_sizes"] == [100] and rec["optimizer"] == "Adam"
    assert np.abs(out["W"] - Q).max() <= 1e-4 and "build_dictionary" in rec["seconds"]


@pytest.mark.parametrize("case", ["same-as-source", "same-as-target", "sizes", "no-anchor", "knn", "anchors-without-shared", "refine"])
def test_fit_refuses_before_any_directory_is_made(job_dirs, tmp_path, case):
    from trainer.postprocess import write_step0_job_dir
    root, X, Y, perm = job_dirs
    A = tmp_path / "A"
    argv = ["fit", "--source-dir", str(root / "S"), "--target-dir", str(root / "T"), "--output-dir", str(A),
            "--dictionary", str(root / "train.txt")]
    if case == "same-as-source":
        argv[6] = str(root / "S")
    elif case == "same-as-target":
        argv[6] = str(root / "T" / ".." / "T")
    elif case == "sizes":
        write_step0_job_dir(tmp_path / "narrow", VOCAB_T, Y[:, :8].copy(), "Adagrad", {})
        argv[4] = str(tmp_path / "narrow")
    elif case == "no-anchor":
        (tmp_path / "none.txt").write_text("nobody nothing\n")
        argv[-1] = str(tmp_path / "none.txt")
    elif case == "knn":
        argv += ["--refine", "1", "--knn", "200"]
    elif case == "anchors-without-shared":
        argv += ["--anchors", "5"]
    elif case == "refine":
        argv += ["--refine", "-1"]
    before = {d: sorted(p.name for p in (root / d).iterdir()) for d in ("S", "T")}
    with pytest.raises(ValueError):
        run(argv)
    assert not A.exists() and {d: sorted(p.name for p in (root / d).iterdir()) for d in ("S", "T")} == before
