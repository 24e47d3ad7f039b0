"""trainer.postprocess on the CPU: the driver (all-but-the-top, PCA reduction, centring, signs) with the NumPy backend of
tests/pca_ref.py, the command line's job directory, and the ABI of include/glove_factor_dense_hip.h.  The kernels
themselves: tests/test_gpu_postprocess.py."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pca_ref as ref
from trainer import postprocess
from trainer.postprocess import postprocess_table, principal_directions

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "glove_factor_dense_hip.h"
GOLDEN = REPO / "tests" / "golden"


@pytest.fixture(scope="module")
def planted():
    return ref.planted()


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


def test_the_header_and_the_binding_declare_the_same_functions(lib):
    """The version query, the workspace query and the three calls: the five entry points the header's table lists."""
    from trainer import hip_api
    declared = declared_functions()
    protos = hip_api.factor_dense_prototypes()
    assert set(declared) == set(protos) == set(hip_api.FACTOR_DENSE_EXPORTED_SYMBOLS)
    assert set(declared) == {"glove_factor_dense_abi_version", "glove_gram_workspace_bytes", "glove_col_sums_f64",
                             "glove_gram_f64", "glove_rows_transform_f32"}
    assert declared == {name: len(args) for name, (_, args) in protos.items()}
    for name in declared:
        assert hasattr(lib, name), name
    others = (hip_api.EXPORTED_SYMBOLS + hip_api.EVAL_EXPORTED_SYMBOLS + hip_api.EVAL_SIM_EXPORTED_SYMBOLS
              + hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS + hip_api.PREP_EXPORTED_SYMBOLS + hip_api.TEXT_EXPORTED_SYMBOLS
              + hip_api.VECTORS_EXPORTED_SYMBOLS + hip_api.FACTOR_EXPORTED_SYMBOLS)
    assert not set(declared) & set(others)
    assert not set(protos) & set(hip_api.factor_prototypes())
    assert lib.glove_factor_dense_abi_version() == hip_api.GLOVE_FACTOR_DENSE_ABI_VERSION == 1
    assert "#define GLOVE_FACTOR_DENSE_ABI_VERSION 1" in HEADER.read_text()


def test_chunk_and_slice_are_the_headers():
    from trainer import hip_api
    text = HEADER.read_text()
    assert "#define GLOVE_GRAM_CHUNK %d" % hip_api.GRAM_CHUNK in text
    assert "#define GLOVE_GRAM_SLICE %d" % hip_api.GRAM_SLICE in text
    assert (hip_api.GRAM_CHUNK, hip_api.GRAM_SLICE) == (1024, 16384) and hip_api.GRAM_SLICE == 16 * hip_api.GRAM_CHUNK


def test_the_size_query_is_a_pure_host_function(lib):
    from trainer.hip_api import GRAM_SLICE as S
    q = lib.glove_gram_workspace_bytes
    assert q(1, 4) == 256                                    # one slot of 16 doubles: never less than 256 B
    for n, d in ((1, 304), (S, 304), (S + 1, 304), (2 * S + 7, 64), (400000, 320), (2 ** 31 - 1, 1024)):
        want = math.ceil(n / S) * d * d * 8
        assert q(n, d) == max(256, (want + 255) // 256 * 256), (n, d)
    for n, d in ((0, 8), (-1, 8), (2 ** 31, 8), (10, 0), (10, 6), (10, 1028), (10, -4), (10, 2)):
        assert q(n, d) == 0, (n, d)


def test_argument_errors_come_back_before_any_launch(lib):
    """Null pointers and sizes out of range: the answer is a GLOVE_E_* code, nothing is enqueued (no device is needed)."""
    big = 1 << 40
    assert lib.glove_col_sums_f64(None, 10, 8, None, None, big, None) == -1
    assert lib.glove_gram_f64(None, 10, 8, None, None, None, big, None) == -1
    assert lib.glove_rows_transform_f32(None, 10, 8, None, 8, None, None, None) == -1
    for n, d in ((0, 8), (2 ** 31, 8), (10, 6), (10, 1028)):
        assert lib.glove_col_sums_f64(16, n, d, 16, 16, big, None) == -1
        assert lib.glove_gram_f64(16, n, d, None, 16, 16, big, None) == -1
        assert lib.glove_rows_transform_f32(16, n, d, 32, 8, None, 48, None) == -1
    for m in (0, 6, 1028):
        assert lib.glove_rows_transform_f32(16, 10, 8, 32, m, None, 48, None) == -1
    assert lib.glove_rows_transform_f32(16, 10, 8, 32, 8, None, 16, None) == -1          # Y_out is X
    assert lib.glove_col_sums_f64(16, 10, 8, 16, 16, 255, None) == -2
    assert lib.glove_gram_f64(16, 20000, 8, None, 16, 16, 2 * 8 * 8 * 8 - 1, None) == -2


def test_missing_factor_library_is_an_error_not_a_fallback(tmp_path):
    from trainer import hip_api
    with pytest.raises(hip_api.GloveHipError, match="no CPU fallback"):
        hip_api.load_factor_library(tmp_path / "libglove_factor_hip.so")


# ---- 2. the driver on the planted table
def test_all_but_the_top_centres_and_removes_the_planted_directions(planted):
    W, Q, mean = planted
    out = postprocess_table(W, remove=2, backend=ref.NumpyBackend())
    Y = out["Y"]
    assert Y.shape == W.shape and Y.dtype == np.float64
    scale = np.abs(W).max()
    assert np.abs(Y.mean(axis=0)).max() <= 1e-12 * scale
    assert np.abs(out["mean"] - W.astype(np.float64).mean(axis=0)).max() <= 1e-12 * scale
    # exactly orthogonal to the two directions that were removed ...
    assert np.abs(Y @ out["components"].T).max() <= 1e-10 * scale
    # ... which are the planted ones up to the sampling error of 20000 rows: the angle between a sample direction and its
    # population one is about sqrt(l_j l_k) / ((l_j - l_k) sqrt(n)) <= 4 / (15 sqrt(20000)) = 0.002; 0.03 is allowed,
    # squared against the variance that stood there
    Xc = W.astype(np.float64) - W.astype(np.float64).mean(axis=0)
    for k in range(2):
        assert np.square(Y @ Q[:, k]).sum() <= 0.03 ** 2 * np.square(Xc @ Q[:, k]).sum()
    # the other directions are left as they were
    assert np.square(Y @ Q[:, 2:]).sum() >= 0.99 * np.square(Xc @ Q[:, 2:]).sum()
    lam = out["eigenvalues"]
    assert lam.shape == (24,) and (np.diff(lam) <= 0).all()
    np.testing.assert_allclose(lam[:2] / len(W), [36.0, 16.0], rtol=0.05)
    assert abs(out["variance_removed"] - lam[:2].sum() / lam.sum()) <= 1e-15
    assert abs(out["variance_removed"] + out["variance_kept"] - 1.0) <= 1e-12
    assert {"col_sums", "gram", "eigh", "rows_transform"} <= set(out["seconds"])


def test_reduce_to_gives_a_diagonal_covariance_with_the_next_eigenvalues(planted):
    W, _, _ = planted
    out = postprocess_table(W, remove=2, reduce_to=7, backend=ref.NumpyBackend())      # 7: padded to 8 rows of T
    Y, lam = out["Y"], out["eigenvalues"]
    assert Y.shape == (len(W), 7) and out["components"].shape == (9, 24)
    cov = Y.T @ Y
    assert np.abs(Y.mean(axis=0)).max() <= 1e-12 * np.abs(W).max()
    np.testing.assert_allclose(np.diag(cov), lam[2:9], rtol=1e-10)
    assert np.abs(cov - np.diag(np.diag(cov))).max() <= 1e-10 * lam[0]
    assert abs(out["variance_kept"] - lam[2:9].sum() / lam.sum()) <= 1e-15
    # remove = 0: plain PCA, the leading components
    pca = postprocess_table(W, remove=0, reduce_to=4, backend=ref.NumpyBackend())
    np.testing.assert_allclose(np.diag(pca["Y"].T @ pca["Y"]), lam[:4], rtol=1e-10)
    assert pca["variance_removed"] == 0.0


def test_without_centring_the_mean_stays_in(planted):
    W, _, mean = planted
    out = postprocess_table(W, remove=1, center=False, backend=ref.NumpyBackend())
    X = W.astype(np.float64)
    lam, E = np.linalg.eigh(X.T @ X)
    u = E[:, -1]
    want = X - np.outer(X @ u, u)                            # the top direction of the uncentred second moments
    np.testing.assert_allclose(out["Y"], want, atol=1e-10 * np.abs(W).max())
    assert np.abs(out["Y"].mean(axis=0)).max() > 0.1         # (the planted mean is 2 N(0, 1) per column)
    np.testing.assert_allclose(out["mean"], X.mean(axis=0), atol=1e-12 * np.abs(W).max())      # still reported


def test_float32_backend_stays_at_float32_rounding(planted):
    """The figure the GPU test's bound is built from (the device is allowed 8 times it): the largest deviation over the
    largest entry.  The components are well conditioned (relative eigenvalue gaps of 0.27 and more), so it stays within
    a few hundred float32 roundings: 2^-24 times the 24 columns times the inverse gap, 6e-6, with a factor of 4 to spare."""
    W, _, _ = planted
    for settings in (dict(remove=2), dict(remove=2, reduce_to=8)):
        f64 = postprocess_table(W, backend=ref.NumpyBackend(), **settings)
        f32 = postprocess_table(W, backend=ref.NumpyBackend(float32=True), **settings)
        assert f32["Y"].dtype == np.float32
        e = np.abs(f32["Y"] - f64["Y"]).max() / np.abs(f64["Y"]).max()
        print("%s: NumPy float32 from float64 %.3g" % (settings, e))
        assert 0 < e <= 4 * 2.0 ** -24 * 24 / 0.27


def test_sign_rule_and_its_ties():
    G = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 0.5]])      # eigenvectors (1, -1, 0), (1, 1, 0), e_3
    lam, E = principal_directions(G)
    np.testing.assert_allclose(lam, [3.0, 1.0, 0.5], atol=1e-14)
    r = math.sqrt(0.5)
    np.testing.assert_allclose(E.T, [[r, -r, 0.0], [r, r, 0.0], [0.0, 0.0, 1.0]], atol=1e-14)     # ties: the lower index
    lam, E = principal_directions(np.diag([1.0, 5.0]))
    assert lam.tolist() == [5.0, 1.0] and E.T.tolist() == [[0.0, 1.0], [1.0, 0.0]]
    out = postprocess_table(ref.planted()[0][:500], remove=3, backend=ref.NumpyBackend())
    C = out["components"]
    assert (C[np.arange(3), np.abs(C).argmax(axis=1)] > 0).all()


def test_driver_refusals():
    W = np.ones((10, 8), np.float32)
    be = ref.NumpyBackend()
    for settings in (dict(remove=-1), dict(remove=9), dict(remove=4, reduce_to=5), dict(remove=0, reduce_to=0)):
        with pytest.raises(ValueError):
            postprocess_table(W, backend=be, **settings)
    with pytest.raises(ValueError, match="table"):
        postprocess_table(np.ones(8, np.float32), remove=1, backend=be)


# ---- 3. the command line
@pytest.fixture(scope="module")
def source_job(tmp_path_factory):
    """A job directory of trainer.svd's on the golden table, the way tests/test_svd.py builds one."""
    import svd_ref
    from trainer import svd
    job = tmp_path_factory.mktemp("post") / "job"
    argv = ["--train-csv", str(GOLDEN / "text8_cov100_ctx2_interaction.csv"), "--vocab-txt", str(GOLDEN / "text8_cov100_ctx2_vocab.txt"),
            "--job-dir", str(job), "--embedding-size", "8", "--optimizer", "Adagrad"]
    return job, svd.main(argv, backend=svd_ref.NumpyBackend(float32=True))


def run(argv):
    return postprocess.main(argv, backend=ref.NumpyBackend(float32=True))


def job_tables(job):
    from trainer.train_utils import CheckpointManager
    return torch.load(CheckpointManager(str(job)).latest(), map_location="cpu", weights_only=False)["tables"]


def test_command_line_writes_an_ordinary_job_dir(source_job, tmp_path):
    from test_analogy import RefBackend
    from trainer.data_utils import read_vocab
    from trainer.estimator import Estimator
    job, svd_out = source_job
    P = tmp_path / "P"
    out = run(["--job-dir", str(job), "--output-dir", str(P), "--optimizer", "Adagrad"])
    V = svd_out["R"].shape[0]
    want = postprocess_table(svd_out["R"], remove=1, backend=ref.NumpyBackend(float32=True))      # the default: max(1, round(8 / 100))
    assert np.array_equal(out["Y"], want["Y"]) and out["Y"].shape == (V, 8)
    t = job_tables(P)
    assert (t["V"], t["d"], int(t["global_step"]), t["optimizer"]) == (V, 8, 0, "Adagrad")
    assert np.array_equal(t["R"].numpy(), out["Y"]) and not t["C"].any() and not t["br"].any() and not t["bc"].any()
    params = json.loads((P / "params.json").read_text())
    assert params["embedding_size"] == 8 and params["job_dir"] == str(P) and Path(params["vocab_txt"]) == P / "vocab.txt"
    assert read_vocab(params["vocab_txt"]) == read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))
    rec = json.loads((P / "postprocess.json").read_text())
    assert rec["source_job_dir"] == str(job) and rec["source_step"] == 0 and rec["remove_components"] == 1
    assert rec["reduce_to"] is None and rec["center"] is True and rec["embeddings"] == "row" and rec["embedding_size"] == 8
    assert rec["top_eigenvalues"] == [float(x) for x in out["eigenvalues"]]
    assert 0 < rec["variance_removed"] < 1 and abs(rec["variance_removed"] + rec["variance_kept"] - 1) < 1e-6
    assert {"load", "col_sums", "gram", "eigh", "rows_transform", "write_job_dir"} <= set(rec["seconds"])
    e = Estimator(params, backend=RefBackend(), device="cpu")
    assert e.vocab_size == V and e.model.tables.global_step == 0
    assert np.array_equal(e._evaluation_table("row", None).numpy()[:, :8], out["Y"])


def test_command_line_reduces_restricts_and_chains(source_job, tmp_path):
    from test_analogy import RefBackend
    from trainer.data_utils import read_vocab
    from trainer.estimator import Estimator
    job, svd_out = source_job
    P, P2 = tmp_path / "P", tmp_path / "P2"
    out = run(["--job-dir", str(job), "--output-dir", str(P), "--embeddings", "sum", "--remove-components", "1", "--reduce-to", "5",
               "--restrict-vocab", "60", "--no-center", "--optimizer", "Adam"])
    W = (svd_out["R"] + svd_out["C"])[:60]
    want = postprocess_table(W, remove=1, reduce_to=5, center=False, backend=ref.NumpyBackend(float32=True))
    assert out["Y"].shape == (60, 5) and np.array_equal(out["Y"], want["Y"])
    params = json.loads((P / "params.json").read_text())
    assert params["embedding_size"] == 5 and params["optimizer"] == "Adam"
    assert read_vocab(params["vocab_txt"]) == read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))[:60]
    t = job_tables(P)
    assert (t["V"], t["d"], t["optimizer"]) == (60, 5, "Adam") and np.array_equal(t["R"].numpy(), out["Y"])
    rec = json.loads((P / "postprocess.json").read_text())
    assert (rec["reduce_to"], rec["restrict_vocab"], rec["center"], rec["source_embedding_size"]) == (5, 60, False, 8)
    e = Estimator(params, backend=RefBackend(), device="cpu")
    assert e.vocab_size == 60
    # chaining: the tool on its own output (Raunak et al.: all-but-the-top once more)
    again = run(["--job-dir", str(P), "--output-dir", str(P2), "--remove-components", "1", "--optimizer", "Adam"])
    assert again["Y"].shape == (60, 5)
    assert json.loads((P2 / "postprocess.json").read_text())["source_job_dir"] == str(P)
    assert np.abs(again["Y"].mean(axis=0)).max() <= 1e-5 * np.abs(out["Y"]).max()


@pytest.mark.parametrize("extra", [["--remove-components", "-1"], ["--remove-components", "9"],
                                   ["--remove-components", "4", "--reduce-to", "5"], ["--reduce-to", "0"], "same"])
def test_command_line_refuses_before_any_directory_is_made(source_job, tmp_path, extra):
    job, _ = source_job
    P = tmp_path / "P"
    before = sorted(p.name for p in job.iterdir())
    with pytest.raises(ValueError):
        run(["--job-dir", str(job), "--output-dir", str(job if extra == "same" else P)] + ([] if extra == "same" else extra))
    assert not P.exists() and sorted(p.name for p in job.iterdir()) == before
