"""trainer.svd on the CPU: the driver (range finder, reweighting, errors, determinism) with the NumPy backend of
tests/svd_ref.py, the command line's job directory, and the ABI of libglove_factor_hip.so.  The kernels themselves:
tests/test_gpu_svd.py."""
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import svd_ref as ref
from trainer import svd
from trainer.svd import svd_embeddings

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "glove_factor_hip.h"
GOLDEN = REPO / "tests" / "golden"
PLANTED = dict(V=700, d=12, transform="none", oversample=4)


@pytest.fixture(scope="module")
def planted():
    return ref.planted_matrix()


def reconstruction(out, n_cols):
    return (out["R"].astype(np.float64) @ out["C"].astype(np.float64).T)[:, :n_cols]


# ---- 1. the planted matrix
@pytest.mark.parametrize("power_iterations", [0, 2])
def test_planted_matrix_float64_matches_the_closed_form(planted, power_iterations):
    row, col, val, M, sv = planted
    out = svd_embeddings(row, col, val, power_iterations=power_iterations, backend=ref.NumpyBackend(), **PLANTED)
    assert out["R"].shape == (700, 12) and out["C"].shape == (700, 12) and out["R"].dtype == np.float64
    assert out["nnz"] == out["nnz_reweighted"] == len(val)
    assert np.abs(out["singular_values"] - sv).max() <= 1e-10 * sv[0]
    assert np.linalg.norm(reconstruction(out, 530) - M) <= 1e-10 * np.linalg.norm(M)
    assert not out["C"][530:].any()                         # the columns the matrix does not have


# ---- 2. reweighting
HAND = np.array([[4.0, 1.0, 0.0, 2.5, 0.0],
                 [1.0, 0.0, 3.0, 0.0, 0.5],
                 [0.0, 3.0, 9.0, 1.0, 0.0],
                 [2.5, 0.0, 1.0, 0.0, 7.0],
                 [0.0, 0.5, 0.0, 7.0, 2.0]])


def hand_expected(kind, cds, shift):
    X = HAND
    if kind == "none":
        return X.copy()
    if kind == "sqrt":
        return np.sqrt(X)
    if kind == "log1p":
        return np.log(1.0 + X)
    r = X.sum(axis=1)
    c = X.sum(axis=0) ** cds
    out = np.zeros_like(X)
    for i in range(5):
        for j in range(5):
            if X[i, j] > 0:
                out[i, j] = max(0.0, math.log(X[i, j] * c.sum() / (r[i] * c[j])) - math.log(shift))
    return out


@pytest.mark.parametrize("kind,cds,shift", [("none", 1, 1), ("sqrt", 1, 1), ("log1p", 1, 1), ("ppmi", 1, 1), ("ppmi", 0.75, 1),
                                            ("ppmi", 1, 5), ("ppmi", 0.75, 5), ("ppmi", 0.75, 1.5)])
def test_every_transform_on_a_hand_sized_table(kind, cds, shift):
    """A full-rank factorisation (d = V, no oversampling) reconstructs the reweighted matrix itself: marginals, smoothing,
    shift and the dropped entries all show in R C^T."""
    want = hand_expected(kind, cds, shift)
    if not want.any():                                       # (shift 5 leaves nothing of this table)
        row, col = np.nonzero(HAND)
        with pytest.raises(ValueError, match="no entry is positive"):
            svd_embeddings(row, col, HAND[row, col], 5, 5, transform=kind, cds=cds, shift=shift, backend=ref.NumpyBackend())
        return
    row, col = np.nonzero(HAND)
    out = svd_embeddings(row, col, HAND[row, col], 5, 5, transform=kind, cds=cds, shift=shift, oversample=0,
                         power_iterations=1, backend=ref.NumpyBackend())
    assert out["nnz"] == 15 and out["nnz_reweighted"] == np.count_nonzero(want)
    np.testing.assert_allclose(reconstruction(out, 5), want, rtol=0, atol=1e-12 * np.abs(want).max())
    # the backend's own transform, entry by entry
    c = HAND.sum(axis=0) ** cds
    got = ref.reweight(row, col, HAND[row, col], kind, HAND.sum(axis=1), c, c.sum(), math.log(shift))
    np.testing.assert_allclose(got, want[row, col], rtol=1e-15, atol=1e-15)


def test_values_that_are_not_positive_leave_the_matrix():
    got = ref.reweight([0, 0, 1], [0, 1, 1], [0.0, -2.0, 4.0], "sqrt")
    assert got.tolist() == [0.0, 0.0, 2.0]


def test_ppmi_of_the_golden_table_keeps_1164_of_2480_entries():
    row, col, val, V = ref.golden_cooccurrence()
    out = svd_embeddings(row, col, val, V, 8, backend=ref.NumpyBackend())          # the defaults: cds 0.75, shift 1
    assert (out["nnz"], out["nnz_reweighted"]) == (2480, 1164)


# ---- 3. errors
def test_argument_errors():
    be = ref.NumpyBackend()
    row, col, val = np.array([0, 1, 2, 1]), np.array([1, 0, 2, 0]), np.ones(4)
    with pytest.raises(ValueError, match="1 .row, col. pairs are listed more than once"):
        svd_embeddings(row, col, val, 3, 2, backend=be)
    with pytest.raises(ValueError, match="nnz == 0"):
        svd_embeddings(row[:0], col[:0], val[:0], 3, 2, backend=be)
    for bad in (np.array([0, 1, 3]), np.array([0, -1, 2])):
        with pytest.raises(ValueError, match="ids must lie in"):
            svd_embeddings(bad, col[:3], val[:3], 3, 2, backend=be)
        with pytest.raises(ValueError, match="ids must lie in"):
            svd_embeddings(row[:3], bad, val[:3], 3, 2, backend=be)
    with pytest.raises(ValueError, match="embedding size"):
        svd_embeddings(row[:3], col[:3], val[:3], 3, 4, backend=be)
    with pytest.raises(ValueError, match="transform"):
        svd_embeddings(row[:3], col[:3], val[:3], 3, 2, transform="pmi", backend=be)


def test_oversampling_beyond_the_vocabulary_clips_the_width():
    row, col = np.nonzero(HAND)
    out = svd_embeddings(row, col, HAND[row, col], 5, 3, transform="none", oversample=10, backend=ref.NumpyBackend())
    assert out["l"] == 5 and out["R"].shape == (5, 3)
    np.testing.assert_allclose(out["singular_values"], np.linalg.svd(HAND, compute_uv=False)[:3], rtol=1e-12)


# ---- 4. determinism
def test_signs_seeds_and_repeats(planted):
    row, col, val, M, sv = planted
    be = ref.NumpyBackend()
    a = svd_embeddings(row, col, val, power_iterations=2, seed=0, backend=be, **PLANTED)
    b = svd_embeddings(row, col, val, power_iterations=2, seed=0, backend=be, **PLANTED)
    c = svd_embeddings(row, col, val, power_iterations=2, seed=1, backend=be, **PLANTED)
    for k in ("R", "C", "singular_values"):
        assert np.array_equal(a[k], b[k])
    assert np.abs(a["singular_values"] - c["singular_values"]).max() <= 1e-10 * sv[0]
    for out in (a, c):
        U = out["R"]                                        # a positive multiple of U, column by column
        top = np.abs(U).argmax(axis=0)
        assert (U[top, np.arange(12)] > 0).all()
    # with distinct singular values and the signs fixed, the vectors themselves do not depend on the seed
    np.testing.assert_allclose(a["R"] @ a["R"].T, c["R"] @ c["R"].T, atol=1e-9 * sv[0])


def test_ties_of_the_sign_rule_go_to_the_lower_index():
    X = np.array([[0.0, 2.0], [2.0, 0.0]])                   # u = (1, +-1) / sqrt 2: two entries of equal magnitude
    row, col = np.nonzero(X)
    out = svd_embeddings(row, col, X[row, col], 2, 2, transform="none", oversample=0, backend=ref.NumpyBackend())
    assert (out["R"][0] > 0).all()


# ---- 5. the command line
@pytest.fixture(scope="module")
def cli_job(tmp_path_factory):
    job = tmp_path_factory.mktemp("svd") / "job"
    argv = ["--train-csv", str(GOLDEN / "text8_cov100_ctx2_interaction.csv"), "--vocab-txt", str(GOLDEN / "text8_cov100_ctx2_vocab.txt"),
            "--job-dir", str(job), "--embedding-size", "8", "--optimizer", "Adagrad"]
    return job, svd.main(argv, backend=ref.NumpyBackend(float32=True))


def test_command_line_writes_an_ordinary_job_dir(cli_job):
    from trainer.data_utils import file_lines, load_interaction_csv
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager
    job, out = cli_job
    V = file_lines(GOLDEN / "text8_cov100_ctx2_vocab.txt")
    latest = CheckpointManager(str(job)).latest()
    assert latest is not None and latest.endswith("model.ckpt-0.pt")
    tables = torch.load(latest, map_location="cpu", weights_only=False)["tables"]
    assert (tables["V"], tables["d"], int(tables["global_step"]), tables["optimizer"]) == (V, 8, 0, "Adagrad")
    assert not tables["br"].any() and not tables["bc"].any()
    assert tables["R"].shape == (V, 8) and np.array_equal(tables["R"].numpy(), out["R"])
    assert np.array_equal(tables["C"].numpy(), out["C"])
    # ... and R is the driver's for the same table
    coo = load_interaction_csv(str(GOLDEN / "text8_cov100_ctx2_interaction.csv"), str(GOLDEN / "text8_cov100_ctx2_vocab.txt"),
                               target_name="value")
    again = svd_embeddings(coo["row"], coo["col"], coo["y"], V, 8, backend=ref.NumpyBackend(float32=True))
    assert np.array_equal(tables["R"].numpy(), again["R"])
    fresh = DeviceTables(V, 8, "Adagrad", device="cpu", seed=3)
    assert CheckpointManager(str(job)).restore(fresh)
    assert fresh.global_step == 0 and np.array_equal(fresh.embeddings("R").numpy(), out["R"])
    assert (fresh.s1["R"] == 0.1).all()                      # Adagrad's initial accumulator
    params = json.loads((job / "params.json").read_text())
    assert params["embedding_size"] == 8 and params["optimizer"] == "Adagrad" and params["job_dir"] == str(job)
    assert Path(params["vocab_txt"]).parent == job and "input_fn_args" in params


def test_command_line_records_the_run(cli_job):
    job, out = cli_job
    rec = json.loads((job / "svd.json").read_text())
    s = rec["singular_values"]
    assert len(s) == 8 and all(a >= b > 0 for a, b in zip(s, s[1:])) and s == [float(x) for x in out["singular_values"]]
    assert rec["transform"] == "ppmi" and rec["cds"] == 0.75 and rec["embedding_size"] == 8
    assert rec["nnz"] == out["nnz"] and 0 < rec["nnz_reweighted"] == out["nnz_reweighted"] < rec["nnz"]
    assert {"load_csv", "csr_and_marginals", "reweight_and_compact", "range_finder", "small_eigenproblem"} <= set(rec["seconds"])


# ---- 6. the ABI
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
    from trainer import hip_api
    declared = declared_functions()
    protos = hip_api.factor_prototypes()
    assert len(declared) == 5
    assert set(declared) == set(protos) == set(hip_api.FACTOR_EXPORTED_SYMBOLS)
    assert declared == {name: len(args) for name, (_, args) in protos.items()}
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.glove_factor_abi_version() == hip_api.GLOVE_FACTOR_ABI_VERSION == 1
    assert "#define GLOVE_FACTOR_CHUNK %d" % hip_api.FACTOR_CHUNK in HEADER.read_text()


def test_the_size_query_is_a_pure_host_function(lib):
    q = lib.glove_csr_spmm_workspace_bytes
    sizes = [q(1000, nnz, 312) for nnz in (0, 1, 512, 513, 100000, 2 ** 31 - 1)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[1]
    assert q(1000, 100000, 312) >= 2 * math.ceil(100000 / 512) * 312 * 4
    assert 0 < q(1000, 100000, 0) < q(1000, 100000, 4)        # row sums: one double per slot
    for n_rows, nnz, l in ((0, 10, 8), (-1, 10, 8), (10, -1, 8), (10, 2 ** 31, 8), (10, 10, 6), (10, 10, 1028), (10, 10, -4)):
        assert q(n_rows, nnz, l) == 0, (n_rows, nnz, l)


def test_missing_factor_library_is_an_error_not_a_fallback(tmp_path):
    from trainer import hip_api
    with pytest.raises(hip_api.GloveHipError, match="no CPU fallback"):
        hip_api.load_factor_library(tmp_path / "libglove_factor_hip.so")
