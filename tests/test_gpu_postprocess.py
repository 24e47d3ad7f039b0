"""The dense half of libglove_factor_hip.so on the GPU (include/glove_factor_dense_hip.h) against the float64 reference of
tests/pca_ref.py: column sums, the Gram matrix and the row transform at the smallest shapes that can go wrong, then
trainer.postprocess's driver and command line.

Shapes: n = 1, CHUNK - 1, CHUNK, CHUNK + 1, SLICE, SLICE + 1, 2 SLICE + 7 (one row; around the end of a float32 chain;
around the end of a float64 slice; three slices, the last of 7 rows) times d = 4 (the smallest width), 36 (one full
32-column tile and a 4-column edge), 64 (whole tiles only), 304 holding a 300-column model (zero padding; five 64-column
blocks, the last of 48 columns), and d = 320 at n = SLICE + 1.  The data are signed with a column mean of 3 to 6
standard deviations.

Tolerances are derived, not measured; u = 2^-24, g(k) = (k + 2) u / (1 - (k + 2) u):
  - Gram matrix: a chunk is a float32 fmaf chain of at most CHUNK terms, |got - ref| <= g(CHUNK) sum_v |x~_vi x~_vj| + 1e-30
    (the float64 combination adds at most n / CHUNK 2^-53 of that sum, which g's two spare terms cover); the reference
    takes x~ as the float32 difference, like the kernel;
  - column sums: |got - ref| <= n 2^-53 sum |x| against the exactly rounded float64 sum (math.fsum);
  - transform: a chain of d terms and one subtraction, |got - ref| <= g(d) (sum_k |x_k T_jk| + |shift_j|) + 1e-30;
  - driver: the deviation e_ref of the NumPy float32 backend from the NumPy float64 backend on the same input is the
    rounding level of the reference itself; the device is allowed 8 e_ref from the float64 result.  Both are printed.
The widths here stop at five 64-column blocks; tests/test_gpu_factor_row_shapes.py goes on to the limit of sixteen, bit for bit."""
import functools
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import pca_ref as ref
from trainer.hip_api import GRAM_CHUNK as CHUNK, GRAM_SLICE as SLICE

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -24
ROWS = (1, CHUNK - 1, CHUNK, CHUNK + 1, SLICE, SLICE + 1, 2 * SLICE + 7)
WIDTHS = ((4, 4), (36, 36), (64, 64), (304, 300))            # (row stride, the model's columns)
SHAPES = [(n, d, dm) for d, dm in WIDTHS for n in ROWS] + [(SLICE + 1, 320, 320)]


def g(k):
    return (k + 2) * U / (1 - (k + 2) * U)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def case(n, d, d_model):
    """A table, its float32 mean and the float64 results every test of that shape shares (built once, never written)."""
    rng = np.random.default_rng(1000003 * d + n)
    X = np.zeros((n, d), np.float32)
    centre = rng.uniform(3.0, 6.0, d_model) * rng.choice([-1.0, 1.0], d_model)
    X[:, :d_model] = rng.standard_normal((n, d_model)) + centre
    X64 = X.astype(np.float64)
    sums = np.array([math.fsum(X64[:, k]) for k in range(d)])
    mean = (sums / n).astype(np.float32)
    c = dict(X=X, mean=mean, sums=sums, sums_bound=n * 2.0 ** -53 * np.abs(X64).sum(axis=0))
    for key, m_ in (("G", mean), ("G0", None)):
        Xc = (X if m_ is None else X - m_).astype(np.float64)                  # the float32 difference, then float64
        c[key] = Xc.T @ Xc
        c[key + "_bound"] = g(CHUNK) * (np.abs(Xc).T @ np.abs(Xc)) + 1e-30
    return c


def ids(shape):
    return "n%d-d%d" % shape[:2]


# ---- 1. column sums
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_col_sums_against_exactly_rounded_sums(hip, shape):
    c = case(*shape)
    X = dev(c["X"])
    got = hip.col_sums(X)
    assert got.shape == (shape[1],) and got.dtype == torch.float64
    err = np.abs(got.cpu().numpy() - c["sums"])
    print("%s: largest error / bound %.3g" % (ids(shape), (err / np.maximum(c["sums_bound"], 1e-300)).max()))
    assert (err <= c["sums_bound"]).all()
    assert (got.cpu().numpy()[shape[2]:] == 0.0).all()        # the padding columns
    assert torch.equal(got, hip.col_sums(X))                  # bitwise repeatable


# ---- 2. the Gram matrix
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_gram_parity_symmetry_and_repeatability(hip, shape):
    n, d, d_model = shape
    c = case(*shape)
    X = dev(c["X"])
    for key, mean in (("G", dev(c["mean"])), ("G0", None)):  # centred, and with a null mean
        got = hip.gram(X, mean)
        assert got.shape == (d, d) and got.dtype == torch.float64
        G = got.cpu().numpy()
        err = np.abs(G - c[key])
        print("%s, %s: largest error / bound %.3g" % (ids(shape), "mean" if mean is not None else "null mean",
                                                      (err / c[key + "_bound"]).max()))
        assert (err <= c[key + "_bound"]).all()
        assert torch.equal(got, got.T)                        # bitwise symmetric
        assert torch.equal(got, hip.gram(X, mean))            # bitwise repeatable
        assert (G[d_model:] == 0.0).all() and (G[:, d_model:] == 0.0).all()       # padding: exact zeros (d = 304: 300 ..)


@pytest.mark.parametrize("d, d_model", [(36, 36), (304, 300)])
@pytest.mark.parametrize("prefix", [CHUNK, SLICE], ids=["chunk", "slice"])
def test_gram_bits_are_those_of_the_chunks_and_slices(hip, prefix, d, d_model):
    """Rows of zeros beyond the first chunk (the first slice) add exact zeros: the bits are the prefix's alone, however
    many chunks, slices and workgroups the call had."""
    n = 2 * SLICE + 7
    X = case(n, d, d_model)["X"].copy()
    X[prefix:] = 0.0
    whole = hip.gram(dev(X))
    assert torch.equal(whole, hip.gram(dev(X[:prefix])))
    assert torch.equal(whole, hip.gram(dev(X[:prefix + CHUNK + 3])))
    assert torch.equal(hip.col_sums(dev(X)), hip.col_sums(dev(X[:prefix])))


def test_gram_chunk_partials_are_float32_chains(hip):
    """One chunk: the fmaf chain of the header, row by row.  The restatement holds a b exactly in float64 and rounds
    a b + s to float64 and then to float32, which differs from fmaf's single rounding only when the float64 sum lands
    on a float32 tie (about 2^-29 per step): one float32 ulp is allowed for that, against g(CHUNK)'s 1025."""
    c = case(CHUNK, 4, 4)
    X = c["X"]
    got = hip.gram(dev(X)).cpu().numpy()
    for i, j in ((0, 0), (0, 3), (2, 1)):
        s = np.float32(0.0)
        for v in range(CHUNK):
            s = np.float32(np.float64(X[v, i]) * np.float64(X[v, j]) + np.float64(s))
        assert got[i, j] == np.float32(got[i, j])             # a single chunk: G is a float32 number
        assert abs(got[i, j] - np.float64(s)) <= np.spacing(np.float32(abs(s)))


# ---- 3. the transform
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_rows_transform_parity(hip, shape):
    n, d, d_model = shape
    c = case(*shape)
    X, X64 = dev(c["X"]), c["X"].astype(np.float64)
    rng = np.random.default_rng(7 * d + n)
    for m in sorted({4, 36, d} if d >= 36 else {4, 36}):
        T = rng.standard_normal((m, d)).astype(np.float32)
        shift = (5.0 * rng.standard_normal(m)).astype(np.float32)
        T64 = T.astype(np.float64)
        plain, mag = X64 @ T64.T, np.abs(X64) @ np.abs(T64).T
        for sh in (shift, None):                              # with the shift, and null
            got = hip.rows_transform(X, dev(T), None if sh is None else dev(sh))
            assert got.shape == (n, m) and got.dtype == torch.float32
            want = plain if sh is None else plain - sh.astype(np.float64)
            bound = g(d) * (mag + (0.0 if sh is None else np.abs(sh.astype(np.float64)))) + 1e-30
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            print("%s, m = %d, %s: largest error / bound %.3g" % (ids(shape), m, "shift" if sh is not None else "null shift",
                                                                  (err / bound).max()))
            assert (err <= bound).all()
            assert torch.equal(got, hip.rows_transform(X, dev(T), None if sh is None else dev(sh)))


def test_rows_transform_rows_do_not_depend_on_the_tile(hip):
    """A k-ordered chain per entry: a row's bits are the same wherever it sits in a workgroup's tile, and a row of T's
    whichever its neighbours are."""
    c = case(SLICE + 1, 36, 36)
    X = dev(c["X"])
    T = dev(np.random.default_rng(3).standard_normal((36, 36)).astype(np.float32))
    whole = hip.rows_transform(X, T)
    assert torch.equal(whole[77:1000], hip.rows_transform(X[77:1000].contiguous(), T))
    assert torch.equal(whole[:, 32:36], hip.rows_transform(X, T[32:36].contiguous()))


# ---- 4. refusals
def test_refusals_return_without_a_launch(hip):
    from trainer.hip_api import GloveHipError, load_factor_library
    lib = load_factor_library()
    X = dev(case(CHUNK + 1, 36, 36)["X"])
    n, d = X.shape
    st = torch.cuda.current_stream().cuda_stream
    sums = torch.full((d,), -7.0, dtype=torch.float64, device="cuda:0")
    G = torch.full((d, d), -7.0, dtype=torch.float64, device="cuda:0")
    Y = torch.full((n, 8), -7.0, device="cuda:0")
    T = torch.ones(8, d, device="cuda:0")
    ws = torch.empty(lib.glove_gram_workspace_bytes(n, d), dtype=torch.uint8, device="cuda:0")
    p = lambda t: t.data_ptr()
    BAD, WS = -1, -2
    for nn, dd in ((0, d), (2 ** 31, d), (n, 0), (n, 34), (n, 1028)):
        assert lib.glove_col_sums_f64(p(X), nn, dd, p(sums), p(ws), ws.numel(), st) == BAD
        assert lib.glove_gram_f64(p(X), nn, dd, None, p(G), p(ws), ws.numel(), st) == BAD
        assert lib.glove_rows_transform_f32(p(X), nn, dd, p(T), 8, None, p(Y), st) == BAD
    for m in (0, 2, 6, 1028):
        assert lib.glove_rows_transform_f32(p(X), n, d, p(T), m, None, p(Y), st) == BAD
    assert lib.glove_col_sums_f64(None, n, d, p(sums), p(ws), ws.numel(), st) == BAD
    assert lib.glove_col_sums_f64(p(X), n, d, None, p(ws), ws.numel(), st) == BAD
    assert lib.glove_col_sums_f64(p(X), n, d, p(sums), None, ws.numel(), st) == BAD
    assert lib.glove_gram_f64(None, n, d, None, p(G), p(ws), ws.numel(), st) == BAD
    assert lib.glove_gram_f64(p(X), n, d, None, None, p(ws), ws.numel(), st) == BAD
    assert lib.glove_gram_f64(p(X), n, d, None, p(G), None, ws.numel(), st) == BAD
    assert lib.glove_rows_transform_f32(None, n, d, p(T), 8, None, p(Y), st) == BAD
    assert lib.glove_rows_transform_f32(p(X), n, d, None, 8, None, p(Y), st) == BAD
    assert lib.glove_rows_transform_f32(p(X), n, d, p(T), 8, None, None, st) == BAD
    assert lib.glove_rows_transform_f32(p(X), n, d, p(T), 8, None, p(X), st) == BAD       # Y_out is X
    assert lib.glove_col_sums_f64(p(X), n, d, p(sums), p(ws), ws.numel() - 1, st) == WS
    assert lib.glove_gram_f64(p(X), n, d, None, p(G), p(ws), ws.numel() - 1, st) == WS
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (G == -7.0).all() and (Y == -7.0).all()     # nothing ran
    # ... and the binding's own checks
    with pytest.raises(GloveHipError):
        hip.gram(X[:, :34].contiguous())
    with pytest.raises(GloveHipError):
        hip.gram(X.double())
    with pytest.raises(GloveHipError):
        hip.gram(X, mean=torch.zeros(d - 4, device="cuda:0"))
    with pytest.raises(GloveHipError):
        hip.col_sums(X[:0])
    with pytest.raises(GloveHipError):
        hip.rows_transform(X, T[:, :32].contiguous())
    with pytest.raises(GloveHipError):
        hip.rows_transform(X, T[:6].contiguous())
    with pytest.raises(GloveHipError, match="GLOVE_E_WORKSPACE"):
        hip.gram(X, ws=torch.empty(16, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(GloveHipError, match="GLOVE_E_BADARG"):
        hip.rows_transform(X, torch.ones(d, d, device="cuda:0"), out=X)


# ---- 5. the driver
@pytest.mark.parametrize("settings", [dict(remove=2), dict(remove=2, reduce_to=8)], ids=["remove2", "remove2-reduce8"])
def test_driver_on_the_planted_table(hip, settings):
    from trainer.postprocess import postprocess_table
    W, _, _ = ref.planted()
    f64 = postprocess_table(W, backend=ref.NumpyBackend(), **settings)
    f32 = postprocess_table(W, backend=ref.NumpyBackend(float32=True), **settings)
    got = postprocess_table(W, backend=hip, **settings)
    assert got["Y"].dtype == np.float32 and got["Y"].shape == f64["Y"].shape
    top = np.abs(f64["Y"]).max()
    e_ref, e_hip = np.abs(f32["Y"] - f64["Y"]).max() / top, np.abs(got["Y"] - f64["Y"]).max() / top
    print("%s: NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (settings, e_ref, e_hip))
    assert e_hip <= 8 * e_ref
    assert np.abs(got["eigenvalues"] - f64["eigenvalues"]).max() <= 8 * max(
        np.abs(f32["eigenvalues"] - f64["eigenvalues"]).max(), 1e-30)


# ---- 6. end to end
def test_cli_end_to_end(hip, tmp_path):
    """`python -m trainer.postprocess` (a child process) on a job directory, then `python -m trainer.wordsim` on its
    output directory."""
    from trainer.config_utils import build_parser, init_params
    from trainer.data_utils import read_vocab
    from trainer.hip_api import DeviceTables
    from trainer.postprocess import postprocess_table
    from trainer.train_utils import CheckpointManager
    vocab = read_vocab(str(GOLDEN / "text8_cov100_ctx2_vocab.txt"))
    V = len(vocab)
    job, P = tmp_path / "job", tmp_path / "P"
    job.mkdir()
    (job / "vocab.txt").write_bytes("\n".join(vocab).encode())
    params = init_params(vars(build_parser().parse_args([
        "--vocab-txt", str(job / "vocab.txt"), "--job-dir", str(job), "--disable-datetime-path", "--embedding-size", "24",
        "--optimizer", "Adagrad"])).copy())
    W = ref.planted(seed=1, n=V)[0]
    tables = DeviceTables(V, 24, "Adagrad", device="cpu", seed=0)
    tables.embeddings("R").copy_(torch.from_numpy(W))
    tables.embeddings("C").zero_()
    CheckpointManager(params["job_dir"]).save(tables)

    proc = subprocess.run([sys.executable, "-m", "trainer.postprocess", "--job-dir", str(job), "--output-dir", str(P),
                           "--remove-components", "2", "--reduce-to", "10", "--optimizer", "Adagrad"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    blob = torch.load(P / "model.ckpt-0.pt", weights_only=False)["tables"]
    rec = json.loads((P / "postprocess.json").read_text())
    assert int(blob["global_step"]) == 0 and blob["R"].shape == (V, 10) and not blob["C"].any()
    assert rec["source_step"] == 0 and rec["embedding_size"] == 10 and len(rec["top_eigenvalues"]) == 24
    assert json.loads((P / "params.json").read_text())["embedding_size"] == 10
    f64 = postprocess_table(W, 2, 10, backend=ref.NumpyBackend())
    f32 = postprocess_table(W, 2, 10, backend=ref.NumpyBackend(float32=True))
    top = np.abs(f64["Y"]).max()
    e_ref, e_hip = np.abs(f32["Y"] - f64["Y"]).max() / top, np.abs(blob["R"].numpy() - f64["Y"]).max() / top
    print("command line: NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (e_ref, e_hip))
    assert e_hip <= 8 * e_ref

    words = [w for w in vocab if w != "<UNK>"][:11]
    ids_ = [(vocab.index(words[0]), vocab.index(w)) for w in words[1:]]
    pfile = tmp_path / "pairs.tab"
    pfile.write_text("".join("%s\t%s\t%.1f\n" % (vocab[i], vocab[j], 10 - k) for k, (i, j) in enumerate(ids_)))
    proc = subprocess.run([sys.executable, "-m", "trainer.wordsim", "--job-dir", str(P), "--pairs", str(pfile), "--no-lowercase"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    out = json.loads((P / "eval" / "wordsim.json").read_text())
    assert (out["pairs_total"], out["pairs_seen"], out["skipped"], out["global_step"]) == (10, 10, 0, 0)
