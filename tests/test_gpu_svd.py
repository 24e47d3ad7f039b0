"""libglove_factor_hip.so on the GPU (include/glove_factor_hip.h) against the float64 reference of tests/svd_ref.py: the
sparse product, the marginals and the reweighting at the smallest shapes that can go wrong, then trainer.svd's driver
and command line.

Tolerances are derived, not measured:
  - sparse product: any summation order of a row's n fma terms satisfies |got - ref| <= g sum_p |val[p]| |B[col[p], k]|
    with g = (n + 2) 2^-24 / (1 - (n + 2) 2^-24), plus 1e-30;
  - row sums: |got - ref| <= n 2^-53 sum |val| against the exactly rounded float64 sum (math.fsum);
  - reweighting: computed in double and rounded once, |got - ref| <= 2^-23 |ref| + 1e-12 (the absolute term covers an
    entry whose PMI meets the shift within double rounding);
  - driver: the deviation e_ref of the NumPy float32 backend from the NumPy float64 backend on the same input is the
    rounding level of the reference itself; the device, which sums in another order, with fma and in chunks, is
    allowed 8 e_ref from the float64 result.  Both figures are printed.

At l = 64 a workgroup holds 16 rows, which divides the 20000 rows of the Zipf case: the case `zipf_odd` has 20003.
The widths here reach three of the seven row shapes; tests/test_gpu_factor_row_shapes.py runs the product at all of them."""
import functools
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import svd_ref as ref
from trainer.hip_api import FACTOR_CHUNK as S

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
CASES = ("one", "small", "full_row", "chunk_edges", "wide", "zipf", "zipf_odd")


def csr_from_rows(rows_cols, n_cols, l, rng):
    lens = np.array([len(c) for c in rows_cols], np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = (np.concatenate(rows_cols) if lens.sum() else np.zeros(0)).astype(np.int32)
    val = rng.standard_normal(len(col)).astype(np.float32)                 # signed
    B = rng.standard_normal((n_cols, l)).astype(np.float32)
    return dict(row_ptr=row_ptr, col=col, val=val, B=B, n_rows=len(rows_cols), n_cols=n_cols, l=l, lens=lens,
                row=np.repeat(np.arange(len(rows_cols), dtype=np.int32), lens))


@functools.lru_cache(maxsize=None)
def case(name):
    """A CSR matrix, a dense operand and the float64 results every test of that matrix shares (built once, never written)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one":
        m = csr_from_rows([np.array([0])], 1, 4, rng)
    elif name == "small":                  # 0 - 9 nonzeros per row, first and last rows empty, a column twice in one row
        rows = [rng.choice(200, int(rng.integers(0, 10)), replace=False) for _ in range(300)]
        rows[0], rows[-1] = np.zeros(0, np.int64), np.zeros(0, np.int64)
        rows[7] = np.array([5, 17, 5, 3])
        m = csr_from_rows(rows, 200, 8, rng)
    elif name == "full_row":               # one row with all 5,000 columns among rows of 0 - 3
        rows = [rng.choice(5000, int(rng.integers(0, 4)), replace=False) for _ in range(64)]
        rows[20] = rng.permutation(5000)
        m = csr_from_rows(rows, 5000, 52, rng)
    elif name == "chunk_edges":            # around the chunk length: one chunk, exactly one, two, three
        m = csr_from_rows([rng.choice(1100, n, replace=False) for n in (S - 1, S, S + 1, 2 * S + 1)], 1100, 312, rng)
    elif name == "wide":
        m = csr_from_rows([rng.choice(130, int(rng.integers(0, 20)), replace=False) for _ in range(130)], 130, 1024, rng)
    else:                                  # Zipf row lengths and Zipf columns, about 2 10^5 nonzeros
        n = 20000 if name == "zipf" else 20003
        lens = np.minimum(19000 // np.arange(1, n + 1), 20000)
        p = 1.0 / np.arange(1, 20001)
        cols = rng.choice(20000, int(lens.sum()), p=p / p.sum())
        m = csr_from_rows(np.split(cols, np.cumsum(lens)[:-1]), 20000, 64, rng)
    A = sp.csr_matrix((m["val"].astype(np.float64), m["col"], m["row_ptr"]), shape=(m["n_rows"], m["n_cols"]))
    m["Y"] = np.asarray(A @ m["B"].astype(np.float64))
    absA = sp.csr_matrix((np.abs(m["val"]).astype(np.float64), m["col"], m["row_ptr"]), shape=A.shape)
    n2 = (m["lens"] + 2) * 2.0 ** -24
    m["Y_bound"] = (n2 / (1 - n2))[:, None] * np.asarray(absA @ np.abs(m["B"]).astype(np.float64)) + 1e-30
    return m


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


# ---- 7. the sparse product
@pytest.mark.parametrize("name", CASES)
def test_spmm_parity_with_the_float64_reference(hip, name):
    m = case(name)
    args = (dev(m["row_ptr"]), dev(m["col"]), dev(m["val"]), m["n_rows"], m["n_cols"], dev(m["B"]))
    got = hip.csr_spmm(*args)
    assert got.shape == (m["n_rows"], m["l"]) and got.dtype == torch.float32
    g = got.cpu().numpy().astype(np.float64)
    err = np.abs(g - m["Y"])
    print("%s: %d x %d, l = %d, nnz = %d, longest row %d: largest error / bound %.3g" % (
        name, m["n_rows"], m["n_cols"], m["l"], len(m["val"]), m["lens"].max(), (err / m["Y_bound"]).max()))
    assert (err <= m["Y_bound"]).all()
    empty = m["lens"] == 0
    assert (g[empty] == 0.0).all()                          # written by the kernel itself, into torch.empty memory
    assert torch.equal(got, hip.csr_spmm(*args))            # bitwise repeatable


def test_spmm_rows_do_not_depend_on_the_other_rows(hip):
    """The bits of a row are a function of that row alone: the last two rows of the chunk-edge matrix, cut out."""
    m = case("chunk_edges")
    whole = hip.csr_spmm(dev(m["row_ptr"]), dev(m["col"]), dev(m["val"]), 4, m["n_cols"], dev(m["B"]))
    a = int(m["row_ptr"][2])
    part = hip.csr_spmm(dev(m["row_ptr"][2:] - a), dev(m["col"][a:]), dev(m["val"][a:]), 2, m["n_cols"], dev(m["B"]))
    assert torch.equal(whole[2:], part)


def test_spmm_refuses_what_the_header_excludes(hip):
    from trainer.hip_api import GloveHipError
    m = case("small")
    rp, col, val, B = dev(m["row_ptr"]), dev(m["col"]), dev(m["val"]), dev(m["B"])
    with pytest.raises(GloveHipError):
        hip.csr_spmm(rp, col, val, 300, 200, B[:, :6].contiguous())          # l % 4 != 0
    with pytest.raises(GloveHipError):
        hip.csr_spmm(rp, col.long(), val, 300, 200, B)
    with pytest.raises(GloveHipError):
        hip.csr_spmm(rp[:-1].contiguous(), col, val, 300, 200, B)
    with pytest.raises(GloveHipError):
        hip.csr_spmm(rp, col, val, 300, 200, B[:100].contiguous())
    with pytest.raises(GloveHipError, match="GLOVE_E_WORKSPACE"):
        hip.csr_spmm(rp, col, val, 300, 200, B, ws=torch.empty(16, dtype=torch.uint8, device="cuda:0"))


# ---- 8. the marginals
@pytest.mark.parametrize("name", CASES)
def test_row_sums_against_exactly_rounded_sums(hip, name):
    m = case(name)
    rp, val = dev(m["row_ptr"]), dev(m["val"])
    got = hip.csr_row_sums(rp, val, m["n_rows"])
    assert got.shape == (m["n_rows"],) and got.dtype == torch.float64
    v = m["val"].astype(np.float64)
    want = np.array([math.fsum(v[a:b]) for a, b in zip(m["row_ptr"][:-1], m["row_ptr"][1:])])
    bound = m["lens"] * 2.0 ** -53 * np.add.reduceat(np.r_[np.abs(v), 0.0], m["row_ptr"][:-1]) * (m["lens"] > 0)
    assert (np.abs(got.cpu().numpy() - want) <= bound).all()
    assert torch.equal(got, hip.csr_row_sums(rp, val, m["n_rows"]))


# ---- 9. the reweighting
@pytest.mark.parametrize("name", CASES)
def test_reweight_every_kind(hip, name):
    """x = the matrix's signed values (the negative ones give 0); the marginals are those of |x|, so that they are positive."""
    m = case(name)
    x = m["val"]
    absx = np.abs(x).astype(np.float64)
    rs = np.bincount(m["row"], weights=absx, minlength=m["n_rows"])
    cs = np.bincount(m["col"], weights=absx, minlength=m["n_cols"])
    row, col, xd = dev(m["row"]), dev(m["col"]), dev(x)
    settings = [("none", 1, 1), ("sqrt", 1, 1), ("log1p", 1, 1)] + [("ppmi", cds, shift) for cds in (1, 0.75) for shift in (1, 5)]
    for kind, cds, shift in settings:
        cw = cs ** cds
        total, log_shift = float(cw.sum()), math.log(shift)
        want = ref.reweight(m["row"], m["col"], x, kind, rs, cw, total, log_shift)
        got = hip.coo_reweight(row, col, xd, kind, dev(rs), dev(cw), total, log_shift)
        g = got.cpu().numpy()
        assert got.dtype == torch.float32 and (g[x <= 0] == 0.0).all()
        assert (np.abs(g.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 1e-12).all(), (kind, cds, shift)
        alias = xd.clone()
        assert hip.coo_reweight(row, col, alias, kind, dev(rs), dev(cw), total, log_shift, out=alias) is alias
        assert torch.equal(alias, got)                      # val_out == val_in: the same bits
    if name == "small":
        assert hip.coo_reweight(row, col, xd, "sqrt").shape == xd.shape      # marginals are read by ppmi only


# ---- 10. the driver
def deviation(out, base, dense=None):
    """The quantities that do not depend on rotations inside the subspace, relative to `base`'s."""
    s, s0 = out["singular_values"], base["singular_values"]
    G, G0 = (x["R"].astype(np.float64) @ x["R"].astype(np.float64).T for x in (out, base))
    dev_ = {"singular_values": np.abs(s - s0).max() / s0[0], "R R^T": np.linalg.norm(G - G0) / np.linalg.norm(G0)}
    if dense is not None:
        rec = (out["R"].astype(np.float64) @ out["C"].astype(np.float64).T)[:, :dense.shape[1]]
        dev_["reconstruction"] = np.linalg.norm(rec - dense) / np.linalg.norm(dense)
    return dev_


def compare_backends(hip, what, row, col, val, dense=None, on_device=False, **settings):
    from trainer.svd import svd_embeddings
    f64 = svd_embeddings(row, col, val, backend=ref.NumpyBackend(), **settings)
    f32 = svd_embeddings(row, col, val, backend=ref.NumpyBackend(float32=True), **settings)
    table = (dev(row), dev(col), dev(val)) if on_device else (row, col, val)
    got = svd_embeddings(*table, backend=hip, **settings)
    assert got["R"].dtype == np.float32 and got["nnz_reweighted"] == f64["nnz_reweighted"]
    e_ref, e_hip = deviation(f32, f64, dense), deviation(got, f64, dense)
    if dense is not None:                  # the float64 result's own reconstruction error is not the device's
        base = deviation(f64, f64, dense)["reconstruction"]
        assert base <= 1e-10
    for key in e_ref:
        print("%s, %s: NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (what, key, e_ref[key], e_hip[key]))
    for key in e_ref:
        assert e_hip[key] <= 8 * e_ref[key], key


@pytest.mark.parametrize("power_iterations", [0, 2])
def test_driver_on_the_planted_matrix(hip, power_iterations):
    row, col, val, M, sv = ref.planted_matrix()
    compare_backends(hip, "planted, %d power iterations" % power_iterations, row, col, val, dense=M, on_device=power_iterations == 2,
                     V=700, d=12, transform="none", oversample=4, power_iterations=power_iterations)


def test_driver_on_the_golden_ppmi_table(hip):
    row, col, val, V = ref.golden_cooccurrence()
    compare_backends(hip, "golden PPMI", row, col, val, V=V, d=8, oversample=8, power_iterations=4)


# ---- 11. end to end
def test_cli_end_to_end(hip, tmp_path):
    """`python -m trainer.svd` (a child process), `python -m trainer.wordsim` on its job directory, then
    trainer.estimator continuing from the SVD vectors."""
    from trainer import estimator
    from trainer.data_utils import load_interaction_csv, read_vocab
    from trainer.svd import svd_embeddings
    csv, vocab_txt = GOLDEN / "text8_cov100_ctx2_interaction.csv", GOLDEN / "text8_cov100_ctx2_vocab.txt"
    job = tmp_path / "job"
    shared = ["--train-csv", str(csv), "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--embedding-size", "8",
              "--optimizer", "Adagrad"]
    proc = subprocess.run([sys.executable, "-m", "trainer.svd"] + shared, cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    blob = torch.load(job / "model.ckpt-0.pt", weights_only=False)["tables"]
    assert int(blob["global_step"]) == 0 and len(json.loads((job / "svd.json").read_text())["singular_values"]) == 8

    vocab = read_vocab(str(vocab_txt))
    words = [w for w in vocab if w != "<UNK>"][:11]
    ids = [(vocab.index(words[0]), vocab.index(w)) for w in words[1:]]
    pfile = tmp_path / "pairs.tab"
    pfile.write_text("".join("%s\t%s\t%.1f\n" % (vocab[i], vocab[j], 10 - k) for k, (i, j) in enumerate(ids)))
    proc = subprocess.run([sys.executable, "-m", "trainer.wordsim", "--job-dir", str(job), "--pairs", str(pfile), "--no-lowercase"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    rec = json.loads((job / "eval" / "wordsim.json").read_text())
    assert (rec["pairs_total"], rec["pairs_seen"], rec["skipped"], rec["global_step"]) == (10, 10, 0, 0)

    # the pairs' cosines: a function of R R^T.  e_ref is the NumPy float32 driver's largest deviation from the float64
    # one over ALL pairs of words (the rounding level of the whole table, not of ten lucky pairs)
    coo = load_interaction_csv(str(csv), str(vocab_txt), target_name="value")

    def cosines(R):
        R = R.astype(np.float64)
        U = R / np.sqrt(np.maximum((R * R).sum(axis=1, keepdims=True), 1e-12))
        return U @ U.T
    c64, c32 = (cosines(svd_embeddings(coo["row"], coo["col"], coo["y"], len(vocab), 8, backend=ref.NumpyBackend(f))["R"])
                for f in (False, True))
    got = cosines(blob["R"].numpy())
    e_ref = np.abs(c32 - c64).max()
    e_hip = max(abs(got[i, j] - c64[i, j]) for i, j in ids)
    print("cosines of the ten pairs: NumPy float32 from float64 (all pairs) %.3g, HIP from float64 %.3g" % (e_ref, e_hip))
    assert e_hip <= 8 * e_ref

    estimator.main(shared + ["--disable-datetime-path", "--learning-rate", "0.05", "--batch-size", "64", "--train-steps", "4",
                             "--log-every", "2", "--seed", "7", "--skip-eval"])
    after = torch.load(job / "model.ckpt-4.pt", weights_only=False)["tables"]
    assert int(after["global_step"]) == 4
    moved = np.abs(after["R"].numpy() - blob["R"].numpy()).max()
    # continued from the SVD vectors, not from a fresh init: an Adagrad step moves an entry by less than the learning rate
    assert np.abs(blob["R"].numpy()).max() > 0.5 and 0 < moved <= 4 * 0.05
