"""The kernels behind trainer.align on the GPU (include/glove_factor_align_hip.h, include/glove_eval_cross_hip.h) against
the float64 reference of tests/align_ref.py, bit for bit against the one-table kernels they extend, then the driver and
the command lines.

Cross-covariance.  n = 1, CHUNK - 1, CHUNK, CHUNK + 1, SLICE, SLICE + 1, 2 SLICE + 7 pairs (one pair; around the end of a
float32 chain; around the end of a float64 slice; three slices, the last of 7 pairs) times (row stride, model columns) =
(4, 4), (36, 36), (64, 64), (304, 300), ids drawn at random from Vx = 700 and Vy = 900 rows (so they repeat), with and
without scales.  The bound is derived like tests/test_gpu_postprocess.py's: a chunk is a float32 fmaf chain of at most
CHUNK terms, |got - ref| <= g(CHUNK) sum_p |x~_pi y~_pj| + 1e-30 with g(k) = (k + 2) u / (1 - (k + 2) u), u = 2^-24 (the
float64 combination adds at most n / CHUNK 2^-53 of that sum, which g's two spare terms cover); the reference takes x~
as the float32 product, like the kernel.

Cross top-k.  (Vq, Vt, d, k, n) = (200, 64, 8, 5, 40), (300, 129, 36, 10, 129), (500, 4097, 64, 10, 257), (1000, 8193,
304 holding 300, 10, 128), (700, 40003, 52, 20, 130): across a query tile of 128, a target tile of 128, a k-slab edge and
one, two and ten top-k segments of 4,096.  Scores by cosine: rtol 1e-5, atol 1e-6 (tests/test_gpu_analogy.py).  Scores by
CSLS: twice that plus 2^-22 (the score doubles the cosine's error and rounds twice more at a magnitude of at most 4); the
reference gets the same penalty arrays as the kernel.  Ids are compared wherever the reference's score is at least GAP
(1e-5 by cosine, 2e-5 by CSLS) away from both neighbours in its ranking; the share left out is capped at 2 %, which is
asserted on the reference before anything is compared.

Driver: the deviation e_ref of the NumPy float32 backend from the NumPy float64 backend on the same input is the rounding
level of the reference itself; the device is allowed 8 e_ref from the float64 result.  Both are printed."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import align_ref as ref
from analogy_ref import separated
from trainer.hip_api import GRAM_CHUNK as CHUNK, GRAM_SLICE as SLICE

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
U = 2.0 ** -24
ROWS = (1, CHUNK - 1, CHUNK, CHUNK + 1, SLICE, SLICE + 1, 2 * SLICE + 7)
WIDTHS = ((4, 4), (36, 36), (64, 64), (304, 300))            # (row stride, the model's columns)
GRAM_SHAPES = [(n, d, dm) for d, dm in WIDTHS for n in ROWS]
VX, VY = 700, 900
RTOL, ATOL, LEFT_OUT_MAX = 1e-5, 1e-6, 0.02
GAP = {"nn": 1e-5, "csls": 2e-5}
TOPK_CASES = [(200, 64, 8, 8, 5, 40), (300, 129, 36, 36, 10, 129), (500, 4097, 64, 64, 10, 257), (1000, 8193, 304, 300, 10, 128),
              (700, 40003, 52, 52, 20, 130)]                 # (Vq, Vt, row stride, model columns, k, n)
KNN = 10


def g(k):
    return (k + 2) * U / (1 - (k + 2) * U)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def padded(W, d):
    out = np.zeros((W.shape[0], d), np.float32)
    out[:, :W.shape[1]] = W
    return out


# ---- 1. the cross-covariance
@functools.lru_cache(maxsize=None)
def gram_case(n, d, d_model):
    """Two tables, id lists, scales and the float64 results every test of that shape shares (built once, never written)."""
    rng = np.random.default_rng(1000003 * d + n)
    X = padded(rng.standard_normal((VX, d_model)) + rng.uniform(-2.0, 2.0, d_model), d)
    Y = padded(rng.standard_normal((VY, d_model)) + rng.uniform(-2.0, 2.0, d_model), d)
    xid, yid = rng.integers(0, VX, n).astype(np.int32), rng.integers(0, VY, n).astype(np.int32)
    xs, ys = rng.uniform(0.5, 2.0, VX).astype(np.float32), rng.uniform(0.5, 2.0, VY).astype(np.float32)
    c = dict(X=X, Y=Y, xid=xid, yid=yid, xs=xs, ys=ys)
    for key, sc in (("scaled", (xs, ys)), ("plain", (None, None))):
        c[key] = ref.cross_gram(X, xid, Y, yid, *sc)
        c[key + "_bound"] = g(CHUNK) * ref.cross_gram_magnitude(X, xid, Y, yid, *sc) + 1e-30
    return c


def gram_id(shape):
    return "n%d-d%d" % shape[:2]


@pytest.mark.parametrize("shape", GRAM_SHAPES, ids=gram_id)
def test_cross_gram_parity_padding_and_repeatability(hip, shape):
    n, d, d_model = shape
    c = gram_case(*shape)
    X, Y, xid, yid = dev(c["X"]), dev(c["Y"]), dev(c["xid"]), dev(c["yid"])
    for key, scales in (("scaled", (dev(c["xs"]), dev(c["ys"]))), ("plain", (None, None))):
        got = hip.cross_gram(X, xid, Y, yid, *scales)
        assert got.shape == (d, d) and got.dtype == torch.float64
        M = got.cpu().numpy()
        err = np.abs(M - c[key])
        print("%s, %s: largest error / bound %.3g" % (gram_id(shape), key, (err / c[key + "_bound"]).max()))
        assert (err <= c[key + "_bound"]).all()
        assert (M[d_model:] == 0.0).all() and (M[:, d_model:] == 0.0).all()       # padding: exact zeros (d = 304: 300 ..)
        assert torch.equal(got, hip.cross_gram(X, xid, Y, yid, *scales))           # bitwise repeatable
    # one scale without the other: each operand on its own
    got = hip.cross_gram(X, xid, Y, yid, dev(c["xs"]), None).cpu().numpy()
    want = ref.cross_gram(c["X"], c["xid"], c["Y"], c["yid"], c["xs"], None)
    assert (np.abs(got - want) <= g(CHUNK) * ref.cross_gram_magnitude(c["X"], c["xid"], c["Y"], c["yid"], c["xs"], None) + 1e-30).all()


@pytest.mark.parametrize("d, d_model", [(36, 36), (304, 300)])
def test_cross_gram_of_a_table_with_itself_has_the_gram_matrix_bits(hip, d, d_model):
    """Y = X, identity ids, null scales: glove_gram_f64's chains, the lower triangle too (fmaf commutes)."""
    n = 2 * SLICE + 7
    rng = np.random.default_rng(d)
    X = dev(padded(rng.standard_normal((n, d_model)) + 1.5, d))
    ids = torch.arange(n, dtype=torch.int32, device="cuda:0")
    got = hip.cross_gram(X, ids, X, ids)
    assert torch.equal(got, hip.gram(X, None))
    assert torch.equal(got, got.T)
    # a scale of exactly 1 multiplies nothing away
    ones = torch.ones(n, device="cuda:0")
    assert torch.equal(got, hip.cross_gram(X, ids, X, ids, ones, ones))


@pytest.mark.parametrize("d, d_model", [(36, 36), (304, 300)])
@pytest.mark.parametrize("prefix", [CHUNK, SLICE], ids=["chunk", "slice"])
def test_cross_gram_bits_are_those_of_the_chunks_and_slices(hip, prefix, d, d_model):
    """Pairs whose source row is zero beyond the first chunk (the first slice) add exact zeros: the bits are the prefix's
    alone, however many chunks, slices and workgroups the call had."""
    n = 2 * SLICE + 7
    c = gram_case(n, d, d_model)
    X = c["X"].copy()
    X[0] = 0.0
    xid = np.where(c["xid"] == 0, 1, c["xid"]).astype(np.int32)               # row 0 is the zero row: nobody's before the prefix ends
    xid[prefix:] = 0
    X, Y, xid, yid = dev(X), dev(c["Y"]), dev(xid), dev(c["yid"])
    whole = hip.cross_gram(X, xid, Y, yid)
    assert torch.equal(whole, hip.cross_gram(X, xid[:prefix].contiguous(), Y, yid[:prefix].contiguous()))
    assert torch.equal(whole, hip.cross_gram(X, xid[:prefix + CHUNK + 3].contiguous(), Y, yid[:prefix + CHUNK + 3].contiguous()))


def test_cross_gram_chunk_partials_are_float32_chains(hip):
    """One chunk: the fmaf chain of the header, pair by pair, on the float32 products x~ and y~ (the restatement rounds
    a b + s to float64 and then to float32: one float32 ulp is allowed for the ties, as in tests/test_gpu_postprocess.py)."""
    c = gram_case(CHUNK, 4, 4)
    got = hip.cross_gram(dev(c["X"]), dev(c["xid"]), dev(c["Y"]), dev(c["yid"]), dev(c["xs"]), dev(c["ys"])).cpu().numpy()
    a, b = ref.scaled_rows(c["X"], c["xid"], c["xs"]), ref.scaled_rows(c["Y"], c["yid"], c["ys"])
    assert a.dtype == np.float32 and b.dtype == np.float32
    for i, j in ((0, 0), (0, 3), (2, 1), (3, 0)):
        s = np.float32(0.0)
        for p in range(CHUNK):
            s = np.float32(np.float64(a[p, i]) * np.float64(b[p, j]) + np.float64(s))
        assert got[i, j] == np.float32(got[i, j])             # a single chunk: M is a float32 number
        assert abs(got[i, j] - np.float64(s)) <= np.spacing(np.float32(abs(s)))


# ---- 2. neighbours across two tables
@functools.lru_cache(maxsize=None)
def topk_case(Vq, Vt, d, d_model, k, n):
    """Two tables, query ids, the penalties and the reference rankings with one rank behind the k-th (built once)."""
    rng = np.random.default_rng(1000 + Vq + Vt + d)
    Q = rng.standard_normal((Vq, d_model)).astype(np.float32)
    T = rng.standard_normal((Vt, d_model)).astype(np.float32)
    qid = rng.choice(Vq, n).astype(np.int32)
    q_pen = ref.csls_penalty(Q, qid, T, KNN)                  # the float32 means of the 10 best cosines each way
    t_pen = ref.csls_penalty(T, np.arange(Vt), Q, KNN)
    extra = 1 if k < Vt else 0
    c = dict(Q=padded(Q, d), T=padded(T, d), qid=qid, q_pen=q_pen, t_pen=t_pen)
    c["nn"] = ref.topk(Q, qid, T, k, extra=extra)
    c["csls"] = ref.topk(Q, qid, T, k, q_pen, t_pen, extra=extra)
    return c


def topk_id(case):
    return "Vq%d-Vt%d-d%d-k%d-n%d" % (case[0], case[1], case[2], case[4], case[5])


@pytest.mark.parametrize("method", ["nn", "csls"])
@pytest.mark.parametrize("case", TOPK_CASES, ids=topk_id)
def test_cross_topk_parity(hip, case, method):
    Vq, Vt, d, d_model, k, n = case
    c = topk_case(*case)
    want_s_ext, want_i_ext = c[method]
    want_s, want_i = want_s_ext[:, :k], want_i_ext[:, :k]
    # the condition on the reference itself, before anything is compared
    clear = separated(want_s_ext, k, GAP[method])
    left_out = 1.0 - clear.mean()
    print("%s, %s: %.2f %% of the positions left out of the id comparison" % (topk_id(case), method, 100 * left_out))
    assert left_out <= LEFT_OUT_MAX
    pens = (dev(c["q_pen"]), dev(c["t_pen"])) if method == "csls" else (None, None)
    got_s, got_i = hip.cross_topk(dev(c["Q"]), dev(c["qid"]), dev(c["T"]), k, *pens)
    assert got_s.shape == (n, k) and got_s.dtype == torch.float32 and got_i.dtype == torch.int32
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    print("%s, %s: largest score deviation %.3g" % (topk_id(case), method, np.abs(got_s - want_s).max()))
    if method == "nn":
        np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=ATOL)
    else:
        assert (np.abs(got_s - want_s) <= 2 * (ATOL + RTOL * np.abs(want_s)) + 2.0 ** -22).all()
    assert (np.diff(got_s, axis=1) <= 0).all()                # descending
    assert ((got_i >= 0) & (got_i < Vt)).all()
    assert (got_i[clear] == want_i[clear]).all()


@pytest.mark.parametrize("V, d, k, n", [(500, 64, 10, 257), (40003, 52, 20, 130)], ids=["V500-d64", "V40003-d52"])
def test_cross_topk_of_a_table_with_itself_has_predicts_bits(hip, V, d, k, n):
    rng = np.random.default_rng(V + d)
    R = dev(rng.standard_normal((V, d)).astype(np.float32))
    qid = dev(rng.choice(V, n).astype(np.int32))
    want = hip.topk_cosine(R, qid, k)
    got = hip.cross_topk(R, qid, R, k)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a query's result does not depend on its batch
    small = hip.cross_topk(R, qid, R, k, batch=128)
    assert torch.equal(small[0], got[0]) and torch.equal(small[1], got[1])
    q_pen, t_pen = hip.csls_penalty(R, qid, R, KNN), torch.rand(V, device="cuda:0")
    a, b = hip.cross_topk(R, qid, R, k, q_pen, t_pen, batch=128), hip.cross_topk(R, qid, R, k, q_pen, t_pen, batch=1024)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and the CSLS score is the header's arithmetic on the cosine's bits: every rank of one small call
    cos, idx = hip.cross_topk(R, qid[:7].contiguous(), R, min(V, 1024))
    s, i = hip.cross_topk(R, qid[:7].contiguous(), R, min(V, 1024), q_pen[:7].contiguous(), t_pen)
    cos_at = {(q, v): c for q in range(7) for v, c in zip(idx[q].tolist(), cos[q].cpu().numpy())}
    qp, tp, s, i = q_pen.cpu().numpy(), t_pen.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()
    seen = 0
    for q in range(7):
        for r in range(s.shape[1]):
            v = int(i[q, r])
            if (q, v) in cos_at:
                want_s = np.float32(np.float32(np.float32(2.0) * cos_at[(q, v)]) - qp[q]) - tp[v]
                assert s[q, r] == np.float32(want_s)
                seen += 1
    assert seen >= 7 * 20


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_topk_mean_is_the_sequential_float32_sum(hip, k):
    rng = np.random.default_rng(k)
    sims = np.sort(rng.uniform(-1.0, 1.0, (301, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    got = hip.topk_mean(dev(sims))
    assert got.shape == (301,) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), ref.topk_mean(sims))
    empty = hip.topk_mean(torch.empty(0, k, device="cuda:0"))
    assert empty.shape == (0,)


def test_csls_penalty_is_the_mean_of_the_best_cosines(hip):
    c = topk_case(*TOPK_CASES[1])
    Q, T, qid = dev(c["Q"]), dev(c["T"]), dev(c["qid"])
    got = hip.csls_penalty(Q, qid, T, KNN)
    assert torch.equal(got, hip.topk_mean(hip.cross_topk(Q, qid, T, KNN)[0]))
    np.testing.assert_allclose(got.cpu().numpy(), c["q_pen"], rtol=RTOL, atol=ATOL)


def test_refusals_leave_the_outputs_alone(hip):
    from trainer.hip_api import GloveHipError, load_eval_library, load_factor_library
    ev, fa = load_eval_library(), load_factor_library()
    c = topk_case(*TOPK_CASES[0])
    Q, T, qid = dev(c["Q"]), dev(c["T"]), dev(c["qid"])
    n, k, (Vq, d), Vt = len(c["qid"]), 5, c["Q"].shape, c["T"].shape[0]
    st = torch.cuda.current_stream().cuda_stream
    sims = torch.full((n, k), -7.0, device="cuda:0")
    idx = torch.full((n, k), -7, dtype=torch.int32, device="cuda:0")
    M = torch.full((d, d), -7.0, dtype=torch.float64, device="cuda:0")
    pen = torch.zeros(Vt, device="cuda:0")
    ws = torch.empty(max(ev.glove_cross_topk_workspace_bytes(n, Vt, d, k), fa.glove_cross_gram_workspace_bytes(n, d)),
                     dtype=torch.uint8, device="cuda:0")
    p = lambda t: t.data_ptr()
    assert ev.glove_cross_topk_f32(p(Q), Vq, p(qid), n, p(T), Vt, d, k, p(pen), None, p(sims), p(idx), p(ws), ws.numel(), st) == -1
    assert ev.glove_cross_topk_f32(p(Q), Vq, p(qid), n, p(T), Vt, d, Vt + 1, None, None, p(sims), p(idx), p(ws), ws.numel(), st) == -1
    assert ev.glove_cross_topk_f32(p(Q), Vq, p(qid), n, p(T), Vt, d, k, None, None, p(sims), p(idx), p(ws), 255, st) == -2
    assert fa.glove_cross_gram_f64(p(Q), Vq, p(T), Vt, d, p(qid), p(qid), n, None, None, p(M), p(ws), 255, st) == -2
    assert fa.glove_cross_gram_f64(p(Q), Vq, p(T), Vt, d, p(qid), p(qid), 0, None, None, p(M), p(ws), ws.numel(), st) == -1
    torch.cuda.synchronize()
    assert (sims == -7.0).all() and (idx == -7).all() and (M == -7.0).all()      # nothing ran
    # ... and the binding's own checks
    with pytest.raises(GloveHipError):
        hip.cross_topk(Q, qid, T, k, q_pen=torch.zeros(n, device="cuda:0"))
    with pytest.raises(GloveHipError):
        hip.cross_topk(Q, qid.long(), T, k)
    with pytest.raises(GloveHipError):
        hip.cross_topk(Q, qid, T[:, :4].contiguous(), k)
    with pytest.raises(GloveHipError, match="GLOVE_E_BADARG"):
        hip.cross_topk(Q, qid, T, Vt + 1)
    with pytest.raises(GloveHipError):
        hip.cross_gram(Q, qid, T, qid[:5].contiguous())
    with pytest.raises(GloveHipError):
        hip.cross_gram(Q, qid, T, qid, x_scale=torch.ones(Vq + 1, device="cuda:0"))
    with pytest.raises(GloveHipError, match="GLOVE_E_WORKSPACE"):
        hip.cross_gram(Q, qid, T, qid, ws=torch.empty(16, dtype=torch.uint8, device="cuda:0"))
    with pytest.raises(GloveHipError):
        hip.topk_mean(torch.zeros(4, device="cuda:0"))


# ---- 3. the driver
def identity_pairs(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.int32)


@pytest.mark.parametrize("normalize", ["unit", "none"])
def test_driver_on_the_planted_rotation(hip, normalize):
    from trainer.align import align_tables
    X, Y, Q = ref.planted_rotation(noise=0.1)                # V = 500, d = 20, 200 anchors
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    f64 = align_tables(X, Y, identity_pairs(200), normalize=normalize, backend=ref.NumpyBackend())
    f32 = align_tables(X, Y, identity_pairs(200), normalize=normalize, backend=ref.NumpyBackend(float32=True))
    got = align_tables(X, Y, identity_pairs(200), normalize=normalize, backend=hip)
    assert got["W"].dtype == np.float32 and got["W"].shape == (20, 20) and got["Y"].shape == (500, 20)
    e_ref, e_hip = np.abs(f32["W"] - f64["W"]).max(), np.abs(got["W"] - f64["W"]).max()
    print("%s: W, NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (normalize, e_ref, e_hip))
    assert e_hip <= 8 * e_ref
    top = np.abs(f64["Y"]).max()
    y_ref, y_hip = np.abs(f32["Y"] - f64["Y"]).max() / top, np.abs(got["Y"] - f64["Y"]).max() / top
    print("%s: mapped rows, NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (normalize, y_ref, y_hip))
    assert y_hip <= 8 * y_ref
    assert got["orthogonality_defect"] <= 64 * U and np.abs(got["W"] - Q).max() < 0.1
    assert abs(got["anchor_cosine_after"] - f64["anchor_cosine_after"]) <= 1e-5


def test_driver_refines_a_planted_permutation(hip):
    from trainer.align import align_tables, translation_precision
    X, _, Q = ref.planted_rotation(seed=3, V=300, d=20)
    perm = np.random.default_rng(5).permutation(300)
    Y = np.empty_like(X)
    Y[perm] = X @ Q.T
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    seed_pairs = np.stack([np.arange(12), perm[:12]], axis=1)
    out = align_tables(X, Y, seed_pairs, refine=3, refine_vocab=300, backend=hip)
    print("dictionary sizes per round:", out["dictionary_sizes"])
    assert out["dictionary_sizes"][-1] == 300 and np.abs(out["W"] - Q).max() <= 1e-5
    full = np.stack([np.arange(300), perm], axis=1)
    for method in ("nn", "csls"):
        assert translation_precision(out["Y"], Y, full, method=method, top_k=(1,), backend=hip)["precision"][1] == 1.0
    # the hub case: the device gives the reference's two figures
    A, T, pairs = ref.hub_case()
    A, T = A.astype(np.float32), T.astype(np.float32)
    for method in ("nn", "csls"):
        want = ref.precision_at(A, T, pairs, (1, 5), method, knn=KNN)
        assert translation_precision(A, T, pairs, method=method, knn=KNN, top_k=(1, 5), backend=hip)["precision"] == want
    assert ref.precision_at(A, T, pairs, (1,), "csls")[1] > ref.precision_at(A, T, pairs, (1,), "nn")[1]


# ---- 4. end to end
def test_cli_end_to_end(hip, tmp_path):
    """`python -m trainer.align fit`, then `eval --method csls` (child processes) on two tiny job directories."""
    from trainer.align import align_tables
    from trainer.postprocess import write_step0_job_dir
    rng = np.random.default_rng(11)
    X, _, Q = ref.planted_rotation(seed=4, V=120, d=12)
    perm = rng.permutation(139)[:120]
    Y = rng.standard_normal((140, 12))
    Y[perm] = X @ Q.T + 0.05 * rng.standard_normal((120, 12))
    X, Y = X.astype(np.float32), Y.astype(np.float32)
    vocab_s = ["<UNK>"] + ["s%03d" % i for i in range(1, 120)]
    vocab_t = ["t%03d" % i for i in range(139)] + ["<UNK>"]
    S, T, A = tmp_path / "S", tmp_path / "T", tmp_path / "A"
    write_step0_job_dir(S, vocab_s, X, "Adagrad", {})
    write_step0_job_dir(T, vocab_t, Y, "Adagrad", {})
    (tmp_path / "train.txt").write_text("".join("%s %s\n" % (vocab_s[i], vocab_t[perm[i]]) for i in range(1, 60)) + "nobody t000\n")
    (tmp_path / "test.txt").write_text("".join("%s %s\n" % (vocab_s[i], vocab_t[perm[i]]) for i in range(60, 120)) + "s060 nothing\n")

    proc = subprocess.run([sys.executable, "-m", "trainer.align", "fit", "--source-dir", str(S), "--target-dir", str(T),
                           "--output-dir", str(A), "--dictionary", str(tmp_path / "train.txt"), "--optimizer", "Adagrad"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    blob = torch.load(A / "model.ckpt-0.pt", weights_only=False)["tables"]
    rec = json.loads((A / "align.json").read_text())
    assert int(blob["global_step"]) == 0 and blob["R"].shape == (120, 12) and not blob["C"].any()
    assert (rec["anchors_used"], rec["anchors_skipped"], rec["source_step"], rec["embedding_size"]) == (59, 1, 0, 12)
    assert len(rec["top_singular_values"]) == 12 and rec["orthogonality_defect"] <= 64 * U
    assert rec["anchor_cosine_after"] > 0.95 > rec["anchor_cosine_before"]
    pairs = np.stack([np.arange(1, 60), perm[1:60]], axis=1)
    f64 = align_tables(X, Y, pairs, backend=ref.NumpyBackend())
    f32 = align_tables(X, Y, pairs, backend=ref.NumpyBackend(float32=True))
    top = np.abs(f64["Y"]).max()
    e_ref, e_hip = np.abs(f32["Y"] - f64["Y"]).max() / top, np.abs(blob["R"].numpy() - f64["Y"]).max() / top
    print("command line: NumPy float32 from float64 %.3g, HIP from float64 %.3g" % (e_ref, e_hip))
    assert e_hip <= 8 * e_ref

    proc = subprocess.run([sys.executable, "-m", "trainer.align", "eval", "--source-dir", str(A), "--target-dir", str(T),
                           "--dictionary", str(tmp_path / "test.txt"), "--method", "csls", "--knn", "7", "--top-k", "1", "5"],
                          cwd=str(REPO), capture_output=True, text=True, timeout=240)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    bli = json.loads((A / "eval" / "bli.json").read_text())
    test_pairs = [[i, perm[i]] for i in range(60, 120)]
    want = ref.precision_at(blob["R"].numpy(), Y, test_pairs, (1, 5), "csls", knn=7)       # the reference scorer on what was written
    assert bli["precision"] == {str(k): v for k, v in want.items()} and bli["precision"]["1"] >= 0.9
    assert (bli["queries"], bli["pairs"], bli["pairs_skipped"], bli["method"], bli["knn"]) == (60, 60, 1, "csls", 7)
