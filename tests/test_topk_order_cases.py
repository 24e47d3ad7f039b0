"""The cases of tests/test_gpu_topk_order.py, proved on the float64 references alone (no GPU): the groups of every
query are GROUP_GAP apart, the expected ranking is the references' own on the same table, and no position is left out."""
import numpy as np
import pytest

import analogy_ref
import cosmul_ref
import glove_ref as ref
import topk_order_cases as toc

CASE_PATHS = [(s.name, p) for s in toc.SPECS for p in toc.runs(s.name)]


def reference_topk(case, path, k):
    """(scores, ids) [n, k] of the project's float64 reference of the path on the case's own table."""
    W = case["W"].astype(np.float64)
    if path == "predict":
        with np.errstate(invalid="ignore"):                 # non-finite rows score NaN, which a sort puts last
            return ref.cosine_topk(W, case["queries"], k)
    if path == "cosadd":
        return analogy_ref.topk(W, case["abc"], k)
    return cosmul_ref.topk(W, case["abc"], k, toc.COSMUL_EPS)


def test_the_cases_are_the_ones_the_selection_needs():
    seg = 4096
    s = toc.BY_NAME
    assert s["tail_of_4"].V % seg == 4 and s["tail_of_4"].k_predict == 1024 and -(-s["tail_of_4"].V // seg) * 1024 <= seg
    v, k = s["three_stages"].V, s["three_stages"].k_predict
    first = -(-v // seg) * k
    assert first > seg and -(-first // seg) * k <= seg and -(-first // seg) > 1          # three stages exactly
    assert v % seg < k                                                                   # a short last segment in stage one
    assert s["tail_of_1"].V % seg == 1 and s["tail_of_1"].n > 128
    assert s["whole_vocabulary"].k_predict == s["whole_vocabulary"].V == s["whole_vocabulary"].k_analogy + 3
    assert s["tail_of_4"].n > 64                                                         # batch=64 splits the call
    for spec in toc.SPECS:
        assert spec.n * spec.V <= 2_100_000
        finite = spec.V - len(spec.dead)
        assert spec.k_predict <= finite and spec.k_analogy <= max(spec.V - 3, 0)
    assert s["dead_rows_all_finite_taken"].k_predict == s["dead_rows_all_finite_taken"].V - 2


@pytest.mark.parametrize("name,path", CASE_PATHS)
def test_groups_are_a_gap_apart_and_the_ranking_is_the_references(name, path):
    case = toc.build(name)
    spec = case["spec"]
    k = spec.k(path)
    W, group_of = case["W"], case["group_of"]
    live = np.setdiff1d(np.arange(spec.V), case["dead"])
    assert (W[live] == case["P"][group_of[live]]).all()      # every row is its prototype, bit for bit
    if spec.groups > 1 and spec.V > 4:
        assert np.bincount(group_of).min() >= 2              # every group holds a tie
    # the gap between groups, from the reference's scores on the full table: two scores of a query are either one group's
    # (equal to rounding of the float64 matmul) or GROUP_GAP apart
    full_s, full_i = reference_topk(case, path, spec.V)
    fin = np.isfinite(full_s)
    n_fin = fin.sum(1)
    assert (n_fin == (spec.V - len(case["dead"]) - (0 if path == "predict" else 3))).all()
    for q in range(len(full_s)):
        sq, gq = full_s[q, :n_fin[q]], group_of[full_i[q, :n_fin[q]]]
        step = sq[:-1] - sq[1:]
        same = gq[:-1] == gq[1:]
        assert (step[same] <= 1e-12).all()
        need = toc.GROUP_GAP * (np.maximum(1.0, np.abs(sq[:-1])) if path == "cosmul" else 1.0)
        assert (step[~same] >= (need[~same] if path == "cosmul" else need)).all(), (name, path, q, step[~same].min())
        assert len(set(gq[np.r_[True, ~same]].tolist())) == (~same).sum() + 1            # a group is one run of the ranking
    # the expected ranking: every position, none left out
    want_s, want_i = toc.expected(name, path)
    assert want_i.shape == want_s.shape == (spec.n, k)
    got_s, got_i = reference_topk(case, path, k)
    # the reference's stable sort gives (score descending, id ascending) wherever it scores the copies of a row alike; a
    # float64 matmul whose blocking depends on the position may round two copies differently (not seen with this NumPy),
    # and then only the order inside a group is its rounding's: the groups and the id sets are compared in any case
    np.testing.assert_allclose(got_s, want_s, rtol=1e-12, atol=1e-14)
    assert (group_of[got_i] == group_of[want_i]).all()
    if ref_is_exact_inside_groups(full_s, full_i, group_of, n_fin):
        assert (got_i == want_i).all()
    # lexsort (score descending, id ascending), spelled out
    for q in range(spec.n):
        s, i = want_s[q], want_i[q]
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:]))).all()
        assert len(set(i.tolist())) == k
    if path != "predict":
        assert not (want_i[:, :, None] == case["abc"][:, None, :]).any()
    assert not np.isin(want_i, case["dead"]).any()
    if path == "predict" and spec.groups > 1 and not len(case["dead"]):
        assert (group_of[want_i[:, 0]] == group_of[case["queries"]]).all()


def ref_is_exact_inside_groups(full_s, full_i, group_of, n_fin):
    """Whether the reference scored all copies of a row alike (then its stable sort is the expected order itself)."""
    for q in range(len(full_s)):
        sq, gq = full_s[q, :n_fin[q]], group_of[full_i[q, :n_fin[q]]]
        if (sq[:-1][gq[:-1] == gq[1:]] != sq[1:][gq[:-1] == gq[1:]]).any():
            return False
    return True


def test_identical_rows_rank_by_id_alone():
    case = toc.build("all_identical")
    _, idx = toc.expected("all_identical", "predict")
    assert (idx == np.arange(100)).all()
    for path in ("cosadd", "cosmul"):
        _, idx = toc.expected("all_identical", path)
        for q, abc in enumerate(case["abc"].tolist()):
            assert idx[q].tolist() == [v for v in range(110) if v not in abc][:100]
