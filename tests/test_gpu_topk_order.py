"""The order of the staged top-k selection (topk_select_kernel of csrc/glove_topk_kernels.h), pinned exactly, through its
three callers: glove_topk_cosine_f32, glove_analogy_topk_f32 and glove_cosmul_topk_f32.

The vocabularies of tests/topk_order_cases.py are copies of a few prototype rows: the scores inside a group are the same
float, the groups are 1e-4 apart in float64, so the ids a call returns must equal lexsort(score descending, id ascending)
at EVERY position — across the 16 registers of a thread, the lanes of a wave, the four waves, the segments of 4,096
candidates and the stages.  tests/test_topk_order_cases.py proves the cases on the float64 references alone.

Scores: rtol 1e-5, atol 1e-6, the project's figures for the similarity GEMM."""
import numpy as np
import pytest
import torch

import topk_order_cases as toc
from helpers import to_dev

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6
CASE_PATHS = [(s.name, p) for s in toc.SPECS for p in toc.runs(s.name)]


def run(hip, case, path, **kw):
    k = case["spec"].k(path)
    if path == "predict":
        return hip.topk_cosine(*to_dev(case["W"], case["queries"]), k)
    if path == "cosadd":
        return hip.analogy_topk(*to_dev(case["W"], case["abc"]), k, **kw)
    return hip.analogy_cosmul_topk(*to_dev(case["W"], case["abc"]), k, toc.COSMUL_EPS, **kw)


@pytest.mark.parametrize("name,path", CASE_PATHS)
def test_every_position_of_the_ranking(hip, name, path):
    case = toc.build(name)
    spec = case["spec"]
    want_s, want_i = toc.expected(name, path)
    sims, idx = run(hip, case, path)
    assert sims.shape == idx.shape == want_i.shape and sims.dtype == torch.float32 and idx.dtype == torch.int32
    got_s, got_i = sims.cpu().numpy(), idx.cpu().numpy()
    wrong = np.argwhere(got_i != want_i)
    print("%s %s: %d of %d positions differ, largest score deviation %.3g"
          % (name, path, len(wrong), want_i.size, np.abs(got_s - want_s).max()))
    assert len(wrong) == 0, (name, path, wrong[:5], got_i[tuple(wrong[0])], want_i[tuple(wrong[0])])
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=ATOL)
    # identical rows, identical floats: inside a group the scores of a query are one bit pattern
    g = case["group_of"][got_i]
    same = g[:, :-1] == g[:, 1:]
    assert (got_s[:, :-1][same] == got_s[:, 1:][same]).all()
    assert not np.isin(got_i, case["dead"]).any()            # a NaN or an infinite row is never returned
    if name == "all_identical" and path == "predict":
        assert (got_i == np.arange(spec.k_predict)).all()


@pytest.mark.parametrize("path", ["cosadd", "cosmul"])
def test_batched_calls_equal_the_single_call_bit_for_bit(hip, path):
    case = toc.build("tail_of_4")
    one = run(hip, case, path)
    batched = run(hip, case, path, batch=64)                 # 64 + 64 + 2 questions through one workspace
    assert torch.equal(one[0], batched[0]) and torch.equal(one[1], batched[1])
    assert (one[1].cpu().numpy() == toc.expected("tail_of_4", path)[1]).all()
