"""libglove_prep_hip.so on the GPU (include/glove_cooc_stream_hip.h): the merge kernel, a chunk's keys and the final
table against the NumPy restatement of tests/cooc_stream_ref.py, exactly; the streamed table against the one-shot call,
bit for bit; trainer.text8 with chunks; the three calls captured into one graph."""

import numpy as np
import pytest
import torch

import cooc_stream_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
KEY_PATTERN, COUNT_PATTERN = -0x0123456789ABCDEF, 0x0FEDCBA987654321


@pytest.fixture(scope="module")
def prep(hip):
    from trainer import hip_api
    return hip_api.load_prep_library()


def dev(a, dtype=torch.int64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the merge
def merge_raw(prep, A, cA, B, cB, cap_out, n_a=None, n_b=None):
    """glove_cooc_merge_u64 itself on device copies of the arrays (capacities = their lengths; *n_a, *n_b default to
    them): (rc, *n_out, keys_out, counts_out), the outputs cap_out + GUARD long and pre-filled with a pattern."""
    ka, ca, kb, cb = dev(A), dev(cA), dev(B), dev(cB)
    sizes = dev(np.asarray([len(A) if n_a is None else n_a, len(B) if n_b is None else n_b, -7], np.int64))
    ko = torch.full((cap_out + GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
    co = torch.full((cap_out + GUARD,), COUNT_PATTERN, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_cooc_merge_workspace_bytes(len(A), len(B)), dtype=torch.uint8, device=DEV)
    rc = prep.glove_cooc_merge_u64(ka.data_ptr(), ca.data_ptr(), sizes[0:1].data_ptr(), len(A), kb.data_ptr(), cb.data_ptr(),
                                   sizes[1:2].data_ptr(), len(B), ko.data_ptr(), co.data_ptr(), sizes[2:3].data_ptr(), cap_out,
                                   ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, int(sizes[2].item()), ko.cpu().numpy(), co.cpu().numpy()


def check_merge(prep, A, cA, B, cB, n_a=None, n_b=None):
    """Against the reference at four capacities: room for both inputs, the true size, one less, none."""
    na, nb = (len(A) if n_a is None else n_a), (len(B) if n_b is None else n_b)
    want_k, want_c = sref.merge(A[:na], cA[:na], B[:nb], cB[:nb])
    true = len(want_k)
    for cap in sorted({na + nb, true, max(true - 1, 0), 0}):
        rc, n_out, ko, co = merge_raw(prep, A, cA, B, cB, cap, n_a, n_b)
        assert rc == 0 and n_out == true, (rc, n_out, true, cap)           # the true size, whatever the capacity
        m = min(true, cap)
        np.testing.assert_array_equal(ko[:m], want_k[:m])
        np.testing.assert_array_equal(co[:m], want_c[:m])
        assert (ko[m:] == KEY_PATTERN).all() and (co[m:] == COUNT_PATTERN).all(), cap    # nothing beyond *n_out or cap_out


def ascending(rng, n, hi, base=0):
    return np.sort(rng.choice(hi, n, replace=False)).astype(np.int64) + base


def merge_cases():
    from trainer.hip_api import COOC_MERGE_TILE as T
    rng = np.random.default_rng(11)
    counts = lambda n: rng.integers(1, 1000, n).astype(np.int64)
    cases = {}
    for label, L in (("0", 0), ("1", 1), ("T-1", T - 1), ("T", T), ("T+1", T + 1), ("3T+5", 3 * T + 5), ("40T+17", 40 * T + 17)):
        na = L // 3                                                        # the merged length around the tile size
        nb = L - na
        hi = max(2 * L, 4)                                                 # dense enough for twins
        cases["merged_length_" + label] = (ascending(rng, na, hi), counts(na), ascending(rng, nb, hi), counts(nb))
    one = np.asarray([5], np.int64)
    none = np.zeros(0, np.int64)
    cases["one_entry_in_a"] = (one, one, none, none)
    n = 3 * T + 5
    some = ascending(rng, n, 10 * n)
    cases["a_empty"] = (none, none, some, counts(n))
    cases["b_empty"] = (some, counts(n), none, none)
    cases["both_empty"] = (none, none, none, none)
    cases["a_equals_b"] = (some, counts(n), some.copy(), counts(n))       # every split lands on a twin pair
    cases["a_below_b"] = (some, counts(n), some + some[-1] + 1, counts(n))
    cases["b_below_a"] = (some + some[-1] + 1, counts(n), some, counts(n))
    cases["interleaved_no_twins"] = (2 * np.arange(n, dtype=np.int64), counts(n), 2 * np.arange(n, dtype=np.int64) + 1, counts(n))
    big = ascending(rng, n, 10 * n, base=(1 << 62) + 12345)
    cases["keys_above_2_62_counts_near_2_40"] = (big, (1 << 40) - counts(n), big[::2].copy() if n else big,
                                                 (1 << 40) + counts(len(big[::2])))
    cases["uneven_sizes"] = (ascending(rng, 7, 40 * T), counts(7), ascending(rng, 9 * T + 3, 40 * T), counts(9 * T + 3))
    return cases


MERGE_CASES = None


def merge_case(name):
    global MERGE_CASES
    if MERGE_CASES is None:
        MERGE_CASES = merge_cases()
    return MERGE_CASES[name]


@pytest.mark.parametrize("name", ["merged_length_%s" % s for s in ("0", "1", "T-1", "T", "T+1", "3T+5", "40T+17")]
                         + ["one_entry_in_a", "a_empty", "b_empty", "both_empty", "a_equals_b", "a_below_b", "b_below_a",
                            "interleaved_no_twins", "keys_above_2_62_counts_near_2_40", "uneven_sizes"])
def test_merge_equals_the_reference_exactly(prep, name):
    A, cA, B, cB = merge_case(name)
    if name == "keys_above_2_62_counts_near_2_40":
        assert A.min() > 1 << 62 and (sref.merge(A, cA, B, cB)[1] > 1 << 40).any()
    check_merge(prep, A, cA, B, cB)


def test_merge_honours_the_device_side_counts(prep):
    from trainer.hip_api import COOC_MERGE_TILE as T
    rng = np.random.default_rng(5)
    A, B = ascending(rng, 2 * T + 9, 8 * T), ascending(rng, T + 3, 8 * T)
    cA, cB = rng.integers(1, 9, len(A)).astype(np.int64), rng.integers(1, 9, len(B)).astype(np.int64)
    n_a, n_b = T + 1, T - 2
    A[n_a:], B[n_b:] = 3, 1                                                 # poison behind the counts: small, unsorted, equal
    cA[n_a:], cB[n_b:] = 1 << 50, 1 << 51
    check_merge(prep, A, cA, B, cB, n_a, n_b)
    check_merge(prep, A, cA, B, cB, 0, n_b)
    A, cA = ascending(rng, 2 * T + 9, 8 * T), np.ones(2 * T + 9, np.int64)
    want = sref.merge(A, cA, B[:0], cB[:0])
    rc, n_out, ko, co = merge_raw(prep, A, cA, B, cB, len(A), len(A) + 100, -4)      # clamped to the capacity / to zero
    assert rc == 0 and n_out == len(A) and (ko[:n_out] == want[0]).all()


def test_merge_refuses_outputs_that_alias_inputs(prep):
    k = torch.zeros(100, dtype=torch.int64, device=DEV)
    c = torch.zeros(100, dtype=torch.int64, device=DEV)
    o = torch.zeros(200, dtype=torch.int64, device=DEV)
    n = torch.zeros(3, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_cooc_merge_workspace_bytes(100, 50), dtype=torch.uint8, device=DEV)
    call = lambda ko, co: prep.glove_cooc_merge_u64(k.data_ptr(), c.data_ptr(), n[0:1].data_ptr(), 100, k.data_ptr(), c.data_ptr(),
                                                    n[1:2].data_ptr(), 50, ko, co, n[2:3].data_ptr(), 100, ws.data_ptr(),
                                                    ws.numel(), stream())
    assert call(k.data_ptr(), o.data_ptr()) == -1 and call(o.data_ptr(), c.data_ptr()) == -1
    assert call(o.data_ptr(), o.data_ptr()) == -1
    assert call(o.data_ptr(), o[100:].data_ptr()) == 0
    torch.cuda.synchronize()


# ---- a chunk's keys
def chunk_keys_raw(prep, tok, n_own, V, context, cap):
    tokens = dev(tok, torch.int32)
    ko = torch.full((cap + GUARD,), KEY_PATTERN, dtype=torch.int64, device=DEV)
    co = torch.full((cap + GUARD,), COUNT_PATTERN, dtype=torch.int64, device=DEV)
    n_out = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_cooc_chunk_workspace_bytes(len(tok), context), dtype=torch.uint8, device=DEV)
    rc = prep.glove_cooc_chunk_keys_i32(tokens.data_ptr() if len(tok) else None, n_own, len(tok), V, context, ko.data_ptr(),
                                        co.data_ptr(), n_out.data_ptr(), cap, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, n_out.cpu().numpy(), ko.cpu().numpy(), co.cpu().numpy()


@pytest.mark.parametrize("n_own, n_total, V, context", [(0, 0, 5, 3), (1, 1, 5, 3), (1, 4, 5, 3), (50, 52, 4, 2), (5000, 5005, 60, 5),
                                                        (3000, 3000, 7, 9), (600, 855, 40, 255)])
def test_chunk_keys_equal_the_reference(prep, n_own, n_total, V, context):
    tok = np.random.default_rng(n_total).integers(0, V, n_total).astype(np.int32)
    want_k, want_c = sref.chunk_keys(tok, n_own, V, context)
    true = len(want_k)
    assert true > 0 or n_own <= 1
    for cap in sorted({max(1, 2 * context * n_own), true, max(true - 1, 0), 0}):
        rc, n_out, ko, co = chunk_keys_raw(prep, tok, n_own, V, context, cap)
        assert rc == 0 and n_out[0] == true and n_out[1] == -7, (rc, n_out, true, cap)
        m = min(true, cap)
        np.testing.assert_array_equal(ko[:m], want_k[:m])
        np.testing.assert_array_equal(co[:m], want_c[:m])
        assert (ko[m:] == KEY_PATTERN).all() and (co[m:] == COUNT_PATTERN).all(), cap


def test_binding_raises_where_a_capacity_is_exceeded(hip):
    from trainer.hip_api import GloveHipError
    tok = dev(np.random.default_rng(0).integers(0, 30, 500), torch.int32)
    keys, counts = hip.cooc_chunk_keys(tok, 500, 30, 4)
    with pytest.raises(GloveHipError, match="capacity"):
        hip.cooc_chunk_keys(tok, 500, 30, 4, cap=len(keys) - 1)
    assert len(hip.cooc_chunk_keys(tok, 500, 30, 4, cap=len(keys))[0]) == len(keys)
    small = torch.empty(len(keys) - 1, dtype=torch.int64, device=DEV)
    with pytest.raises(GloveHipError, match="capacity"):
        hip.cooc_merge(keys, counts, keys[:0], counts[:0], small, torch.empty_like(small))
    with pytest.raises(GloveHipError, match="capacity"):
        hip.cooc_finalize(keys, counts, 30, 4, cap=3)
    row, col, cnt, val = hip.cooc_finalize(keys, counts, 30, 4)
    want = sref.finalize(keys.cpu().numpy(), counts.cpu().numpy(), 30, 4)
    for g, w in zip((row, col, cnt, val), want):
        assert g.cpu().numpy().dtype == w.dtype
        np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---- streamed equals one-shot, bit for bit
def zipf_tokens(n, V, seed):
    p = 1.0 / np.arange(1, V + 1)
    return np.random.default_rng(seed).choice(V, size=n, p=p / p.sum()).astype(np.int32)


def stream_table(hip, tok, V, context, chunk, min_count=0):
    from trainer.cooccur import CoocAccumulator, iter_chunks
    acc = CoocAccumulator(V, context, hip)
    for piece, n_own in iter_chunks([tok], chunk, context):
        acc.add(piece, n_own)
    return acc, [t.cpu().numpy() for t in acc.finalize(min_count)]


ONE_SHOT = {}


def one_shot(hip, n, V, context):
    """(tokens, the one-shot call's table): computed once per shape and left unchanged."""
    if (n, V, context) not in ONE_SHOT:
        tok = zipf_tokens(n, V, seed=n)
        ONE_SHOT[n, V, context] = (tok, [t.cpu().numpy() for t in hip.cooccurrence(dev(tok, torch.int32), V, context)])
    return ONE_SHOT[n, V, context]


@pytest.mark.parametrize("n, V, context, chunk", [(2000, 1000, 5, 1)]
                         + [(n, V, 5, c) for n, V in ((20000, 1000), (200000, 50000)) for c in (4096, "n-1", "n")])
def test_streamed_equals_one_shot_bit_for_bit(hip, n, V, context, chunk):
    tok, want = one_shot(hip, n, V, context)
    chunk = {"n-1": n - 1, "n": n}.get(chunk, chunk)
    acc, got = stream_table(hip, tok, V, context, chunk)
    assert acc.chunks == -(-n // chunk) and len(want[0]) > n // 4
    for g, w, name in zip(got, want, ("row", "col", "count", "value")):
        assert g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)                 # `value` too: the same doubles, not close ones


def test_min_count_filter_is_the_host_filter(hip):
    tok, want = one_shot(hip, 20000, 1000, 5)
    keep = want[2] >= 10
    assert 0 < keep.sum() < len(keep)
    _, got = stream_table(hip, tok, 1000, 5, 4096, min_count=10)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w[keep])


def test_text8_with_chunks_writes_identical_files(hip, tmp_path):
    from pathlib import Path
    from trainer import text8
    text = (Path(__file__).resolve().parent / "golden" / "text8_corpus.txt").read_text()
    whole = text8.process_data(text, None, 0.9, 5, hip=hip, seed=3)
    chunked = text8.process_data(text, None, 0.9, 5, hip=hip, seed=3, chunk_tokens=1000)
    assert set(whole["interaction"]) == set(chunked["interaction"]) and len(whole["interaction"]["count"]) > 100
    for k, v in whole["interaction"].items():
        np.testing.assert_array_equal(chunked["interaction"][k], v, err_msg=k)
    text8.save_data(whole, tmp_path / "whole")
    text8.save_data(chunked, tmp_path / "chunked")
    for f in ("vocab.csv", "vocab.txt", "interaction.csv"):
        assert (tmp_path / "whole" / f).read_bytes() == (tmp_path / "chunked" / f).read_bytes(), f


# ---- the calls promise to be capturable
def test_chunk_merge_finalize_captured_into_one_graph(hip, prep):
    V, context, n_own = 200, 5, 3000
    first, second, third = (zipf_tokens(n_own + context, V, seed) for seed in (1, 2, 3))
    keys_a, counts_a = hip.cooc_chunk_keys(dev(first, torch.int32), n_own, V, context)
    keys_a, counts_a = keys_a.clone(), counts_a.clone()
    n_a = dev(np.asarray([len(keys_a)], np.int64))
    cap_b = 2 * context * n_own
    cap = len(keys_a) + cap_b
    tokens = dev(second, torch.int32)
    new = lambda n, dtype=torch.int64: torch.zeros(n, dtype=dtype, device=DEV)
    keys_b, counts_b, n_b = new(cap_b), new(cap_b), new(2)
    keys_o, counts_o, n_o = new(cap), new(cap), new(2)
    row, col, cnt, val, nnz = new(cap, torch.int32), new(cap, torch.int32), new(cap), new(cap, torch.float64), new(2)
    bytes_ = lambda n: torch.empty(n, dtype=torch.uint8, device=DEV)
    ws = (bytes_(prep.glove_cooc_chunk_workspace_bytes(n_own + context, context)),
          bytes_(prep.glove_cooc_merge_workspace_bytes(len(keys_a), cap_b)), bytes_(prep.glove_cooc_finalize_workspace_bytes(cap)))

    def enqueue():
        hip.cooc_chunk_keys_enqueue(tokens, n_own, V, context, keys_b, counts_b, n_b, ws[0])
        hip.cooc_merge_enqueue(keys_a, counts_a, n_a, keys_b, counts_b, n_b, keys_o, counts_o, n_o, ws[1])
        hip.cooc_finalize_enqueue(keys_o, counts_o, n_o, V, context, 2, row, col, cnt, val, nnz, ws[2])

    def result():
        torch.cuda.synchronize()
        m = int(nnz[0].item())
        return [t[:m].cpu().numpy().copy() for t in (row, col, cnt, val)]

    def expected(tok):
        kb, cb = sref.chunk_keys(tok, n_own, V, context)
        return sref.finalize(*sref.merge(keys_a.cpu().numpy(), counts_a.cpu().numpy(), kb, cb), V, context, 2)

    enqueue()                                       # eager, and the warm-up of every kernel
    eager = result()
    for g, w in zip(eager, expected(second)):
        np.testing.assert_array_equal(g, w)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for tok in (third, second):                     # two replays, on fresh input each
        tokens.copy_(dev(tok, torch.int32))
        nnz.fill_(-1)
        graph.replay()
        for g, w in zip(result(), expected(tok)):
            np.testing.assert_array_equal(g, w)
    for g, w in zip(result(), eager):
        np.testing.assert_array_equal(g, w)
