"""The fourth header of libglove_prep_hip.so on the GPU (include/glove_cooc_options_hip.h): the token filter against the
NumPy restatement of tests/cooc_options_ref.py, bit for bit, at every tile edge and position width; the weighted
finalisation against glove_cooc_finalize (harmonic) and the restatement (uniform, dynamic), doubles compared as bits;
`python -m trainer.cooccur` with the options set, device tokenizer, against the NumPy backend with the python tokenizer."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cooc_options_ref as oref
import cooc_stream_ref as sref
import text_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = Path(__file__).resolve().parent.parent
CORPUS = Path(__file__).resolve().parent / "golden" / "text8_corpus.txt"
FILES = ("vocab.csv", "vocab.txt", "interaction.csv")
GUARD = 64
ID_PATTERN, COUNT_PATTERN, VALUE_PATTERN = -0x01234567, 0x0FEDCBA987654321, -7.25
V = 1000
POSITIONS = (0, 2 ** 32 - 3, 2 ** 40)                 # 2^32 - 3: positions cross 32 bits inside the first tile


@pytest.fixture(scope="module")
def prep(hip):
    from trainer import hip_api
    return hip_api.load_prep_library()


def tile():
    from trainer.hip_api import FILTER_TILE
    return FILTER_TILE


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def threshold_table(kind):
    if kind == "all_keep":
        return np.full(V, 0xFFFFFFFF, np.uint32)
    if kind == "all_drop":
        return np.zeros(V, np.uint32)
    if kind == "alternating":
        return np.where(np.arange(V) % 2 == 0, 0xFFFFFFFF, 0).astype(np.uint32)
    assert kind == "zipf"
    counts = np.maximum(1, (1e6 / np.arange(1, V + 1))).astype(np.int64)
    table = oref.thresholds(counts, 1e-3)
    assert 10 < (table < 0xFFFFFFFF).sum() < V and table.min() > 0
    return table


def zipf_ids(n, seed):
    p = 1.0 / np.arange(1, V + 1)
    return np.random.default_rng(seed).choice(V, size=n, p=p / p.sum()).astype(np.int32)


IDS = {}


def ids_of(n):
    """One id stream per length: made once and left unchanged."""
    if n not in IDS:
        IDS[n] = zipf_ids(n, seed=n)
    return IDS[n]


def filter_raw(prep, ids, pos0, table, seed, cap, in_shift=0, out_shift=0):
    """glove_token_filter_i32 itself: (rc, *n_out, ids_out [cap + GUARD], pre-filled with a pattern).  in_shift / out_shift:
    elements by which ids / ids_out start behind a 256-B aligned address."""
    n = len(ids)
    src = torch.zeros(n + in_shift + 4, dtype=torch.int32, device=DEV)
    src[in_shift:in_shift + n] = dev(ids, torch.int32)
    thr = dev(np.asarray(table, np.uint32).view(np.int32), torch.int32)
    out = torch.full((out_shift + cap + GUARD,), ID_PATTERN, dtype=torch.int32, device=DEV)
    n_out = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_token_filter_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    rc = prep.glove_token_filter_i32(src[in_shift:].data_ptr(), n, pos0, thr.data_ptr(), len(table), seed, out[out_shift:].data_ptr(),
                                     n_out.data_ptr(), cap, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:out_shift] == ID_PATTERN).all()                          # nothing in front of ids_out
    return rc, n_out.cpu().numpy(), got[out_shift:]


def check_filter(prep, ids, pos0, table, seed, **shifts):
    want = oref.token_filter(ids, pos0, table, seed)
    rc, n_out, got = filter_raw(prep, ids, pos0, table, seed, len(ids), **shifts)
    assert rc == 0 and n_out[0] == len(want) and n_out[1] == -7, (rc, n_out, len(want))
    np.testing.assert_array_equal(got[:len(want)], want)
    assert (got[len(want):] == ID_PATTERN).all()                          # nothing beyond the survivors
    return want


@pytest.mark.parametrize("kind", ["all_keep", "all_drop", "alternating", "zipf"])
@pytest.mark.parametrize("n", ["1", "63", "64", "65", "T-1", "T", "T+1", "3T+5", "300T+17"])
def test_filter_equals_the_reference_bit_for_bit(prep, n, kind):
    T = tile()
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5, "300T+17": 300 * T + 17}.get(n) or int(n)
    ids, table = ids_of(n), threshold_table(kind)
    for pos0 in POSITIONS:
        want = check_filter(prep, ids, pos0, table, seed=5)
        if kind == "all_keep":
            assert len(want) == n
        elif kind == "all_drop":
            assert len(want) == 0
        elif kind == "zipf" and n >= T - 1:
            assert 0 < len(want) < n


def test_filter_at_every_alignment_of_input_and_output(prep):
    T = tile()
    ids, table = ids_of(3 * T + 5), threshold_table("zipf")
    for in_shift in range(4):                                             # 16-B loads only where ids allow them
        for out_shift in range(4):                                        # 16-B stores from the first aligned element on
            check_filter(prep, ids, 2 ** 32 - 3, table, seed=9, in_shift=in_shift, out_shift=out_shift)
    for n in (1, 2, 3, 5, 9):                                             # fewer survivors than an aligned head plus a quad
        for out_shift in range(4):
            check_filter(prep, ids_of(3 * T + 5)[:n], 7, threshold_table("all_keep"), seed=0, in_shift=1, out_shift=out_shift)


def test_an_empty_block_writes_a_zero_count_and_nothing_else(prep):
    out = torch.full((GUARD,), ID_PATTERN, dtype=torch.int32, device=DEV)
    n_out = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    thr = dev(threshold_table("zipf").view(np.int32), torch.int32)
    ws = torch.empty(prep.glove_token_filter_workspace_bytes(0), dtype=torch.uint8, device=DEV)
    rc = prep.glove_token_filter_i32(None, 0, 12, thr.data_ptr(), V, 0, out.data_ptr(), n_out.data_ptr(), GUARD, ws.data_ptr(),
                                     ws.numel(), stream())
    torch.cuda.synchronize()
    assert rc == 0 and n_out.tolist() == [0, -7] and (out.cpu().numpy() == ID_PATTERN).all()


def test_a_block_s_survivors_do_not_depend_on_where_the_stream_was_cut(hip):
    T = tile()
    n = 40 * T + 17
    ids, table = ids_of(n), threshold_table("zipf")
    for pos0 in (0, 2 ** 32 - 5 * T - 3):
        whole = oref.token_filter(ids, pos0, table, 3)
        got = hip.token_filter(dev(ids, torch.int32), pos0, table, 3)
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.cpu().numpy(), whole)
        rng = np.random.default_rng(pos0 % 1000)
        cuts = np.sort(np.concatenate([rng.integers(0, n, 12), [1, T, T + 1, 5 * T + 3, n - 1]]))
        parts, pos = [], pos0
        thr = dev(table.view(np.int32), torch.int32)
        for block in np.split(ids, cuts):
            parts.append(hip.token_filter(dev(block, torch.int32), pos, thr, 3).cpu().numpy())
            pos += len(block)
        np.testing.assert_array_equal(np.concatenate(parts), whole)


def test_two_runs_give_equal_bits(prep):
    T = tile()
    ids, table = ids_of(300 * T + 17), threshold_table("zipf")
    a = filter_raw(prep, ids, 2 ** 40, table, 1, len(ids))
    b = filter_raw(prep, ids, 2 ** 40, table, 1, len(ids))
    assert a[0] == b[0] == 0 and a[1].tolist() == b[1].tolist()
    np.testing.assert_array_equal(a[2], b[2])
    c = filter_raw(prep, ids, 2 ** 40, table, 2, len(ids))                # another seed, other survivors
    assert not np.array_equal(a[2], c[2])


def test_the_true_count_comes_back_where_the_capacity_is_short(prep):
    T = tile()
    ids, table = ids_of(3 * T + 5), threshold_table("zipf")
    want = oref.token_filter(ids, 0, table, 4)
    assert len(want) > T
    for cap in (len(want), len(want) - 1, T + 3, T, 1, 0):                # also: a tile that starts beyond the capacity
        for out_shift in (0, 3):
            rc, n_out, got = filter_raw(prep, ids, 0, table, 4, cap, out_shift=out_shift)
            assert rc == 0 and n_out[0] == len(want), (cap, n_out)
            np.testing.assert_array_equal(got[:cap], want[:cap])
            assert (got[cap:] == ID_PATTERN).all(), cap                   # the guard behind the capacity is intact


def test_filter_captured_into_a_graph_and_replayed(hip, prep):
    T = tile()
    n = 5 * T + 77
    table = threshold_table("zipf")
    thr = dev(table.view(np.int32), torch.int32)
    ids = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    n_out = torch.zeros(2, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_token_filter_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    pos0, seed = 2 ** 32 - 3, 6

    def result():
        torch.cuda.synchronize()
        return out[:int(n_out[0].item())].cpu().numpy().copy()

    first, second = zipf_ids(n, 21), zipf_ids(n, 22)
    ids.copy_(dev(first, torch.int32))
    hip.token_filter_enqueue(ids, pos0, thr, seed, out, n_out, ws)        # eager, and the warm-up of every kernel
    eager = result()
    np.testing.assert_array_equal(eager, oref.token_filter(first, pos0, table, seed))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.token_filter_enqueue(ids, pos0, thr, seed, out, n_out, ws)
    for tok in (second, first):                                           # two replays, on fresh input each
        ids.copy_(dev(tok, torch.int32))
        n_out.fill_(-1)
        out.fill_(ID_PATTERN)
        graph.replay()
        np.testing.assert_array_equal(result(), oref.token_filter(tok, pos0, table, seed))
    np.testing.assert_array_equal(result(), eager)


# ---- the weighted finalisation
STATES = {}


def state(hip, n, V_, context):
    """(keys, counts) of the tokens tests/test_gpu_cooc_stream.py counts for (n, V, context): made once per shape."""
    from test_gpu_cooc_stream import zipf_tokens
    if (n, V_, context) not in STATES:
        keys, counts = hip.cooc_chunk_keys(dev(zipf_tokens(n, V_, seed=n), torch.int32), n, V_, context)
        STATES[n, V_, context] = (keys.clone(), counts.clone())
    return STATES[n, V_, context]


def finalize_raw(prep, keys, counts, V_, context, min_count, weighting, cap):
    """glove_cooc_finalize (weighting None) or glove_cooc_finalize_weighted itself: (rc, *out_nnz, row, col, count, value),
    the outputs cap + GUARD long and pre-filled with patterns."""
    m = int(keys.numel())
    sizes = torch.tensor([m, -7, -7], dtype=torch.int64).to(DEV)
    row = torch.full((cap + GUARD,), ID_PATTERN, dtype=torch.int32, device=DEV)
    col = torch.full((cap + GUARD,), ID_PATTERN, dtype=torch.int32, device=DEV)
    cnt = torch.full((cap + GUARD,), COUNT_PATTERN, dtype=torch.int64, device=DEV)
    val = torch.full((cap + GUARD,), VALUE_PATTERN, dtype=torch.float64, device=DEV)
    if weighting is None:
        ws = torch.empty(prep.glove_cooc_finalize_workspace_bytes(m), dtype=torch.uint8, device=DEV)
        rc = prep.glove_cooc_finalize(keys.data_ptr(), counts.data_ptr(), sizes[0:1].data_ptr(), m, V_, context, min_count,
                                      row.data_ptr(), col.data_ptr(), cnt.data_ptr(), val.data_ptr(), sizes[1:2].data_ptr(), cap,
                                      ws.data_ptr(), ws.numel(), stream())
    else:
        ws = torch.empty(prep.glove_cooc_finalize_weighted_workspace_bytes(m), dtype=torch.uint8, device=DEV)
        rc = prep.glove_cooc_finalize_weighted(keys.data_ptr(), counts.data_ptr(), sizes[0:1].data_ptr(), m, V_, context, min_count,
                                               weighting, row.data_ptr(), col.data_ptr(), cnt.data_ptr(), val.data_ptr(),
                                               sizes[1:2].data_ptr(), cap, ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, int(sizes[1].item()), [t.cpu().numpy() for t in (row, col, cnt, val)]


@pytest.mark.parametrize("n, V_, context", [(2000, 1000, 5), (20000, 1000, 5), (200000, 50000, 5)])
@pytest.mark.parametrize("min_count", [0, 3])
def test_harmonic_is_glove_cooc_finalize_bit_for_bit(hip, prep, n, V_, context, min_count):
    keys, counts = state(hip, n, V_, context)
    cap = int(keys.numel())
    rc_a, nnz_a, a = finalize_raw(prep, keys, counts, V_, context, min_count, None, cap)
    rc_b, nnz_b, b = finalize_raw(prep, keys, counts, V_, context, min_count, 0, cap)
    assert rc_a == rc_b == 0 and nnz_a == nnz_b > 0
    for x, y, name in zip(a, b, ("row", "col", "count", "value")):
        assert x.dtype == y.dtype
        assert x.tobytes() == y.tobytes(), name                             # the guard patterns included


@pytest.mark.parametrize("weighting", ["uniform", "dynamic"])
@pytest.mark.parametrize("n, V_, context", [(3000, 50, 1), (3000, 50, 2), (20000, 1000, 5), (600, 40, 255)])
def test_uniform_and_dynamic_equal_the_reference_exactly(hip, prep, n, V_, context, weighting):
    from trainer.hip_api import WINDOW_WEIGHTINGS
    keys, counts = state(hip, n, V_, context)
    hk, hc = keys.cpu().numpy(), counts.cpu().numpy()
    for min_count in (0, 4):
        want = oref.finalize_weighted(hk, hc, V_, context, min_count, weighting)
        true = len(want[0])
        assert true > 0
        for cap in sorted({len(hk), true, max(true - 1, 0), 0}):
            rc, nnz, got = finalize_raw(prep, keys, counts, V_, context, min_count, WINDOW_WEIGHTINGS[weighting], cap)
            assert rc == 0 and nnz == true, (rc, nnz, true, cap)
            m = min(true, cap)
            for g, w, pattern in zip(got, want, (ID_PATTERN, ID_PATTERN, COUNT_PATTERN, VALUE_PATTERN)):
                assert g.dtype == w.dtype
                assert g[:m].tobytes() == w[:m].tobytes()                   # the doubles as bits
                assert (g[m:] == pattern).all(), cap
    # the binding routes by name and returns the same arrays
    got = hip.cooc_finalize(keys, counts, V_, context, 4, weighting=weighting)
    for g, w in zip(got, oref.finalize_weighted(hk, hc, V_, context, 4, weighting)):
        assert g.cpu().numpy().tobytes() == w.tobytes()


def test_min_count_is_applied_on_count_not_on_value(hip):
    from trainer.hip_api import GloveHipError
    keys, counts = state(hip, 20000, 1000, 5)
    row, col, cnt, val = (t.cpu().numpy() for t in hip.cooc_finalize(keys, counts, 1000, 5, 6, weighting="dynamic"))
    assert cnt.min() == 6 and (val < 6).any() and (val[cnt == 6] < 6).all()       # kept by their count, whatever their value
    everything = [t.cpu().numpy() for t in hip.cooc_finalize(keys, counts, 1000, 5, 0, weighting="dynamic")]
    keep = everything[2] >= 6
    for g, w in zip((row, col, cnt, val), everything):
        np.testing.assert_array_equal(g, w[keep])
    with pytest.raises(GloveHipError, match="weighting"):
        hip.cooc_finalize(keys, counts, 1000, 5, 0, weighting="linear")
    with pytest.raises(GloveHipError, match="capacity"):
        hip.cooc_finalize(keys, counts, 1000, 5, 0, cap=3, weighting="uniform")


# ---- end to end
class Backends(oref.NumpyBackend, text_ref.NumpyTextBackend):
    pass


def test_the_command_line_writes_the_files_of_the_numpy_backend(hip, tmp_path):
    from trainer import cooccur
    options = dict(subsample=0.005, subsample_seed=11, delete_unknown=True, window_weighting="dynamic")
    cooccur.main(str(CORPUS), tmp_path / "want", vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000, count_minimum=10,
                 seed=3, backend=Backends(), tokenizer="python", **options)
    want = [(tmp_path / "want" / f).read_bytes() for f in FILES + ("prep.json",)]
    assert len(want[2]) > 2000
    for chunk_tokens in (1000, 77):
        dest = tmp_path / ("got%d" % chunk_tokens)
        proc = subprocess.run([sys.executable, "-m", "trainer.cooccur", "--corpus", str(CORPUS), "--dest", str(dest), "--coverage", "0.9",
                               "--context-size", "5", "--chunk-tokens", str(chunk_tokens), "--count-minimum", "10", "--seed", "3",
                               "--tokenizer", "device", "--subsample", "0.005", "--subsample-seed", "11", "--delete-unknown",
                               "--window-weighting", "dynamic"], cwd=str(REPO), capture_output=True, text=True, timeout=240)
        assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
        assert [(dest / f).read_bytes() for f in FILES + ("prep.json",)] == want, chunk_tokens
