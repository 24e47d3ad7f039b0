"""Counting a corpus chunk by chunk, without a GPU: trainer.cooccur (block reader, chunker, CoocAccumulator, the CLI) on
the NumPy backend of tests/cooc_stream_ref.py, and the surface and host-side argument checks of libglove_prep_hip.so
(include/glove_cooc_stream_hip.h)."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import cooc_stream_ref
import glove_ref as ref
from test_analogy import BADARG, FAKE, declared_functions

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
HEADER = REPO / "include" / "glove_cooc_stream_hip.h"
CASES = {"cov100_ctx2": 2, "cov90_ctx5": 5}


def golden_ids(tag):
    tokens = (GOLDEN / "text8_corpus.txt").read_text().split()
    token2id = {t: i for i, t in enumerate((GOLDEN / ("text8_%s_vocab.txt" % tag)).read_text().split("\n"))}
    return np.asarray([token2id.get(t, 0) for t in tokens], np.int32), len(token2id)


def streamed(ids, V, context, chunk_tokens, min_count=0, backend=None):
    from trainer.cooccur import CoocAccumulator, iter_chunks
    acc = CoocAccumulator(V, context, backend or cooc_stream_ref.NumpyBackend())
    owned = 0
    for piece, n_own in iter_chunks([ids], chunk_tokens, context):
        assert len(piece) - n_own == min(context, len(ids) - owned - n_own)      # the halo: min(context, tokens left)
        np.testing.assert_array_equal(piece, ids[owned:owned + len(piece)])
        acc.add(piece, n_own)
        owned += n_own
    assert owned == len(ids)
    if acc.keys is None:
        acc.add(np.zeros(0, np.int32), 0)
    return acc.finalize(min_count)


@pytest.fixture(scope="module", params=sorted(CASES))
def golden_case(request):
    """(ids, V, context, the single-chunk table, the oracle's table, the golden csv): computed once per window."""
    tag = request.param
    ids, V = golden_ids(tag)
    context = CASES[tag]
    return (ids, V, context, streamed(ids, V, context, len(ids)), ref.cooccurrence(ids, context),
            pd.read_csv(GOLDEN / ("text8_%s_cooccurrence.csv" % tag)))


# ---- chunking on the golden corpus
def test_single_chunk_equals_the_oracle_and_the_golden_table(golden_case):
    ids, V, context, whole, want, csv = golden_case
    np.testing.assert_array_equal(whole[0], want[0])
    np.testing.assert_array_equal(whole[1], want[1])
    np.testing.assert_array_equal(whole[2], want[2])
    np.testing.assert_allclose(whole[3], want[3], rtol=1e-12)
    np.testing.assert_array_equal(whole[0], csv["row_token_id"])
    np.testing.assert_array_equal(whole[1], csv["col_token_id"])
    np.testing.assert_array_equal(whole[2], csv["count"])
    np.testing.assert_allclose(whole[3], csv["value"], rtol=1e-12)


@pytest.mark.parametrize("chunk", [1, 7, 997, "n", "n+5"])
def test_every_chunking_gives_the_single_chunk_arrays(golden_case, chunk):
    ids, V, context, whole, _, _ = golden_case
    chunk = {"n": len(ids), "n+5": len(ids) + 5}.get(chunk, chunk)
    got = streamed(ids, V, context, chunk)
    for g, w in zip(got, whole):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)       # `value` too: the state holds integers, the cut cannot show


def test_min_count_is_the_host_filter(golden_case):
    ids, V, context, whole, _, _ = golden_case
    keep = whole[2] >= 10
    assert 0 < keep.sum() < len(keep)
    for g, w in zip(streamed(ids, V, context, 997, min_count=10), whole):
        np.testing.assert_array_equal(g, w[keep])


# ---- halo edges
@pytest.mark.parametrize("ids, context, chunk", [
    ([3, 1, 2], 5, 2),                          # a corpus shorter than the window
    ([3, 1, 2, 3, 0, 1, 4, 4, 2, 1, 0], 5, 2),  # chunks shorter than the window
    ([3, 1, 2, 3, 0, 1, 4], 3, 3),              # a last chunk of one token
    ([2], 3, 1),                                # one token: nothing to pair
    ([4, 4, 4, 4, 4, 4], 2, 4),                 # an all-equal corpus produces no keys
])
def test_halo_edges(ids, context, chunk):
    ids = np.asarray(ids, np.int32)
    got = streamed(ids, 5, context, chunk)
    whole = streamed(ids, 5, context, len(ids))
    want = ref.cooccurrence(ids, context)
    for g, w in zip(got, whole):
        np.testing.assert_array_equal(g, w)
    if len(want[0]):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_allclose(got[3], want[3], rtol=1e-12)
    else:
        assert all(len(g) == 0 for g in got)
    if len(set(ids.tolist())) == 1:
        assert len(got[0]) == 0


def test_a_pair_belongs_to_the_chunk_that_owns_its_left_position():
    tok = np.asarray([0, 1, 2, 3], np.int32)
    keys, counts = cooc_stream_ref.chunk_keys(tok, 1, 5, 3)         # own: position 0; halo: three tokens
    assert sorted(keys.tolist()) == sorted([(0 * 5 + b) * 3 + b - 1 for b in (1, 2, 3)] + [(b * 5 + 0) * 3 + b - 1 for b in (1, 2, 3)])
    assert counts.tolist() == [1] * 6
    assert len(cooc_stream_ref.chunk_keys(tok, 0, 5, 3)[0]) == 0


def test_the_state_buffers_swap_and_grow_geometrically():
    from trainer.cooccur import CoocAccumulator
    ids, V = golden_ids("cov90_ctx5")
    acc = CoocAccumulator(V, 5, cooc_stream_ref.NumpyBackend())
    caps, fronts = [], []
    for s in range(0, 400, 10):
        acc.add(ids[s:s + 15], 10)
        caps.append(len(acc._front[0]))
        fronts.append(id(acc._front[0]))
        assert len(acc) <= caps[-1] and np.all(np.diff(acc.keys) > 0)
    assert len(set(caps)) <= 2 + np.log2(caps[-1] / caps[0])       # allocations double: their number is logarithmic
    assert any(a != b for a, b in zip(fronts, fronts[1:]))


# ---- block reader
@pytest.mark.parametrize("block_bytes", [1, 2, 3, 4096])
def test_block_reader_returns_the_split_of_the_text(tmp_path, block_bytes):
    from trainer.cooccur import iter_token_blocks
    text = "  \n alpha  beta\n\ngamma\t delta   a_token_that_is_far_longer_than_any_small_block  x y\n z   \n "
    path = tmp_path / "corpus.txt"
    path.write_text(text)
    blocks = list(iter_token_blocks(path, block_bytes))
    assert [t for b in blocks for t in b] == text.split()
    assert all(blocks)
    for other in ("", "   \n", "one", "no_trailing space", "é ü ß"):
        path.write_text(other)
        assert [t for b in iter_token_blocks(path, block_bytes) for t in b] == other.split(), other


# ---- the library: workspace queries, surface, argument checks (all before any launch)
@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.PREP_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_prep_library()


def test_workspace_queries_are_pure_host_functions(lib):
    from trainer import hip_api
    chunk, merge, fin = lib.glove_cooc_chunk_workspace_bytes, lib.glove_cooc_merge_workspace_bytes, lib.glove_cooc_finalize_workspace_bytes
    # zero for sizes the calls would refuse
    for bad in ((-1, 5), (100, 0), (100, 256), (100, -3), (2 ** 32 // 10 + 1, 5), (1 << 40, 1)):
        assert chunk(*bad) == 0, bad
    assert chunk(2 ** 32 // 10, 5) > 0 and chunk(0, 5) > 0 and chunk(100, 255) > 0
    for bad in ((-1, 5), (5, -1), ((1 << 40) + 1, 0), (1 << 39, (1 << 39) + 1)):
        assert merge(*bad) == 0, bad
    assert merge(0, 0) > 0 and merge(1 << 39, 1 << 39) > 0
    assert fin(-1) == 0 and fin((1 << 40) + 1) == 0 and fin(0) > 0 and fin(1 << 40) > 0
    # monotone in their arguments
    sizes = [0, 1, 1000, 2047, 2048, 2049, 10 ** 6, 10 ** 8]
    for a, b in zip(sizes, sizes[1:]):
        assert chunk(a, 5) <= chunk(b, 5) and chunk(10 ** 6, 5) <= chunk(10 ** 6, 6)
        assert merge(a, 7) <= merge(b, 7) and merge(7, a) <= merge(7, b) and fin(a) <= fin(b)
    assert chunk(10 ** 6, 5) < chunk(10 ** 7, 5) and merge(10 ** 6, 0) < merge(10 ** 7, 0) and fin(10 ** 6) < fin(10 ** 7)
    # the merge's layout, as the header states it
    up = lambda x: (x + 255) // 256 * 256
    tiles = (10 ** 6 + 12345 + hip_api.COOC_MERGE_TILE - 1) // hip_api.COOC_MERGE_TILE
    assert merge(10 ** 6, 12345) == 2 * up(8 * (tiles + 1)) + 2 * up(8 * tiles) + up((64 << 10) + 8 * tiles)
    # a billion tokens at window 10 do not fit the one-shot call; a 32 Mi-token chunk costs what the one-shot call costs
    # on as many tokens
    one_shot = hip_api.load_library().glove_cooc_workspace_bytes
    assert one_shot(10 ** 9, 10) > 288e9
    n = 32 * 2 ** 20 + 10
    assert abs(chunk(n, 10) - one_shot(n, 10)) <= 4096
    # ... which is the one-shot call on the chunk's 32 Mi own tokens plus the halo's 10 x 20 slots of 52 B
    assert abs(chunk(n, 10) - one_shot(32 * 2 ** 20, 10) - 10 * 20 * 52) <= 4096
    assert chunk(n, 10) < 288e9 / 8


def test_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADER)
    assert set(names) == set(hip_api.PREP_EXPORTED_SYMBOLS) and len(names) == len(hip_api.PREP_EXPORTED_SYMBOLS) == 7
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_cooc_stream_abi_version() == hip_api.GLOVE_COOC_STREAM_ABI_VERSION == 1
    text = HEADER.read_text()
    assert "GLOVE_COOC_STREAM_ABI_VERSION 1" in text
    assert "GLOVE_COOC_MERGE_TILE %d" % hip_api.COOC_MERGE_TILE in text
    others = set(hip_api.EXPORTED_SYMBOLS) | set(hip_api.EVAL_EXPORTED_SYMBOLS) | set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS) \
        | set(hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS)
    assert not set(names) & others
    train = hip_api.load_library()
    assert not any(hasattr(train, n) for n in names)            # a library of its own
    assert hip_api.GLOVE_ABI_VERSION == 15 and len(hip_api.EXPORTED_SYMBOLS) == 42


def test_missing_prep_library_is_an_error_not_a_fallback(tmp_path):
    from trainer import hip_api
    with pytest.raises(hip_api.GloveHipError, match="no CPU fallback"):
        hip_api.load_prep_library(tmp_path / "libglove_prep_hip.so")


def test_argument_errors_are_reported_before_any_launch(lib):
    big = 1 << 30
    ck = lambda **kw: lib.glove_cooc_chunk_keys_i32(*[{**dict(tokens=FAKE, n_own=10, n_total=12, V=5, context=3, keys=FAKE,
                                                           counts=FAKE, n_out=FAKE, cap=100, ws=FAKE, ws_bytes=big,
                                                           stream=None), **kw}[k]
                                                      for k in ("tokens", "n_own", "n_total", "V", "context", "keys", "counts",
                                                                "n_out", "cap", "ws", "ws_bytes", "stream")])
    for kw in (dict(n_own=-1), dict(n_total=9), dict(V=0), dict(context=0), dict(context=256), dict(V=1_400_000_000, context=5),
               dict(cap=-1), dict(n_out=None), dict(ws=None), dict(tokens=None), dict(keys=None),
               dict(n_own=2 ** 32 // 6, n_total=2 ** 32 // 6 + 3)):
        assert ck(**kw) == BADARG, kw
    assert ck(ws_bytes=16) == -2                                     # GLOVE_E_WORKSPACE
    A, B, O = 0x100000, 0x200000, 0x300000                           # distinct "device" ranges, 1 MiB apart
    mg = lambda **kw: lib.glove_cooc_merge_u64(*[{**dict(ka=A, ca=A + 0x40000, na=A + 0x80000, cap_a=100, kb=B, cb=B + 0x40000,
                                                      nb=B + 0x80000, cap_b=50, ko=O, co=O + 0x40000, no=O + 0x80000, cap_out=150,
                                                      ws=FAKE, ws_bytes=big, stream=None), **kw}[k]
                                                 for k in ("ka", "ca", "na", "cap_a", "kb", "cb", "nb", "cap_b", "ko", "co", "no",
                                                           "cap_out", "ws", "ws_bytes", "stream")])
    for kw in (dict(cap_a=-1), dict(cap_b=-1), dict(cap_out=-1), dict(na=None), dict(nb=None), dict(no=None), dict(ws=None),
               dict(ka=None), dict(cb=None), dict(ko=None), dict(cap_a=(1 << 40) + 1),
               dict(ko=A), dict(ko=A + 99 * 8), dict(ko=A - 149 * 8), dict(co=A), dict(ko=B + 8), dict(co=B + 0x40000),
               dict(ko=A + 0x40000), dict(no=A + 0x80000), dict(no=B + 0x80000), dict(no=A + 8), dict(co=O), dict(no=O + 8)):
        assert mg(**kw) == BADARG, kw
    assert mg(ws_bytes=16) == -2
    fz = lambda **kw: lib.glove_cooc_finalize(*[{**dict(keys=A, counts=A + 0x40000, n=A + 0x80000, cap_keys=100, V=5, context=3,
                                                     min_count=0, row=O, col=O + 0x10000, cnt=O + 0x20000, val=O + 0x30000,
                                                     nnz=O + 0x40000, cap_out=100, ws=FAKE, ws_bytes=big, stream=None), **kw}[k]
                                                for k in ("keys", "counts", "n", "cap_keys", "V", "context", "min_count", "row", "col",
                                                          "cnt", "val", "nnz", "cap_out", "ws", "ws_bytes", "stream")])
    for kw in (dict(cap_keys=-1), dict(V=0), dict(context=256), dict(cap_out=-1), dict(n=None), dict(nnz=None), dict(ws=None),
               dict(keys=None), dict(counts=None), dict(row=None), dict(val=None)):
        assert fz(**kw) == BADARG, kw
    assert fz(ws_bytes=16) == -2


# ---- the CLI, end to end on the NumPy backend
def test_cli_writes_files_the_trainer_reads(tmp_path):
    from trainer import cooccur, data_utils, text8
    corpus = GOLDEN / "text8_corpus.txt"
    cooccur.main(str(corpus), tmp_path, vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000, count_minimum=10, seed=3,
                 backend=cooc_stream_ref.NumpyBackend())
    assert (tmp_path / "vocab.txt").read_text() == (GOLDEN / "text8_cov90_ctx5_vocab.txt").read_text()
    got, want = (pd.read_csv(f, keep_default_na=False, na_filter=False)
                 for f in (tmp_path / "vocab.csv", GOLDEN / "text8_cov90_ctx5_vocab.csv"))
    assert list(got["token"]) == list(want["token"]) and list(got["count"]) == list(want["count"])
    np.testing.assert_allclose(got["proportion"], want["proportion"], rtol=1e-12)
    got = pd.read_csv(tmp_path / "interaction.csv", keep_default_na=False, na_filter=False)
    want = pd.read_csv(GOLDEN / "text8_cov90_ctx5_interaction.csv", keep_default_na=False, na_filter=False)
    assert list(got.columns) == list(want.columns) and len(got.columns) == 9 and len(got) == len(want)
    # the same rows in another order (the permutation is drawn over the filtered rows)
    key = ["row_token_id", "col_token_id"]
    got, want = got.sort_values(key).reset_index(drop=True), want.sort_values(key).reset_index(drop=True)
    for c in want.columns:
        if not pd.api.types.is_numeric_dtype(want[c]):
            assert (got[c] == want[c]).all(), c
        else:
            np.testing.assert_allclose(got[c], want[c], rtol=1e-12, err_msg=c)
    coo = data_utils.load_interaction_csv(str(tmp_path / "interaction.csv"), str(tmp_path / "vocab.txt"))
    assert len(coo["row"]) == len(want) and coo["w"].min() > 0
    # the vocabulary of a Counter kept block by block is create_vocabulary's
    tokens = corpus.read_text().split()
    a = text8.create_vocabulary(tokens, None, 0.9)
    b = text8.vocabulary_from_counts(cooccur.count_vocabulary(corpus, 1000), None, 0.9)
    assert a[0] == b[0] and (a[1] == b[1]).all()
