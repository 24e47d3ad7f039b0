"""The preprocessing options of the corpus-to-counts stage, without a GPU: subsampling, rare-word deletion and window
weightings of trainer.cooccur on the NumPy backend of tests/cooc_options_ref.py, and the surface and host-side argument
checks of the fourth header of libglove_prep_hip.so (include/glove_cooc_options_hip.h)."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

import cooc_options_ref as oref
import cooc_stream_ref
import text_ref
from test_analogy import BADARG, FAKE, WORKSPACE, declared_functions

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
CORPUS = GOLDEN / "text8_corpus.txt"
HEADER = REPO / "include" / "glove_cooc_options_hip.h"
FILES = ("vocab.csv", "vocab.txt", "interaction.csv")
KW = dict(vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000, count_minimum=10, seed=3)
SUBSAMPLE, SUBSAMPLE_SEED = 0.005, 11


class Backends(oref.NumpyBackend, text_ref.NumpyTextBackend):
    """Counting, filtering, weighting and tokenizing in NumPy: what trainer.cooccur drives with either tokenizer."""


class OldBackends(cooc_stream_ref.NumpyBackend, text_ref.NumpyTextBackend):
    """The backend as it was before the options: no `token_filter`, a `cooc_finalize` that knows no `weighting`."""


@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.PREP_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_prep_library()


def header_define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, HEADER.read_text()).group(1))


# ---- surface
def test_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADER)
    assert set(names) == set(hip_api.COOC_OPTIONS_EXPORTED_SYMBOLS)
    assert len(names) == len(hip_api.COOC_OPTIONS_EXPORTED_SYMBOLS) == 5          # the thresholds are made on the host
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_cooc_options_abi_version() == hip_api.GLOVE_COOC_OPTIONS_ABI_VERSION == 1
    assert header_define("GLOVE_COOC_OPTIONS_ABI_VERSION") == 1
    assert header_define("GLOVE_FILTER_TILE") == hip_api.FILTER_TILE
    assert {k: header_define("GLOVE_WINDOW_" + k.upper()) for k in oref.WEIGHTINGS} == hip_api.WINDOW_WEIGHTINGS \
        == {"harmonic": 0, "uniform": 1, "dynamic": 2}
    every = {k: v for k, v in vars(hip_api).items() if k.endswith("EXPORTED_SYMBOLS")}
    assert len(every) >= 10
    for k, v in every.items():
        if k != "COOC_OPTIONS_EXPORTED_SYMBOLS":
            assert not set(names) & set(v), k
    train = hip_api.load_library()
    assert not any(hasattr(train, n) for n in names)            # the prep library's, not the training library's
    # the other prep headers still say 1, and their symbol lists are what they were
    for header, macro in (("glove_cooc_stream_hip.h", "GLOVE_COOC_STREAM_ABI_VERSION"), ("glove_text_hip.h", "GLOVE_TEXT_ABI_VERSION"),
                          ("glove_vectors_hip.h", "GLOVE_VECTORS_ABI_VERSION")):
        assert "%s 1" % macro in (REPO / "include" / header).read_text() and getattr(hip_api, macro) == 1
    assert lib.glove_cooc_stream_abi_version() == lib.glove_text_abi_version() == lib.glove_vectors_abi_version() == 1
    assert (len(hip_api.PREP_EXPORTED_SYMBOLS), len(hip_api.TEXT_EXPORTED_SYMBOLS), len(hip_api.VECTORS_EXPORTED_SYMBOLS)) == (7, 8, 6)
    assert hip_api.GLOVE_ABI_VERSION == 15 and len(hip_api.EXPORTED_SYMBOLS) == 42


# ---- workspace
def test_workspace_queries_equal_the_stated_layouts(lib):
    from trainer import hip_api
    flt, fin = lib.glove_token_filter_workspace_bytes, lib.glove_cooc_finalize_weighted_workspace_bytes
    T = hip_api.FILTER_TILE
    up = lambda x: (x + 255) // 256 * 256
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 5, 10 ** 6, 64 << 20, 2 ** 31 - 1):
        tiles = max(1, -(-n // T))
        assert flt(n) == 2 * up(8 * tiles) + up((64 << 10) + 8 * tiles), n
    assert flt(-1) == 0 and flt(2 ** 31) == 0 and flt(1 << 40) == 0
    for cap in (0, 1, 1000, 10 ** 6, 1 << 40):
        assert fin(cap) == lib.glove_cooc_finalize_workspace_bytes(cap) > 0, cap
    m = 10 ** 6
    assert fin(m) == 2 * up(8 * m) + up((1 << 20) + m // 16)
    assert fin(-1) == 0 and fin((1 << 40) + 1) == 0


# ---- refusals, all before any launch
def test_argument_errors_are_reported_before_any_launch(lib):
    big = 1 << 30
    I, T, O, N = 0x100000, 0x400000, 0x700000, 0xA00000              # distinct "device" ranges, 3 MiB apart
    order = ("ids", "n", "pos0", "thr", "V", "seed", "out", "n_out", "cap", "ws", "ws_bytes", "stream")
    base = dict(ids=I, n=1000, pos0=0, thr=T, V=50, seed=0, out=O, n_out=N, cap=1000, ws=FAKE, ws_bytes=big, stream=None)
    flt = lambda **kw: lib.glove_token_filter_i32(*[{**base, **kw}[k] for k in order])
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(pos0=-1), dict(pos0=2 ** 63 - 1000, n=1001), dict(pos0=2 ** 63 - 1, n=1),
               dict(V=0), dict(V=-3), dict(cap=-1), dict(n_out=None), dict(ws=None), dict(ids=None), dict(thr=None), dict(out=None),
               dict(out=I), dict(out=I + 999 * 4), dict(out=I - 999 * 4), dict(out=I + 400, cap=10),      # ids_out over ids
               dict(out=T), dict(out=T + 49 * 4), dict(n_out=O), dict(n_out=O + 999 * 4), dict(n_out=I + 8), dict(n_out=T)):
        assert flt(**kw) == BADARG, kw
    assert flt(ws_bytes=16) == WORKSPACE
    assert flt(ws_bytes=lib.glove_token_filter_workspace_bytes(1000) - 1) == WORKSPACE
    A = 0x100000
    order = ("keys", "counts", "n", "cap_keys", "V", "context", "min_count", "weighting", "row", "col", "cnt", "val", "nnz",
             "cap_out", "ws", "ws_bytes", "stream")
    base = dict(keys=A, counts=A + 0x40000, n=A + 0x80000, cap_keys=100, V=5, context=3, min_count=0, weighting=2, row=O,
                col=O + 0x10000, cnt=O + 0x20000, val=O + 0x30000, nnz=O + 0x40000, cap_out=100, ws=FAKE, ws_bytes=big, stream=None)
    fz = lambda **kw: lib.glove_cooc_finalize_weighted(*[{**base, **kw}[k] for k in order])
    for kw in (dict(weighting=3), dict(weighting=-1), dict(weighting=255), dict(cap_keys=-1), dict(V=0), dict(context=256),
               dict(context=0), dict(cap_out=-1), dict(n=None), dict(nnz=None), dict(ws=None), dict(keys=None), dict(counts=None),
               dict(row=None), dict(val=None), dict(V=1_400_000_000, context=5)):
        assert fz(**kw) == BADARG, kw
    for w in (0, 1, 2):
        assert fz(weighting=w, ws_bytes=16) == WORKSPACE


# ---- the hash
def plain_u(seed, p):
    M = (1 << 64) - 1
    x = (p + (seed + 1) * 0x9E3779B97F4A7C15) & M
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M
    x ^= x >> 31
    return x >> 32


def test_the_hash_is_the_header_s_on_plain_python_ints():
    # the header states the hash with the constants and shifts the restatements use, in their order
    stated = re.search(r"x = p \+ \(seed \+ 1\) \* (0x[0-9A-F]+)\s*\*\s*x \^= x >> (\d+);\s*x \*= (0x[0-9A-F]+)\s*\*\s*x \^= x >> (\d+);"
                       r"\s*x \*= (0x[0-9A-F]+)\s*\*\s*x \^= x >> (\d+);\s*u = x >> (\d+)", HEADER.read_text())
    assert stated is not None
    assert [int(g, 0) for g in stated.groups()] == [oref.GOLDEN_GAMMA, 30, oref.MUL_A, 27, oref.MUL_B, 31, 32] \
        == [0x9E3779B97F4A7C15, 30, 0xBF58476D1CE4E5B9, 27, 0x94D049BB133111EB, 31, 32]
    rng = np.random.default_rng(3)
    edges = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7, 2 ** 63 - 1]
    ps = edges + [int(v) for v in rng.integers(0, 2 ** 63 - 1, 60)] + [int(v) for v in rng.integers(0, 2 ** 20, 20)]
    seeds = [0, 1, 7, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    assert len(ps) * len(seeds) > 300
    for seed in seeds:
        got = oref.hash_u(seed, np.asarray(ps, np.uint64))
        assert got.dtype == np.uint32
        assert got.tolist() == [plain_u(seed, p) for p in ps], seed
    # the definition, pinned: u(s, 0) is the high half of SplitMix64's output number s + 1 from state 0
    literal = {(0, 0): 0xE220A839, (0, 1): 0x910A2DEC, (0, 2 ** 32 - 1): 0x73B13BA2, (0, 2 ** 32): 0xC42C5A1A,
               (0, 2 ** 40 + 7): 0xB94083AA, (1, 0): 0x6E789E6A, (7, 12345): 0x6E7411B0, (2 ** 64 - 1, 5): 0xB6BF613D,
               (2 ** 63, 2 ** 62): 0x09590F27}
    for (seed, p), want in literal.items():
        assert plain_u(seed, p) == want == int(oref.hash_u(seed, np.asarray([p], np.uint64))[0]), (seed, p)


def test_reference_filter_and_thresholds():
    thr = np.asarray([0xFFFFFFFF, 0, 1 << 31, 1], np.uint32)
    ids = np.tile(np.arange(4, dtype=np.int32), 5000)
    got = oref.token_filter(ids, 2 ** 32 - 3, thr, 5)
    assert (got == 0).sum() == 5000 and (got == 1).sum() == 0 and 2300 < (got == 2).sum() < 2700 and (got == 3).sum() <= 1
    cut = 777                                                      # a block's survivors do not depend on where it was cut
    parts = [oref.token_filter(ids[:cut], 2 ** 32 - 3, thr, 5), oref.token_filter(ids[cut:], 2 ** 32 - 3 + cut, thr, 5)]
    np.testing.assert_array_equal(np.concatenate(parts), got)
    counts = np.asarray([500, 300, 150, 40, 9, 1, 0], np.int64)
    t = oref.thresholds(counts, 0.04)
    assert t.dtype == np.uint32 and t.tolist()[3:] == [0xFFFFFFFF] * 4                    # f = 0.04 is q = 1 exactly
    assert t.tolist()[:3] == [int(np.floor(np.sqrt(0.04 / f) * 2 ** 32)) for f in (0.5, 0.3, 0.15)]
    assert oref.thresholds(counts, 0).tolist() == [0xFFFFFFFF] * 7
    assert oref.thresholds(counts, 0.04, True).tolist() == [0] + t.tolist()[1:]
    from trainer import cooccur
    for T, delete in ((0.0, False), (0.04, False), (0.04, True), (1e-5, True), (0.3, False), (0.999, False)):
        np.testing.assert_array_equal(cooccur.subsample_thresholds(counts, T, delete), oref.thresholds(counts, T, delete))
    for bad in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="subsample"):
            cooccur.subsample_thresholds(counts, bad)


# ---- the driver on the golden corpus
def run_main(dest, backend=None, **kw):
    from trainer import cooccur
    cooccur.main(str(CORPUS), dest, backend=backend or Backends(), **{**KW, **kw})
    return [(dest / f).read_bytes() for f in FILES]


@pytest.fixture(scope="module")
def golden():
    """(vocab, the raw id stream, its stream counts): the golden corpus as process_corpus numbers it, computed once."""
    from trainer import cooccur, text8
    tokens = CORPUS.read_text().split()
    vocab = text8.create_vocabulary(tokens, None, 0.9)
    ids = text8.token_ids(tokens, vocab[0])
    counts = cooccur.stream_counts(vocab)
    np.testing.assert_array_equal(counts, np.bincount(ids, minlength=len(vocab[0])))     # id 0 carries everything out of vocabulary
    assert vocab[0].index("<UNK>") != 0 and counts[vocab[0].index("<UNK>")] == 0          # ... which here is not "<UNK>"'s id
    return vocab, ids, counts


def expected_files(dest, vocab, row, col, cnt, val):
    """The three files from a finished (row, col, count, value) table, by the functions the driver had before the options."""
    from trainer import text8
    table = text8.interaction_columns(row, col, cnt, val, vocab, KW["seed"])
    text8.save_data({"vocabulary": vocab, "interaction": text8.create_glove_table(table, KW["count_minimum"])}, dest)
    return [(dest / f).read_bytes() for f in FILES]


@pytest.mark.parametrize("tokenizer", ["python", "device"])
def test_default_flags_write_the_files_they_always_wrote(tmp_path, golden, tokenizer):
    vocab, ids, _ = golden
    # the old backend has no token_filter and its cooc_finalize takes no weighting: no filter stage, the old finalize call
    got = run_main(tmp_path / "got", backend=OldBackends(), tokenizer=tokenizer, block_bytes=4096)
    table = cooc_stream_ref.finalize(*cooc_stream_ref.chunk_keys(ids, len(ids), len(vocab[0]), 5), len(vocab[0]), 5, 10)
    assert got == expected_files(tmp_path / "want", vocab, *table)
    assert got[1] == (GOLDEN / "text8_cov90_ctx5_vocab.txt").read_bytes()
    assert not (tmp_path / "got" / "prep.json").exists()
    explicit = run_main(tmp_path / "explicit", tokenizer=tokenizer, subsample=0.0, subsample_seed=0, delete_unknown=False,
                        window_weighting="harmonic")
    assert explicit == got and not (tmp_path / "explicit" / "prep.json").exists()


@pytest.fixture(scope="module")
def filtered(golden):
    """(the thresholds, the filtered id list, its one-shot tables by brute force under the three weightings)."""
    vocab, ids, counts = golden
    thr = oref.thresholds(counts, SUBSAMPLE, delete_unknown=True)
    kept = oref.token_filter(ids, 0, thr, SUBSAMPLE_SEED)
    assert 1000 < len(kept) < len(ids) - counts[0] and not (kept == 0).any()
    return thr, kept, {w: oref.brute_force_table(kept, len(vocab[0]), 5, 10, w) for w in oref.WEIGHTINGS}


@pytest.mark.parametrize("tokenizer, chunk_tokens, block_bytes", [("python", 1, 16 << 20), ("python", 7, 4096), ("python", 4096, 100),
                                                                  ("device", 7, 4096), ("device", 4096, 333), ("device", 1000, 16 << 20)])
def test_filtered_files_equal_counting_the_filtered_ids_in_one_shot(tmp_path, golden, filtered, tokenizer, chunk_tokens, block_bytes):
    vocab, ids, _ = golden
    _, kept, tables = filtered
    got = run_main(tmp_path / "got", tokenizer=tokenizer, chunk_tokens=chunk_tokens, block_bytes=block_bytes, subsample=SUBSAMPLE,
                   subsample_seed=SUBSAMPLE_SEED, delete_unknown=True)
    want = expected_files(tmp_path / "want", vocab, *tables["harmonic"])
    assert got == want and len(got[2]) > 2000
    # the vocabulary files are the raw corpus's
    assert got[1] == (GOLDEN / "text8_cov90_ctx5_vocab.txt").read_bytes()
    prep = json.loads((tmp_path / "got" / "prep.json").read_text())
    assert prep == {"subsample": SUBSAMPLE, "subsample_seed": SUBSAMPLE_SEED, "delete_unknown": True, "window_weighting": "harmonic",
                    "tokens_read": len(ids), "tokens_kept": len(kept)}


def test_the_harmonic_brute_force_is_the_stream_reference(golden, filtered):
    vocab, _, _ = golden
    _, kept, tables = filtered
    V = len(vocab[0])
    keys, counts = cooc_stream_ref.chunk_keys(kept, len(kept), V, 5)
    for g, w in zip(cooc_stream_ref.finalize(keys, counts, V, 5, 10), tables["harmonic"]):
        assert g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)
    for weighting in oref.WEIGHTINGS:
        for g, w in zip(oref.finalize_weighted(keys, counts, V, 5, 10, weighting), tables[weighting]):
            assert g.dtype == w.dtype
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("weighting", ["uniform", "dynamic"])
@pytest.mark.parametrize("with_filter", [False, True])
def test_window_weightings_equal_the_brute_force_weights_exactly(tmp_path, golden, filtered, weighting, with_filter):
    vocab, ids, _ = golden
    _, kept, tables = filtered
    V = len(vocab[0])
    options = dict(subsample=SUBSAMPLE, subsample_seed=SUBSAMPLE_SEED, delete_unknown=True) if with_filter else {}
    got = run_main(tmp_path / "got", chunk_tokens=997, window_weighting=weighting, **options)
    table = tables[weighting] if with_filter else oref.brute_force_table(ids, V, 5, 10, weighting)
    assert got == expected_files(tmp_path / "want", vocab, *table)
    row, col, cnt, val = table
    if weighting == "uniform":
        np.testing.assert_array_equal(val, cnt.astype(np.float64))
    else:                                               # every distance weighs between 1 / context and 1
        assert (val <= cnt).all() and (val * 5 >= cnt).all() and (val < cnt).any()
    prep = json.loads((tmp_path / "got" / "prep.json").read_text())
    assert prep["window_weighting"] == weighting and prep["tokens_read"] == len(ids)
    assert prep["tokens_kept"] == (len(kept) if with_filter else len(ids)) and prep["delete_unknown"] == with_filter


def test_filter_blocks_keeps_the_running_position(golden, filtered):
    from trainer import cooccur
    _, ids, _ = golden
    thr, kept, _ = filtered
    for cuts in ([], [1], [1, 2, 3], [777, 778, 4000], list(range(0, 5000, 64))):
        totals = {}
        blocks = np.split(ids, cuts)
        out = list(cooccur.filter_blocks(iter(blocks), thr, SUBSAMPLE_SEED, Backends(), totals))
        np.testing.assert_array_equal(np.concatenate(out), kept)
        assert totals == {"read": len(ids), "kept": len(kept)} and all(len(o) for o in out)
    assert not np.array_equal(oref.token_filter(ids, 0, thr, SUBSAMPLE_SEED + 1), kept)      # the seed matters
    assert not np.array_equal(oref.token_filter(ids, 1, thr, SUBSAMPLE_SEED), kept)          # ... and so does the position


def test_bad_options_are_refused():
    from trainer import cooccur
    for kw in (dict(subsample=1.0), dict(subsample=-1e-3), dict(subsample=float("nan")), dict(window_weighting="linear")):
        with pytest.raises(ValueError):
            cooccur.process_corpus(str(CORPUS), backend=Backends(), **{**KW, **kw})
    acc = cooccur.CoocAccumulator(5, 2, Backends())
    acc.add(np.asarray([1, 2, 3, 1], np.int32), 4)
    with pytest.raises(ValueError, match="weighting"):
        acc.finalize(0, "linear")


# ---- subsampling statistics
def test_kept_counts_lie_within_five_binomial_standard_deviations(golden):
    vocab, ids, counts = golden
    thr = oref.thresholds(counts, SUBSAMPLE)
    q = oref.keep_probability(thr)
    assert (q < 1).sum() >= 5
    kept = np.bincount(oref.token_filter(ids, 0, thr, SUBSAMPLE_SEED), minlength=len(counts))
    checked = 0
    for w in np.flatnonzero(q < 1):
        n, expect = int(counts[w]), counts[w] * q[w]
        np.testing.assert_allclose(q[w], np.sqrt(SUBSAMPLE / (n / len(ids))), rtol=1e-8)
        if expect < 20:
            continue
        sd = np.sqrt(n * q[w] * (1 - q[w]))
        assert abs(kept[w] - expect) <= 5 * sd, (w, vocab[0][w], n, q[w], int(kept[w]), expect, sd)
        checked += 1
    assert checked >= 5
    np.testing.assert_array_equal(kept[q >= 1], counts[q >= 1])                                # words at q = 1 are never touched
