"""The fifth header of libglove_prep_hip.so on the GPU (include/glove_phrases_hip.h): a block's bigram table, the selection
of the accepted phrases and the join, each against the NumPy restatement of tests/phrases_ref.py bit for bit (scores as
their bit patterns) at every tile edge, with poison behind every capacity; `trainer.phrases` on GloveHip against the same
driver on the NumPy backend, file for file."""
import collections
from pathlib import Path

import numpy as np
import pytest
import torch

import cooc_stream_ref
import phrases_cases as cases
import phrases_ref as pref
import text_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
KEY_POISON, COUNT_POISON, SCORE_POISON, BYTE_POISON = 0x0123456789ABCDEF, -0x0FEDCBA987654321, -7.25, 0xA5
EDGES = cases.edge_cases()


class Backends(pref.NumpyPhrasesBackend, text_ref.NumpyTextBackend, cooc_stream_ref.NumpyBackend):
    """The reference backend trainer.phrases runs on."""


def tile():
    from trainer.hip_api import PHRASE_TILE
    return PHRASE_TILE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def number(data: bytes, min_count: int, n_tokens=None):
    """The block as the device sees it, by text_ref: (bytes uint8, start, length, ids, unigram, tokens): kept words (count >=
    min_count) numbered 1 .. by count descending, ties by first occurrence; everything else 0.  n_tokens: the first so many."""
    spans = text_ref.token_spans(data)
    if n_tokens is not None:
        assert len(spans) >= n_tokens
        spans = spans[:n_tokens]
        data = data[:spans[-1][0] + spans[-1][1] + 1] if spans else b""
    words = [data[s:s + n] for s, n in spans]
    counts = collections.Counter(words)
    first = {}
    for t, w in enumerate(words):
        first.setdefault(w, t)
    kept = sorted((w for w in counts if counts[w] >= min_count), key=lambda w: (-counts[w], first[w]))
    ident = {w: i + 1 for i, w in enumerate(kept)}
    ids = np.asarray([ident.get(w, 0) for w in words], np.int32)
    unigram = np.asarray([len(words) - sum(counts[w] for w in kept)] + [counts[w] for w in kept], np.int64)
    return (np.frombuffer(data, np.uint8).copy(), np.asarray([s for s, _ in spans], np.int32), np.asarray([n for _, n in spans], np.int32),
            ids, unigram, len(words))


@pytest.fixture(scope="module")
def corpus():
    """One generated corpus, numbered once and left unchanged: (data, block arrays, its whole bigram table by the reference)."""
    data = cases.generated(1)
    arrays = number(data, 5)
    block, start, length, ids, unigram, tokens = arrays
    table = pref.bigram_keys(block, start, length, ids)
    assert tokens >= 6000 and len(table[0]) > 2000 and (ids == 0).any()
    return data, arrays, table


# ---- bigram keys
def bigram_raw(hip, block, start, length, ids, n_tokens, cap):
    keys = torch.full((cap + GUARD,), KEY_POISON, dtype=torch.int64, device=DEV)
    counts = torch.full((cap + GUARD,), COUNT_POISON, dtype=torch.int64, device=DEV)
    sizes = torch.tensor([n_tokens, -1, -1], dtype=torch.int64).to(DEV)
    hip.phrase_bigram_keys_enqueue(dev(block), dev(start), dev(length), dev(ids), sizes[0:1], keys[:cap], counts[:cap], sizes[1:3])
    torch.cuda.synchronize()
    return int(sizes[1].item()), host(keys), host(counts)


@pytest.mark.parametrize("tiles, more", [(0, 0), (0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (3, 5)])
def test_bigram_keys_at_every_tile_edge(hip, corpus, tiles, more):
    n = tiles * tile() + more
    block, start, length, ids, _, _ = number(corpus[0], 5, n)
    assert len(ids) == n
    want_keys, want_counts = pref.bigram_keys(block, start, length, ids)
    m = len(want_keys)
    assert n < 3 or m > 0
    got_n, keys, counts = bigram_raw(hip, block, start, length, ids, n, m + 5)
    assert got_n == m
    np.testing.assert_array_equal(keys[:m], want_keys)
    np.testing.assert_array_equal(counts[:m], want_counts)
    assert (keys[m:] == KEY_POISON).all() and (counts[m:] == COUNT_POISON).all()
    if m > 4:                                       # too small a capacity: the true size, nothing at or beyond the capacity
        cap = m - 3
        got_n, keys, counts = bigram_raw(hip, block, start, length, ids, n, cap)
        assert got_n == m
        np.testing.assert_array_equal(keys[:cap], want_keys[:cap])
        np.testing.assert_array_equal(counts[:cap], want_counts[:cap])
        assert (keys[cap:] == KEY_POISON).all() and (counts[cap:] == COUNT_POISON).all()
    # the wrapper, and a token count below the arrays' capacity: what lies behind it is not read as tokens
    if n:
        got = hip.phrase_bigram_keys(dev(block), dev(start), dev(length), dev(ids))
        np.testing.assert_array_equal(host(got[0]), want_keys)
        np.testing.assert_array_equal(host(got[1]), want_counts)
    if n > 7:
        short_keys, short_counts = pref.bigram_keys(block, start[:n - 7], length[:n - 7], ids[:n - 7])
        got_n, keys, counts = bigram_raw(hip, block, start, length, ids, n - 7, m + 5)
        assert got_n == len(short_keys)
        np.testing.assert_array_equal(keys[:got_n], short_keys)
        np.testing.assert_array_equal(counts[:got_n], short_counts)


# ---- select
def select_raw(hip, keys, counts, unigram, total, min_count, threshold, cap):
    out_keys = torch.full((cap + GUARD,), KEY_POISON, dtype=torch.int64, device=DEV)
    out_counts = torch.full((cap + GUARD,), COUNT_POISON, dtype=torch.int64, device=DEV)
    scores = torch.full((cap + GUARD,), SCORE_POISON, dtype=torch.float64, device=DEV)
    sizes = torch.tensor([len(keys), -1, -1], dtype=torch.int64).to(DEV)
    hip.phrase_select_enqueue(dev(keys), dev(counts), sizes[0:1], dev(unigram), total, min_count, threshold, out_keys[:cap],
                              out_counts[:cap], scores[:cap], sizes[1:3])
    torch.cuda.synchronize()
    return int(sizes[1].item()), host(out_keys), host(out_counts), host(scores)


def check_select(hip, keys, counts, unigram, total, min_count, threshold):
    want = pref.select(keys, counts, unigram, total, min_count, threshold)
    m = len(want[0])
    got_n, out_keys, out_counts, scores = select_raw(hip, keys, counts, unigram, total, min_count, threshold, m + 5)
    assert got_n == m
    np.testing.assert_array_equal(out_keys[:m], want[0])
    np.testing.assert_array_equal(out_counts[:m], want[1])
    np.testing.assert_array_equal(scores[:m].view(np.int64), want[2].view(np.int64))       # every bit of every score
    assert (out_keys[m:] == KEY_POISON).all() and (out_counts[m:] == COUNT_POISON).all() and (scores[m:] == SCORE_POISON).all()
    if m > 2:
        cap = m - 2
        got_n, out_keys, out_counts, scores = select_raw(hip, keys, counts, unigram, total, min_count, threshold, cap)
        assert got_n == m
        np.testing.assert_array_equal(out_keys[:cap], want[0][:cap])
        np.testing.assert_array_equal(scores[:cap].view(np.int64), want[2][:cap].view(np.int64))
        assert (out_keys[cap:] == KEY_POISON).all() and (out_counts[cap:] == COUNT_POISON).all() and (scores[cap:] == SCORE_POISON).all()
    return m


@pytest.mark.parametrize("min_count, threshold", [(5, 10.0), (5, 100.0), (1, 0.5), (2, 1e-9), (30, 1.0)])
def test_select_on_the_generated_table(hip, corpus, min_count, threshold):
    from trainer.hip_api import PHRASE_SELECT_TILE
    _, (block, start, length, ids, unigram, tokens), (keys, counts) = corpus
    assert len(keys) > 2 * PHRASE_SELECT_TILE                     # the table crosses three select tiles
    m = check_select(hip, keys, counts, unigram, tokens, min_count, threshold)
    assert m >= 3
    if min_count == 1:                                             # accepted keys in every tile
        accepted = pref.select(keys, counts, unigram, tokens, min_count, threshold)[0]
        at = np.searchsorted(keys, accepted) // PHRASE_SELECT_TILE
        assert set(at.tolist()) >= {0, 1, 2} and m > 500
    got = hip.phrase_select(dev(keys), dev(counts), dev(unigram), tokens, min_count, threshold)
    want = pref.select(keys, counts, unigram, tokens, min_count, threshold)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(host(g).view(np.int64), w.view(np.int64))


@pytest.mark.parametrize("name, threshold, accepted", [("score_equals_threshold", 4.0, 0), ("score_equals_threshold", 3.999, 1),
                                                       ("count_at_and_above_min_count", 1.0, 1), ("rare_word_in_strong_pair", 1.0, 1)])
def test_select_at_the_threshold_and_min_count_edges(hip, name, threshold, accepted):
    data, options, _ = EDGES[name]
    block, start, length, ids, unigram, tokens = number(data, options["min_count"])
    keys, counts = pref.bigram_keys(block, start, length, ids)
    assert check_select(hip, keys, counts, unigram, tokens, options["min_count"], threshold) == accepted
    if name == "score_equals_threshold":
        got = hip.phrase_select(dev(keys), dev(counts), dev(unigram), tokens, options["min_count"], 3.999)
        assert host(got[2]).tolist() == [4.0]                      # the score is the other case's threshold exactly: > is strict


# ---- join
def join_raw(hip, block, start, length, ids, phrase_keys, carry, delimiter=ord("_"), n_tokens=None):
    """glove_phrase_join_u8 on a poisoned buffer: (the buffer with its guard, carry out, joined, n_joined)."""
    buf = torch.full((len(block) + GUARD,), BYTE_POISON, dtype=torch.uint8, device=DEV)
    buf[:len(block)] = dev(block)
    carry_t = torch.tensor([carry], dtype=torch.int32).to(DEV)
    joined = torch.zeros(len(phrase_keys), dtype=torch.int64, device=DEV)
    sizes = torch.tensor([len(ids) if n_tokens is None else n_tokens, len(phrase_keys), -1, -1], dtype=torch.int64).to(DEV)
    hip.phrase_join_enqueue(buf[:len(block)], dev(start), dev(length), dev(ids), sizes[0:1], dev(phrase_keys), sizes[1:2], delimiter,
                            carry_t, joined, sizes[2:4])
    torch.cuda.synchronize()
    return host(buf), int(carry_t.item()), host(joined), int(sizes[2].item())


def check_join(hip, block, start, length, ids, phrase_keys, carry, delimiter=ord("_")):
    want_block, want_carry, want_joined = block.copy(), np.asarray([carry], np.int32), np.zeros(len(phrase_keys), np.int64)
    want_n = pref.join(want_block, start, length, ids, phrase_keys, delimiter, want_carry, want_joined)
    buf, got_carry, joined, got_n = join_raw(hip, block, start, length, ids, phrase_keys, carry, delimiter)
    np.testing.assert_array_equal(buf[:len(block)], want_block)                # the whole buffer: only chosen separators differ
    assert (buf[len(block):] == BYTE_POISON).all()
    assert (got_carry, got_n) == (int(want_carry[0]), want_n) and got_n == int((want_block != block).sum())
    np.testing.assert_array_equal(joined, want_joined)
    return want_block.tobytes(), got_carry, got_n


XY_KEYS = np.asarray([(1 << 32) | 2, (2 << 32) | 1], np.int64)


def pattern_block(cand):
    """x y x y ... with a single space where cand[t], a newline elsewhere; x = 1, y = 2 and both orders are accepted, so the
    candidates are exactly `cand`.  -> (block arrays, the joined bytes under the greedy rule read left to right, per carry)."""
    n = len(cand) + 1
    data = bytearray(cases.alternating(n))
    for t in np.flatnonzero(~cand):
        data[2 * t + 1] = 0x0A
    block = np.frombuffer(bytes(data), np.uint8).copy()
    start = np.arange(n, dtype=np.int32) * 2
    ids = (np.arange(n) % 2 + 1).astype(np.int32)
    want = {}
    for carry in (0, 1):
        out, prev = bytearray(data), bool(carry)
        for t in range(n - 1):
            prev = bool(cand[t]) and not prev
            if prev:
                out[2 * t + 1] = ord("_")
        want[carry] = (bytes(out), int(prev))
    return (block, start, np.ones(n, np.int32), ids), want


@pytest.mark.parametrize("carry", [0, 1])
def test_join_one_run_across_three_tiles(hip, carry):
    n = 3 * tile() + 5
    (block, start, length, ids), want = pattern_block(np.ones(n - 1, bool))
    got, carry_out, joins = check_join(hip, block, start, length, ids, XY_KEYS, carry)
    assert got == cases.alternating_joined(n, flipped=bool(carry)) == want[carry][0]
    assert got.startswith(b"x y_x y_x" if carry else b"x_y x_y x") and carry_out == want[carry][1]
    assert joins == (n - 1 - carry + 1) // 2


def tile_patterns():
    T = tile()
    n = 3 * T + 5
    straddle = np.zeros(n - 1, bool)
    straddle[[T - 1, T, 5, 6, 7, 2 * T - 2, 2 * T - 1, 2 * T, 2 * T + 1]] = True     # a run in tile 0's last pair and tile 1's first
    full_tile = np.ones(n - 1, bool)
    full_tile[[3, T - 4, 2 * T + 9, 3 * T + 1]] = False               # tile 1 holds no non-candidate; tiles 0, 2 and 3 do
    rng = np.random.default_rng(7)
    return {"straddle": straddle, "full_tile": full_tile, "none": np.zeros(n - 1, bool), "random": rng.random(n - 1) < 0.6,
            "dense": rng.random(n - 1) < 0.97}


@pytest.mark.parametrize("carry", [0, 1])
@pytest.mark.parametrize("name", ["straddle", "full_tile", "none", "random", "dense"])
def test_join_runs_across_tile_edges(hip, name, carry):
    cand = tile_patterns()[name]
    (block, start, length, ids), want = pattern_block(cand)
    got, carry_out, _ = check_join(hip, block, start, length, ids, XY_KEYS, carry)
    assert got == want[carry][0] and carry_out == want[carry][1]


@pytest.mark.parametrize("carry", [0, 1])
def test_join_of_short_blocks_leaves_the_carry(hip, carry):
    for data in (b"", b" \n ", b"x", b" x\n"):
        block, start, length, _, _, _ = number(data, 1)
        ids = np.ones(len(start), np.int32)
        got, carry_out, joins = check_join(hip, block, start, length, ids, XY_KEYS, carry)
        assert (got, carry_out, joins) == (data, carry, 0)
    # two tokens are one pair: the carry decides it and is written
    block, start, length, _, _, _ = number(b"x y", 1)
    got, carry_out, joins = check_join(hip, block, start, length, np.asarray([1, 2], np.int32), XY_KEYS, carry)
    assert (got, carry_out, joins) == ((b"x y", 0, 0) if carry else (b"x_y", 1, 1))
    # a token count below the arrays' capacity: the pairs behind it are no pairs
    (block, start, length, ids), _ = pattern_block(np.ones(9, bool))
    buf, carry_out, joined, joins = join_raw(hip, block, start, length, ids, XY_KEYS, carry, n_tokens=4)
    assert buf[:len(block)].tobytes() == (b"x y_x y x y x y x y" if carry else b"x_y x_y x y x y x y") and joins == 2 - carry
    # no accepted phrase at all
    empty = np.zeros(0, np.int64)
    got, carry_out, joins = check_join(hip, block, start, length, ids, empty, carry)
    assert (got, carry_out, joins) == (block.tobytes(), 0, 0)


@pytest.mark.parametrize("threshold", cases.THRESHOLDS)
def test_join_with_every_separator_kind(hip, corpus, threshold):
    data, (block, start, length, ids, unigram, tokens), (keys, counts) = corpus
    phrase_keys = pref.select(keys, counts, unigram, tokens, 5, threshold)[0]
    for carry in (0, 1):
        got, _, joins = check_join(hip, block, start, length, ids, phrase_keys, carry, ord("+") if carry else ord("_"))
        assert joins >= 100
    got, _, _ = check_join(hip, block, start, length, ids, phrase_keys, 0)
    assert got == pref.word2phrase_plain(data, 5, threshold)[0]


# ---- end to end
def run(tmp_path, data, name, backend, **kw):
    from trainer import phrases
    src, out = tmp_path / "corpus.txt", tmp_path / name
    src.write_bytes(data)
    phrases.process_corpus(src, out, backend=backend, **kw)
    return [Path(str(out) + ext).read_bytes() for ext in ("", ".phrases.txt", ".phrases.json")]


@pytest.mark.parametrize("block_bytes", [257, 4096, 1 << 30])
def test_process_corpus_writes_the_reference_s_files(hip, tmp_path, corpus, block_bytes):
    data = corpus[0]
    want = run(tmp_path, data, "want", Backends(), min_count=5, threshold=10.0)
    assert want[0] == pref.word2phrase_plain(data, 5, 10.0)[0] and want[0] != data
    got = run(tmp_path, data, "got", hip, min_count=5, threshold=10.0, block_bytes=block_bytes)
    assert got == want
    assert run(tmp_path, data, "again", hip, min_count=5, threshold=10.0, block_bytes=block_bytes) == got


def test_two_passes_equal_the_reference(hip, tmp_path, corpus):
    data = corpus[0]
    want = run(tmp_path, data, "want", Backends(), min_count=5, threshold=10.0, passes=2)
    got = run(tmp_path, data, "got", hip, min_count=5, threshold=10.0, passes=2, block_bytes=4096)
    assert got == want and b"san_francisco_bay_area" in got[0]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_cases_end_to_end(hip, tmp_path, name):
    data, options, want = EDGES[name]
    got = run(tmp_path, data, "got", hip, block_bytes=64, **options)
    assert got == run(tmp_path, data, "want", Backends(), **options)
    assert want is None or got[0] == want
