"""Tokenizing and numbering a corpus, without a GPU: the restatement of tests/text_ref.py against str.split(),
text8.vocabulary_from_arrays against vocabulary_from_counts, trainer.cooccur with tokenizer="device" on the NumPy backends
against tokenizer="python" (files byte for byte), and the surface and host-side argument checks of the text entry points
of libglove_prep_hip.so (include/glove_text_hip.h)."""
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import cooc_stream_ref
import text_ref
from test_analogy import BADARG, FAKE, declared_functions

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
HEADER = REPO / "include" / "glove_text_hip.h"
FILES = ("vocab.csv", "vocab.txt", "interaction.csv")


class NumpyBackends(cooc_stream_ref.NumpyBackend, text_ref.NumpyTextBackend):
    """Everything trainer.cooccur asks of a backend, on numpy arrays."""


# ---- the token definition
def test_the_separators_are_the_29_whitespace_characters():
    assert len(text_ref.WHITESPACE) == 29
    one_byte = [c for c in text_ref.WHITESPACE if len(c.encode()) == 1]
    assert sorted(c.encode() for c in one_byte) == [bytes([b]) for b in (9, 10, 11, 12, 13, 0x1c, 0x1d, 0x1e, 0x1f, 0x20)]
    assert len(text_ref.WHITESPACE) - len(one_byte) == 19
    for c in text_ref.WHITESPACE:
        assert text_ref.SEPARATOR.fullmatch(c.encode()), hex(ord(c))
        assert text_ref.token_spans(b"a" + c.encode() + b"b") == [(0, 1), (1 + len(c.encode()), 1)]
    for c in text_ref.LOOK_ALIKES:
        assert not c.isspace() and text_ref.token_spans(("a" + c + "b").encode()) == [(0, 2 + len(c.encode()))]


def test_reference_tokens_equal_str_split_on_random_strings():
    rng = np.random.default_rng(0)
    alphabet = text_ref.WHITESPACE + text_ref.LOOK_ALIKES + list("abcxyz_09") + ["\u00e9", "\u00df", "\u1681", "\u2010", "\u3001", "\U0001d11e", " "]
    weights = np.asarray([1.0] * len(text_ref.WHITESPACE) + [1.0] * len(text_ref.LOOK_ALIKES) + [6.0] * 9 + [2.0] * 6 + [12.0])
    weights /= weights.sum()
    for _ in range(3000):
        text = "".join(rng.choice(alphabet, size=rng.integers(0, 40), p=weights))
        data = text.encode()
        got = [data[s:s + n].decode() for s, n in text_ref.token_spans(data)]
        assert got == text.split(), repr(text)


def test_hash_is_fnv1a_of_the_first_65535_bytes():
    assert text_ref.fnv1a(b"") == 0xcbf29ce484222325 and text_ref.fnv1a(b"a") == 0xaf63dc4c8601ec8c
    assert text_ref.fnv1a(b"foobar") == 0x85944171f73967e8                      # the published FNV-1a test vectors
    long = b"x" * 65535
    assert text_ref.fnv1a(long + b"y") == text_ref.fnv1a(long) != text_ref.fnv1a(long[:-1])
    from trainer import cooccur
    for w in (b"", b"a", b"foobar", long + b"yz", "\u00e9\u3001".encode()):
        assert cooccur.token_hash(w) == text_ref.fnv1a(w)


# ---- the vocabulary from arrays
def zipf_corpus(rng, n, types, ties=True):
    p = 1.0 / np.arange(1, types + 1)
    ids = rng.choice(types, size=n, p=p / p.sum())
    if ties:                                           # many types with the same small count
        ids = np.concatenate([ids, np.repeat(np.arange(types, types + 30), 2), np.arange(types + 30, types + 60)])
        rng.shuffle(ids)
    return ["w%d" % i for i in ids]


@pytest.mark.parametrize("vocab_size, coverage", [(None, .9), (5, .9), (3, 1.0), (None, .5)])
def test_vocabulary_from_arrays_equals_vocabulary_from_counts(vocab_size, coverage):
    from trainer import text8
    rng = np.random.default_rng(7)
    for trial in range(50):
        tokens = zipf_corpus(rng, int(rng.integers(1, 400)), int(rng.integers(1, 40)), ties=trial % 2 == 0)
        want = text8.vocabulary_from_counts(Counter(tokens), vocab_size, coverage)
        first = {}
        for pos, t in enumerate(tokens):
            first.setdefault(t, pos)
        types = sorted(first, key=lambda t: text_ref.fnv1a(t.encode()))          # hash order, as the device returns them
        counts = np.asarray([Counter(tokens)[t] for t in types], np.int64)
        where = np.asarray([(first[t] * 7 + 3) << 16 | len(t) for t in types], np.int64)
        by_where = dict(zip(where.tolist(), types))
        asked = []
        got = text8.vocabulary_from_arrays(counts, where, lambda w: asked.append(w) or by_where[w], vocab_size, coverage)
        assert got[0] == want[0]
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        assert got[1].dtype == want[1].dtype and len(asked) == len(want[0]) - 1        # kept tokens only


# ---- the block reader
@pytest.mark.parametrize("block_bytes", [1, 7, 1000])
def test_byte_blocks_reassemble_the_file_and_end_on_separators(tmp_path, block_bytes):
    from trainer.cooccur import iter_byte_blocks, iter_token_blocks
    path = tmp_path / "corpus.txt"
    texts = ["  \n alpha  beta\n\ngamma\t delta   a_token_that_is_far_longer_than_any_small_block  x y\n z   \n ", "", "   \n",
             "one", "no_trailing space", "\u00e9 \u00fc \u00df", "a b c d", (GOLDEN / "text8_corpus.txt").read_text()[:5000]]
    for text in texts:
        path.write_text(text)
        data = path.read_bytes()
        blocks = list(iter_byte_blocks(path, block_bytes))
        assert b"".join(b for _, b in blocks) == data and all(b for _, b in blocks)
        assert [o for o, _ in blocks] == list(np.cumsum([0] + [len(b) for _, b in blocks[:-1]]))[:len(blocks)]
        assert all(b[-1:] in (b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c") for _, b in blocks[:-1])
        tokens = [t for _, b in blocks for t in b.decode().split()]
        assert tokens == text.split() == [t for b in iter_token_blocks(path, block_bytes) for t in b]


# ---- the two passes end to end on the NumPy backends
def unicode_corpus(tmp_path):
    """A small corpus with every separator, look-alikes inside words, count ties and a literal <UNK>."""
    rng = np.random.default_rng(3)
    words = ["w%d" % i for i in range(40)] + ["\u00e9", "na\u200bme", "\u00df\u0084", "<UNK>", "\u65e5\u672c", "x" * 70]
    p = 1.0 / np.arange(1, len(words) + 1)
    picks = list(rng.choice(len(words), size=3000, p=p / p.sum())) + list(range(len(words))) * 2       # ties in the tail
    seps = text_ref.WHITESPACE + [" "] * 60 + ["\n", " \t ", "\u2003\u3000"]
    text = "".join(words[i] + seps[rng.integers(len(seps))] for i in picks)
    path = tmp_path / "unicode_corpus.txt"
    path.write_bytes(text.encode())
    assert len(set(Counter(text.split()).values())) < len(words) - 5
    return path


def both_tokenizers(corpus, tmp_path, **kw):
    from trainer import cooccur
    for tokenizer in ("python", "device"):
        cooccur.main(str(corpus), tmp_path / tokenizer, backend=NumpyBackends(), tokenizer=tokenizer, **kw)
    for f in FILES:
        assert (tmp_path / "python" / f).read_bytes() == (tmp_path / "device" / f).read_bytes(), f
    return (tmp_path / "device" / "vocab.txt").read_text().split("\n")


def test_device_tokenizer_writes_the_files_of_the_python_tokenizer_on_the_golden_corpus(tmp_path):
    vocab = both_tokenizers(GOLDEN / "text8_corpus.txt", tmp_path, vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000,
                            count_minimum=10, seed=3, block_bytes=1000)
    assert vocab == (GOLDEN / "text8_cov90_ctx5_vocab.txt").read_text().split("\n")


@pytest.mark.parametrize("vocab_size, coverage, block_bytes", [(None, 0.9, 100), (12, 0.95, 1000), (None, 1.0, 1 << 20)])
def test_device_tokenizer_on_unicode_separators_and_count_ties(tmp_path, vocab_size, coverage, block_bytes):
    vocab = both_tokenizers(unicode_corpus(tmp_path), tmp_path, vocab_size=vocab_size, coverage=coverage, context_size=3,
                            chunk_tokens=500, count_minimum=2, seed=1, block_bytes=block_bytes)
    assert "<UNK>" in vocab and len(vocab) > 5
    if coverage == 1.0:
        assert "na\u200bme" in vocab and vocab.count("<UNK>") == 2


def test_an_unknown_tokenizer_is_refused():
    from trainer import cooccur
    with pytest.raises(ValueError, match="tokenizer"):
        cooccur.process_corpus(str(GOLDEN / "text8_corpus.txt"), backend=NumpyBackends(), tokenizer="gpu")


class Reporting(NumpyBackends):
    """A backend that reports tokens too long / hash mismatches."""
    def __init__(self, n_long=0, n_mismatch=0):
        self.long, self.mismatch = n_long, n_mismatch

    def text_tokenize(self, block):
        start, length, hashes, _ = super().text_tokenize(block)
        n_long, self.long = self.long, 0                 # once: the accumulator sums what the blocks report
        return start, length, hashes, n_long

    def text_token_ids(self, block, start, length, hashes, kept):
        return super().text_token_ids(block, start, length, hashes, kept)[0], self.mismatch


def test_long_tokens_and_mismatches_are_value_errors(tmp_path):
    from trainer import cooccur
    corpus = str(GOLDEN / "text8_corpus.txt")
    with pytest.raises(ValueError, match=r"(?s)\b3 tokens.*--tokenizer python"):
        cooccur.process_corpus(corpus, None, 0.9, 5, 1000, backend=Reporting(n_long=3), block_bytes=1 << 20, tokenizer="device")
    with pytest.raises(ValueError, match=r"(?s)\b4 tokens.*--tokenizer python"):
        cooccur.process_corpus(corpus, None, 0.9, 5, 1000, backend=Reporting(n_mismatch=4), block_bytes=1 << 20, tokenizer="device")
    cooccur.process_corpus(corpus, None, 0.9, 5, 1000, backend=Reporting(3, 4), block_bytes=1 << 20)      # python: not asked
    # a real one: a token of 65536 bytes
    path = tmp_path / "long.txt"
    path.write_bytes(b"a b " + b"x" * 65536 + b" a b a\n")
    with pytest.raises(ValueError, match="1 tokens are longer than 65535"):
        cooccur.process_corpus(str(path), None, 1.0, 2, 100, backend=NumpyBackends(), tokenizer="device")
    # ... and a real mismatch: a kept table whose entry has the hash of a present word and other bytes
    data = np.frombuffer(b"aa bb aa cc", np.uint8)
    start, length, hashes, _ = text_ref.tokenize(data)
    kept = (np.asarray([text_ref.fnv1a(b"aa")], np.uint64), np.asarray([5], np.int32), np.asarray([0, 2], np.int64),
            np.frombuffer(b"ab", np.uint8))
    ids, n = text_ref.token_ids(data, start, length, hashes, *kept)
    assert ids.tolist() == [0, 0, 0, 0] and n == 2


# ---- the library: surface, workspace queries, argument checks (all before any launch)
@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.PREP_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_prep_library()


def test_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADER)
    assert set(names) == set(hip_api.TEXT_EXPORTED_SYMBOLS) and len(names) == len(hip_api.TEXT_EXPORTED_SYMBOLS) == 8
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_text_abi_version() == hip_api.GLOVE_TEXT_ABI_VERSION == 1
    text = HEADER.read_text()
    assert "GLOVE_TEXT_ABI_VERSION 1" in text
    assert "GLOVE_TEXT_TILE_BYTES %d" % hip_api.TEXT_TILE_BYTES in text and "GLOVE_TEXT_MAX_TOKEN %d" % hip_api.TEXT_MAX_TOKEN in text
    assert hip_api.TEXT_MAX_TOKEN == text_ref.MAX_TOKEN == 65535
    others = set(hip_api.EXPORTED_SYMBOLS) | set(hip_api.EVAL_EXPORTED_SYMBOLS) | set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS) \
        | set(hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS) | set(hip_api.PREP_EXPORTED_SYMBOLS)
    assert not set(names) & others
    train = hip_api.load_library()
    assert not any(hasattr(train, n) for n in names)            # the prep library's, not the training library's
    assert len(hip_api.PREP_EXPORTED_SYMBOLS) == 7 and hip_api.GLOVE_ABI_VERSION == 15 and len(hip_api.EXPORTED_SYMBOLS) == 42


def test_workspace_queries_are_pure_host_functions(lib):
    from trainer import hip_api
    tok, voc, mrg = (lib.glove_text_tokenize_workspace_bytes, lib.glove_text_block_vocab_workspace_bytes,
                     lib.glove_text_vocab_merge_workspace_bytes)
    assert tok(-1) == 0 and tok(2 ** 31) == 0 and tok(0) > 0 and tok(2 ** 31 - 1) > 0
    assert voc(-1) == 0 and voc(2 ** 31) == 0 and voc(0) > 0 and voc(2 ** 31 - 1) > 0
    for bad in ((-1, 5), (5, -1), ((1 << 40) + 1, 0), (1 << 39, (1 << 39) + 1)):
        assert mrg(*bad) == 0, bad
    assert mrg(0, 0) > 0 and mrg(1 << 39, 1 << 39) > 0
    T = hip_api.TEXT_TILE_BYTES
    sizes = [0, 1, T - 1, T, T + 1, 10 ** 6, 10 ** 8, 2 ** 31 - 1]
    for a, b in zip(sizes, sizes[1:]):
        assert tok(a) <= tok(b) and voc(a) <= voc(b) and mrg(a, 7) <= mrg(b, 7) and mrg(7, a) <= mrg(7, b)
    assert tok(10 ** 6) < tok(10 ** 8) and voc(10 ** 6) < voc(10 ** 7) and mrg(10 ** 6, 0) < mrg(10 ** 7, 0)
    # the layouts, as the header states them
    up = lambda x: (x + 255) // 256 * 256
    tiles = (10 ** 6 + T - 1) // T
    assert tok(10 ** 6) == 2 * up(8 * tiles) + up((64 << 10) + 8 * tiles)
    assert mrg(10 ** 6, 12345) == lib.glove_cooc_merge_workspace_bytes(10 ** 6, 12345)
    n = 10 ** 6
    assert voc(n) == 2 * up(8 * n) + 4 * up(4 * n) + 256 + up((16 << 20) + 24 * n)


def test_argument_errors_are_reported_before_any_launch(lib):
    big = 1 << 30
    call = lambda fn, order, defaults, kw: fn(*[{**defaults, **kw}[k] for k in order])
    A, B, O = 0x100000, 0x400000, 0x700000                           # distinct "device" ranges, 3 MiB apart
    # tokenize
    order = ("bytes", "n_bytes", "start", "len", "hash", "n_tokens", "n_long", "cap", "ws", "ws_bytes", "stream")
    base = dict(bytes=FAKE, n_bytes=100, start=A, len=A + 0x10000, hash=A + 0x20000, n_tokens=O, n_long=O + 64, cap=50, ws=FAKE,
                ws_bytes=big, stream=None)
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap=-1), dict(bytes=None), dict(start=None), dict(len=None),
               dict(hash=None), dict(n_tokens=None), dict(n_long=None), dict(ws=None), dict(n_long=O), dict(n_long=O + 4)):
        assert call(lib.glove_text_tokenize_u8, order, base, kw) == BADARG, kw
    assert call(lib.glove_text_tokenize_u8, order, base, dict(ws_bytes=16)) == -2                # GLOVE_E_WORKSPACE
    # block vocabulary
    order = ("hash", "start", "len", "n_tokens", "cap_tokens", "base_offset", "keys", "counts", "where", "n_out", "cap_out", "ws",
             "ws_bytes", "stream")
    base = dict(hash=A, start=A + 0x10000, len=A + 0x20000, n_tokens=A + 0x30000, cap_tokens=100, base_offset=0, keys=O,
                counts=O + 0x10000, where=O + 0x20000, n_out=O + 0x30000, cap_out=100, ws=FAKE, ws_bytes=big, stream=None)
    for kw in (dict(cap_tokens=-1), dict(cap_tokens=2 ** 31), dict(cap_out=-1), dict(base_offset=-1), dict(base_offset=1 << 46),
               dict(hash=None), dict(start=None), dict(len=None), dict(n_tokens=None), dict(keys=None), dict(counts=None),
               dict(where=None), dict(n_out=None), dict(ws=None)):
        assert call(lib.glove_text_block_vocab, order, base, kw) == BADARG, kw
    assert call(lib.glove_text_block_vocab, order, base, dict(ws_bytes=16)) == -2
    # merge
    order = ("ka", "ca", "wa", "na", "cap_a", "kb", "cb", "wb", "nb", "cap_b", "ko", "co", "wo", "no", "cap_out", "ws", "ws_bytes",
             "stream")
    base = dict(ka=A, ca=A + 0x40000, wa=A + 0x80000, na=A + 0xC0000, cap_a=100, kb=B, cb=B + 0x40000, wb=B + 0x80000,
                nb=B + 0xC0000, cap_b=50, ko=O, co=O + 0x40000, wo=O + 0x80000, no=O + 0xC0000, cap_out=150, ws=FAKE, ws_bytes=big,
                stream=None)
    for kw in (dict(cap_a=-1), dict(cap_b=-1), dict(cap_out=-1), dict(na=None), dict(nb=None), dict(no=None), dict(ws=None),
               dict(ka=None), dict(cb=None), dict(wa=None), dict(wb=None), dict(ko=None), dict(wo=None), dict(cap_a=(1 << 40) + 1),
               dict(ko=A), dict(ko=A + 99 * 8), dict(ko=A - 149 * 8), dict(co=A), dict(wo=A + 0x80000), dict(wo=B + 0x80000 + 8),
               dict(ko=B + 8), dict(co=B + 0x40000), dict(ko=A + 0x40000), dict(no=A + 0xC0000), dict(no=B + 0xC0000),
               dict(no=A + 8), dict(co=O), dict(wo=O), dict(wo=O + 0x40000 + 8), dict(no=O + 8), dict(no=O + 0x80000)):
        assert call(lib.glove_text_vocab_merge, order, base, kw) == BADARG, kw
    assert call(lib.glove_text_vocab_merge, order, base, dict(ws_bytes=16)) == -2
    # token ids
    order = ("bytes", "n_bytes", "start", "len", "hash", "n_tokens", "cap_tokens", "kept_keys", "kept_id", "kept_off", "kept_bytes",
             "n_kept", "ids", "n_mismatch", "stream")
    base = dict(bytes=FAKE, n_bytes=100, start=A, len=A + 0x10000, hash=A + 0x20000, n_tokens=A + 0x30000, cap_tokens=50,
                kept_keys=B, kept_id=B + 0x10000, kept_off=B + 0x20000, kept_bytes=B + 0x30000, n_kept=10, ids=O,
                n_mismatch=O + 0x10000, stream=None)
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap_tokens=-1), dict(n_kept=-1), dict(bytes=None), dict(start=None),
               dict(len=None), dict(hash=None), dict(n_tokens=None), dict(kept_keys=None), dict(kept_id=None), dict(kept_off=None),
               dict(kept_bytes=None), dict(ids=None), dict(n_mismatch=None)):
        assert call(lib.glove_text_token_ids_i32, order, base, kw) == BADARG, kw
