"""The text entry points of libglove_prep_hip.so on the GPU (include/glove_text_hip.h): the tokenizer, a block's
vocabulary, the merge of two vocabularies and the token ids against the restatement of tests/text_ref.py, exactly;
trainer.cooccur with tokenizer="device" against tokenizer="python", files byte for byte; three calls captured into one graph."""
from pathlib import Path

import numpy as np
import pytest
import torch

import text_ref as tref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
I32_PATTERN, I64_PATTERN = -0x01234567, -0x0123456789ABCDEF
GOLDEN = Path(__file__).resolve().parent / "golden"
WHITESPACE_BYTES = [c.encode() for c in tref.WHITESPACE]


@pytest.fixture(scope="module")
def prep(hip):
    from trainer import hip_api
    return hip_api.load_prep_library()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a).copy())
    return (t if dtype is None else t.to(dtype)).to(DEV)


def dev_bytes(data: bytes, shift=0):
    """The bytes on the device, `shift` bytes behind a 256-B aligned address."""
    buf = torch.zeros(len(data) + shift + 16, dtype=torch.uint8, device=DEV)
    buf[shift:shift + len(data)] = dev(np.frombuffer(data, np.uint8))
    return buf[shift:shift + len(data)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def filled(n, dtype, pattern):
    return torch.full((n + GUARD,), pattern, dtype=dtype, device=DEV)


def bits(t):
    return t.cpu().numpy().view(np.uint64)


# ---- the tokenizer
def tokenize_raw(prep, data: bytes, cap, shift=0):
    block = dev_bytes(data, shift)
    start, length, hashes = filled(cap, torch.int32, I32_PATTERN), filled(cap, torch.int32, I32_PATTERN), filled(cap, torch.int64, I64_PATTERN)
    sizes = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_text_tokenize_workspace_bytes(len(data)), dtype=torch.uint8, device=DEV)
    rc = prep.glove_text_tokenize_u8(block.data_ptr() if len(data) else None, len(data), start.data_ptr(), length.data_ptr(),
                                     hashes.data_ptr(), sizes[0:1].data_ptr(), sizes[2:3].data_ptr(), cap, ws.data_ptr(), ws.numel(),
                                     stream())
    torch.cuda.synchronize()
    return rc, sizes.cpu().numpy(), start.cpu().numpy(), length.cpu().numpy(), hashes.cpu().numpy()


def check_tokenize(prep, data: bytes, want=None, shift=0):
    """Against the reference at four capacities: room for every token the bytes could hold, the true size, one less, none."""
    w_start, w_len, w_hash, _ = want or tref.tokenize(data)
    true = len(w_start)
    for cap in sorted({(len(data) + 1) // 2, true, max(true - 1, 0), 0}):
        rc, sizes, start, length, hashes = tokenize_raw(prep, data, cap, shift)
        m = min(true, cap)
        assert rc == 0 and sizes[0] == true and sizes[2] == (w_len[:m] > tref.MAX_TOKEN).sum(), (rc, sizes, true, cap)
        assert sizes[1] == -7 and sizes[3] == -7                                # one int64 each
        np.testing.assert_array_equal(start[:m], w_start[:m])
        np.testing.assert_array_equal(length[:m], w_len[:m])
        np.testing.assert_array_equal(hashes[:m].view(np.uint64), w_hash[:m])
        assert (start[m:] == I32_PATTERN).all() and (length[m:] == I32_PATTERN).all() and (hashes[m:] == I64_PATTERN).all(), cap
    return true


SEQUENCES = [s for s in WHITESPACE_BYTES if len(s) > 1]
NEAR_MISSES = [b"\xc2\x84", b"\xe2\x80\x8b", b"\xe2\x80", b"\xe2\x81\x9e", b"\xe3\x80\x81", b"\xe1\x9a\x81", b"\xc2"]
EDGE_BLOCKS = {
    "empty": b"", "all_separators": b" \n\t \x1c\xc2\xa0\xe3\x80\x80 ", "one_token_no_trailing_separator": b"token",
    "token_at_byte_0": b"a bc  def\n", "one_byte": b"a", "one_separator": b" ",
    "each_separator_between_letters": b"".join(b"a" + s + b"b" + s + s for s in WHITESPACE_BYTES),
    "near_misses_stay_token_bytes": b" ".join(b"a" + s + b"b" for s in NEAR_MISSES) + b" x\xe2\x80 y\xc2",
    "sequence_at_start_and_end": b"\xe2\x80\xa8word\xe1\x9a\x80", "two_byte_sequence_at_start_and_end": b"\xc2\x85w\xc2\xa0",
    "mixed_runs": b" \t\xe2\x80\x83\n\xc2\xa0a\x1f\x1e\xe2\x81\x9f\xe3\x80\x80bc \xc2\x85\x0b\x0cd",
    "high_bytes_inside_words": "na\u00efve caf\u00e9 \u65e5\u672c\u8a9e \U0001d11ex \u00e9".encode() + b" \xff\xfe\x80 \xe2\xe2\x80\xe2\x80\x80z",
    "lone_c2_last": b"ab \xc2", "truncated_sequence_last": b"ab \xe2\x80",
}


@pytest.mark.parametrize("name", sorted(EDGE_BLOCKS))
def test_tokenizer_edge_blocks(prep, name):
    data = EDGE_BLOCKS[name]
    true = check_tokenize(prep, data)
    if name == "each_separator_between_letters":
        assert len(WHITESPACE_BYTES) == 29 and len(SEQUENCES) == 19 and true == 2 * 29
    if name == "near_misses_stay_token_bytes":
        assert true == len(NEAR_MISSES) + 2
    if name in ("empty", "all_separators", "one_separator"):
        assert true == 0


def random_words(rng, n_bytes, seps=(b" ", b" ", b" ", b"\n", b"  ", b"\xc2\xa0", b"\xe2\x80\x83", b"\t")):
    """Random words of 1-12 bytes (letters and a few multibyte ones) with separators between them, cut to n_bytes."""
    letters = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz"] + ["\u00e9".encode(), "\u65e5".encode(), b"\xe2\x80\x8b"]
    out, size = [], 0
    while size < n_bytes:
        word = b"".join(letters[i] for i in rng.integers(0, len(letters), rng.integers(1, 13)))
        out += [word, seps[rng.integers(len(seps))]]
        size += len(out[-2]) + len(out[-1])
    return b"".join(out)[:n_bytes]


@pytest.mark.parametrize("label", ["T-1", "T", "T+1", "3T+5", "40T+17"])
def test_tokenizer_block_lengths_around_the_tile(prep, label):
    from trainer.hip_api import TEXT_TILE_BYTES as T
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5, "40T+17": 40 * T + 17}[label]
    data = random_words(np.random.default_rng(n), n)
    want = tref.tokenize(data)
    assert check_tokenize(prep, data, want) > n // 12
    if label in ("T+1", "3T+5"):
        check_tokenize(prep, data, want, shift=1)            # a block that starts off a 16-B boundary: the byte-wise loads
        check_tokenize(prep, data, want, shift=8)


def test_tokens_and_separators_that_straddle_a_tile_boundary(prep):
    from trainer.hip_api import TEXT_TILE_BYTES as T
    pad = random_words(np.random.default_rng(1), 3 * T)
    for off in range(-3, 4):                                  # a token that starts / ends `off` bytes from the boundary
        for word in (b"straddle", b"xy", b"q"):
            at = T + off
            data = pad[:at - 1] + b" " + word + b" " + pad[:T]
            check_tokenize(prep, data)
            at = 2 * T + off - len(word)
            data = pad[:at - 1] + b" " + word + b" " + pad[:40]
            check_tokenize(prep, data)
    for seq in (b"\xe2\x80\x83", b"\xe3\x80\x80", b"\xc2\xa0", b"\xe2\x80\x8b", b"\xc2\x84"):      # the last two: near misses
        for split in range(len(seq) + 1):                     # `split` bytes of it in the first tile
            data = b"a" * (T - split) + seq + b"b" * 5
            assert data[T - split:T - split + len(seq)] == seq
            check_tokenize(prep, data)
            data = b"a " * ((T - split) // 2) + b"c" * ((T - split) % 2) + seq + seq + b" b"
            check_tokenize(prep, data)


@pytest.mark.parametrize("length, n_long", [(65535, 0), (65536, 1)])
def test_the_longest_hashed_token_and_one_byte_more(prep, length, n_long):
    word = bytes(np.random.default_rng(length).integers(97, 123, length).astype(np.uint8))
    data = b"ab " + word + b" cd " + word[:100] + b"\n"
    want = tref.tokenize(data)
    assert want[3] == n_long and want[1].tolist() == [2, length, 2, 100]
    assert int(want[2][1]) == tref.fnv1a(word[:65535])                                      # the hash covers 65535 bytes
    check_tokenize(prep, data, want)
    rc, sizes, start, length_, hashes = tokenize_raw(prep, data, 10)
    assert rc == 0 and sizes[0] == 4 and sizes[2] == n_long and length_[1] == length   # the true length is written


def test_binding_tokenizes(hip):
    data = EDGE_BLOCKS["mixed_runs"] + b" " + EDGE_BLOCKS["high_bytes_inside_words"]
    start, length, hashes, n_long = hip.text_tokenize(dev_bytes(data))
    want = tref.tokenize(data)
    assert n_long == 0 and start.dtype == torch.int32 and hashes.dtype == torch.int64
    np.testing.assert_array_equal(start.cpu().numpy(), want[0])
    np.testing.assert_array_equal(length.cpu().numpy(), want[1])
    np.testing.assert_array_equal(bits(hashes), want[2])
    empty = hip.text_tokenize(torch.zeros(0, dtype=torch.uint8, device=DEV))
    assert len(empty[0]) == len(empty[1]) == len(empty[2]) == 0 and empty[3] == 0


# ---- a block's vocabulary
def vocab_raw(prep, start, length, hashes, n_tokens, base_offset, cap_out):
    cap_tokens = len(hashes)
    d_start, d_len, d_hash = dev(start, torch.int32), dev(length, torch.int32), dev(np.asarray(hashes, np.uint64).view(np.int64))
    keys, counts, where = (filled(cap_out, torch.int64, I64_PATTERN) for _ in range(3))
    sizes = dev(np.asarray([n_tokens, -7, -7], np.int64))
    ws = torch.empty(prep.glove_text_block_vocab_workspace_bytes(cap_tokens), dtype=torch.uint8, device=DEV)
    rc = prep.glove_text_block_vocab(d_hash.data_ptr() if cap_tokens else None, d_start.data_ptr() if cap_tokens else None,
                                     d_len.data_ptr() if cap_tokens else None, sizes[0:1].data_ptr(), cap_tokens, base_offset,
                                     keys.data_ptr(), counts.data_ptr(), where.data_ptr(), sizes[1:2].data_ptr(), cap_out,
                                     ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, sizes.cpu().numpy(), keys.cpu().numpy(), counts.cpu().numpy(), where.cpu().numpy()


def check_vocab(prep, start, length, hashes, base_offset=0, n_tokens=None):
    n = len(hashes) if n_tokens is None else n_tokens
    want = tref.block_vocab(hashes[:n], start[:n], length[:n], base_offset)
    true = len(want[0])
    for cap in sorted({max(n, 1), true, max(true - 1, 0), 0}):
        rc, sizes, keys, counts, where = vocab_raw(prep, start, length, hashes, n, base_offset, cap)
        m = min(true, cap)
        assert rc == 0 and sizes[1] == true and (sizes[2] == -7 or len(hashes) == 0), (rc, sizes, true, cap)
        np.testing.assert_array_equal(keys[:m].view(np.uint64), want[0][:m])
        np.testing.assert_array_equal(counts[:m], want[1][:m])
        np.testing.assert_array_equal(where[:m], want[2][:m])
        assert (keys[m:] == I64_PATTERN).all() and (counts[m:] == I64_PATTERN).all() and (where[m:] == I64_PATTERN).all(), cap
    return want


def zipf_text(rng, n, types, seps=(b" ",)):
    """n words drawn from `types` by a Zipf law (so: ties among the rare ones), separated."""
    p = 1.0 / np.arange(1, types + 1)
    picks = rng.choice(types, size=n, p=p / p.sum())
    return b"".join(b"w%d" % i + seps[rng.integers(len(seps))] for i in picks)


VOCAB_CASES = {
    "one_token": lambda rng: b"word", "all_equal": lambda rng: b"same " * 3000,
    "all_distinct": lambda rng: b"".join(b"t%d " % i for i in range(3000)), "zipf_with_ties": lambda rng: zipf_text(rng, 6000, 900),
    "no_token": lambda rng: b"   ", "n_2047": lambda rng: zipf_text(rng, 2047, 300), "n_2048": lambda rng: zipf_text(rng, 2048, 300),
    "n_2049": lambda rng: zipf_text(rng, 2049, 300),
}


@pytest.mark.parametrize("name", sorted(VOCAB_CASES))
def test_block_vocab_equals_the_reference(prep, name):
    data = VOCAB_CASES[name](np.random.default_rng(len(name)))
    start, length, hashes, _ = tref.tokenize(data)
    if name.startswith("n_"):
        assert len(hashes) == int(name[2:])
    want = check_vocab(prep, start, length, hashes)
    if name == "all_equal":
        assert want[1].tolist() == [3000] and want[2].tolist() == [4]
    if name == "zipf_with_ties":
        assert len(np.unique(want[1])) < len(want[1]) // 4
        # first occurrences, not any occurrence: `where` names the earliest start of its word
        first = {}
        for s, n in zip(start.tolist(), length.tolist()):
            first.setdefault(data[s:s + n], s)
        assert sorted(w >> 16 for w in want[2].tolist()) == sorted(first.values())


def test_block_vocab_offsets_long_tokens_and_device_side_counts(prep):
    data = zipf_text(np.random.default_rng(2), 3000, 200) + b"x" * 70000 + b" end"
    start, length, hashes, n_long = tref.tokenize(data)
    assert n_long == 1
    base = (1 << 40) + 12345
    want = check_vocab(prep, start, length, hashes, base)
    assert (want[2] >> 16).min() == base and (want[2] & 0xFFFF).max() == 65535       # the long token's length is clamped
    check_vocab(prep, start, length, hashes, (1 << 46) - 1)
    start[2000:], length[2000:], hashes[2000:] = -5, -9, hashes[0]                   # poison behind the count
    check_vocab(prep, start, length, hashes, base, n_tokens=2000)
    check_vocab(prep, start, length, hashes, base, n_tokens=1)
    check_vocab(prep, start, length, hashes, base, n_tokens=0)


def test_binding_makes_a_block_vocabulary(hip):
    data = zipf_text(np.random.default_rng(4), 5000, 400, seps=(b" ", b"\n", b"\xe2\x80\x83"))
    block = dev_bytes(data)
    start, length, hashes, _ = hip.text_tokenize(block)
    keys, counts, where = hip.text_block_vocab(hashes, start, length, 1 << 33)
    want = tref.block_vocab(*[tref.tokenize(data)[i] for i in (2, 0, 1)], 1 << 33)
    for g, w in zip((bits(keys), counts.cpu().numpy(), where.cpu().numpy()), want):
        np.testing.assert_array_equal(g, w)
    none = hip.text_block_vocab(hashes[:0], start[:0], length[:0], 0)
    assert all(len(a) == 0 for a in none)


# ---- the merge
def merge_raw(prep, A, B, cap_out, n_a=None, n_b=None):
    a, b = [dev(x, torch.int64) for x in A], [dev(x, torch.int64) for x in B]
    sizes = dev(np.asarray([len(A[0]) if n_a is None else n_a, len(B[0]) if n_b is None else n_b, -7, -7], np.int64))
    out = [filled(cap_out, torch.int64, I64_PATTERN) for _ in range(3)]
    ws = torch.empty(prep.glove_text_vocab_merge_workspace_bytes(len(A[0]), len(B[0])), dtype=torch.uint8, device=DEV)
    rc = prep.glove_text_vocab_merge(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), sizes[0:1].data_ptr(), len(A[0]),
                                     b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), sizes[1:2].data_ptr(), len(B[0]),
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), sizes[2:3].data_ptr(), cap_out,
                                     ws.data_ptr(), ws.numel(), stream())
    torch.cuda.synchronize()
    return rc, sizes.cpu().numpy(), [o.cpu().numpy() for o in out]


def check_merge(prep, A, B, n_a=None, n_b=None):
    na, nb = (len(A[0]) if n_a is None else n_a), (len(B[0]) if n_b is None else n_b)
    want = tref.vocab_merge(*[tref.as_keys(x[:na]) if i == 0 else x[:na] for i, x in enumerate(A)],
                            *[tref.as_keys(x[:nb]) if i == 0 else x[:nb] for i, x in enumerate(B)])
    true = len(want[0])
    for cap in sorted({na + nb, true, max(true - 1, 0), 0}):
        rc, sizes, out = merge_raw(prep, A, B, cap, n_a, n_b)
        assert rc == 0 and sizes[2] == true and sizes[3] == -7, (rc, sizes, true, cap)
        m = min(true, cap)
        np.testing.assert_array_equal(out[0][:m].view(np.uint64), want[0][:m])
        np.testing.assert_array_equal(out[1][:m], want[1][:m])
        np.testing.assert_array_equal(out[2][:m], want[2][:m])
        assert all((o[m:] == I64_PATTERN).all() for o in out), cap
    return want


def with_where(case, seed):
    """A merge case of the co-occurrence merge's test as two (keys, counts, where) tables; keys spread over all 64 bits."""
    A, cA, B, cB = case
    rng = np.random.default_rng(seed)
    spread = lambda k: (np.asarray(k, np.int64).view(np.uint64) * np.uint64((1 << 46) - 3) + np.uint64(7)).view(np.int64) \
        if len(k) and np.asarray(k).max() < (1 << 18) else np.asarray(k, np.int64)        # monotone: no wrap below 2^18
    where = lambda n: (rng.integers(0, 1 << 46, n) << 16 | rng.integers(1, 65536, n)).astype(np.int64)
    return (spread(A), cA, where(len(A))), (spread(B), cB, where(len(B)))


MERGE_NAMES = ["merged_length_%s" % s for s in ("0", "1", "T-1", "T", "T+1", "3T+5", "40T+17")] + [
    "one_entry_in_a", "a_empty", "b_empty", "both_empty", "a_equals_b", "a_below_b", "b_below_a", "interleaved_no_twins",
    "keys_above_2_62_counts_near_2_40", "uneven_sizes"]


@pytest.mark.parametrize("name", MERGE_NAMES)
def test_vocab_merge_equals_the_reference_exactly(prep, name):
    from test_gpu_cooc_stream import merge_case
    A, B = with_where(merge_case(name), len(name))
    if len(A[0]) > 1:
        assert (np.diff(tref.as_keys(A[0]).astype(object)) > 0).all()
    want = check_merge(prep, A, B)
    check_merge(prep, B, A)                                        # commutative: the same table
    if name == "a_equals_b":                                       # twins take the smaller `where`, from whichever side holds it
        assert (A[2] < B[2]).any() and (B[2] < A[2]).any()
        np.testing.assert_array_equal(want[2], np.minimum(A[2], B[2]))
    if name == "merged_length_40T+17":
        assert int(tref.as_keys(A[0]).max()) > 1 << 63                 # the order is the unsigned one


def test_vocab_merge_honours_the_device_side_counts_and_refuses_aliases(prep):
    from trainer.hip_api import COOC_MERGE_TILE as T
    rng = np.random.default_rng(5)
    table = lambda n: (np.sort(rng.choice(8 * T, n, replace=False)).astype(np.int64), rng.integers(1, 9, n).astype(np.int64),
                       rng.integers(0, 1 << 60, n).astype(np.int64))
    A, B = table(2 * T + 9), table(T + 3)
    n_a, n_b = T + 1, T - 2
    for t, n in ((A, n_a), (B, n_b)):                                # poison behind the counts
        t[0][n:], t[1][n:], t[2][n:] = 3, 1 << 50, -1
    check_merge(prep, A, B, n_a, n_b)
    check_merge(prep, A, B, 0, n_b)
    k = torch.zeros(300, dtype=torch.int64, device=DEV)
    o = torch.zeros(600, dtype=torch.int64, device=DEV)
    n = torch.zeros(3, dtype=torch.int64, device=DEV)
    ws = torch.empty(prep.glove_text_vocab_merge_workspace_bytes(100, 50), dtype=torch.uint8, device=DEV)
    p = lambda t, i: t[i:].data_ptr()
    call = lambda ko, co, wo: prep.glove_text_vocab_merge(p(k, 0), p(k, 100), p(k, 200), p(n, 0), 100, p(k, 0), p(k, 100), p(k, 200),
                                                          p(n, 1), 50, ko, co, wo, p(n, 2), 100, ws.data_ptr(), ws.numel(), stream())
    assert call(p(k, 0), p(o, 100), p(o, 200)) == -1 and call(p(o, 0), p(k, 100), p(o, 200)) == -1
    assert call(p(o, 0), p(o, 100), p(k, 250)) == -1 and call(p(o, 0), p(o, 50), p(o, 200)) == -1
    assert call(p(o, 0), p(o, 100), p(o, 200)) == 0
    torch.cuda.synchronize()


# ---- token ids
def ids_raw(prep, data, tokens, kept, n_tokens=None):
    start, length, hashes = tokens
    cap = len(hashes)
    block = dev_bytes(data)
    d = [dev(start, torch.int32), dev(length, torch.int32), dev(np.asarray(hashes, np.uint64).view(np.int64))]
    kk, ki, ko, kb = kept
    n_kept = len(kk)
    dk = [dev(np.asarray(kk, np.uint64).view(np.int64)), dev(ki, torch.int32), dev(ko, torch.int64), dev(np.frombuffer(bytes(kb) + b"\0", np.uint8))]
    ids = filled(cap, torch.int32, I32_PATTERN)
    sizes = dev(np.asarray([cap if n_tokens is None else n_tokens, -7, -7], np.int64))
    ptr = lambda t, n: t.data_ptr() if n else None
    rc = prep.glove_text_token_ids_i32(ptr(block, len(data)), len(data), ptr(d[0], cap), ptr(d[1], cap), ptr(d[2], cap),
                                       sizes[0:1].data_ptr(), cap, ptr(dk[0], n_kept), ptr(dk[1], n_kept), dk[2].data_ptr(),
                                       ptr(dk[3], n_kept), n_kept, ids.data_ptr(), sizes[1:2].data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, sizes.cpu().numpy(), ids.cpu().numpy()


def kept_from_words(words, ids=None):
    from trainer import cooccur
    lookup = {w: (i + 1 if ids is None else ids[i]) for i, w in enumerate(words)}
    keys, kid, off, data = cooccur.kept_table(lookup)
    return keys.view(np.uint64), kid, off, data


def check_ids(prep, data, kept, n_tokens=None):
    start, length, hashes, _ = tref.tokenize(data)
    n = len(hashes) if n_tokens is None else n_tokens
    want, mismatch = tref.token_ids(data, start[:n], length[:n], hashes[:n], *kept)
    rc, sizes, ids = ids_raw(prep, data, (start, length, hashes), kept, n_tokens)
    assert rc == 0 and sizes[1] == mismatch and sizes[0] == n, (rc, sizes, mismatch)
    np.testing.assert_array_equal(ids[:n], want)
    assert (ids[n:] == I32_PATTERN).all()
    return want, mismatch


@pytest.mark.parametrize("n_kept", [0, 1, 1000])
def test_token_ids_equal_the_reference(prep, n_kept):
    rng = np.random.default_rng(n_kept)
    data = zipf_text(rng, 5000, 1500, seps=(b" ", b"\n", b"\xc2\xa0")) + "\u65e5\u672c \u00e9 w0".encode()
    words = ["w%d" % i for i in rng.permutation(3000)[:n_kept]]            # half of them never occur
    if n_kept == 1:
        words = ["w0"]
    want, mismatch = check_ids(prep, data, kept_from_words(words))
    assert mismatch == 0 and (want != 0).any() == (n_kept > 0) and (want == 0).any()
    check_ids(prep, data, kept_from_words(words), n_tokens=100)
    check_ids(prep, b"", kept_from_words(words))


def test_token_ids_every_token_kept_and_no_token_kept(prep):
    data = zipf_text(np.random.default_rng(8), 4000, 300) + "\u65e5\u672c caf\u00e9".encode()
    present = sorted(set(data.decode().split()))
    want, mismatch = check_ids(prep, data, kept_from_words(present, ids=list(range(7, 7 + len(present)))))
    assert mismatch == 0 and (want >= 7).all()
    want, mismatch = check_ids(prep, data, kept_from_words(["absent%d" % i for i in range(500)]))
    assert mismatch == 0 and (want == 0).all()


def test_token_ids_count_hash_collisions(prep):
    data = b"alpha beta alpha gamma beta alpha delta"
    # `alpha`'s hash with bytes that differ in the last byte; `beta`'s with bytes that differ in length only
    kept = kept_from_words(["alpha", "beta", "gamma"])
    keys, kid, off, kb = kept
    words = {int(tref.fnv1a(w)): w for w in (b"alpha", b"beta", b"gamma")}
    fake = {b"alpha": b"alphb", b"beta": b"bet", b"gamma": b"gamma"}
    spelled = [fake[words[int(k)]] for k in keys]
    off = np.concatenate([[0], np.cumsum([len(w) for w in spelled])]).astype(np.int64)
    want, mismatch = check_ids(prep, data, (keys, kid, off, np.frombuffer(b"".join(spelled), np.uint8)))
    assert mismatch == 5 and (want != 0).sum() == 1                   # three alphas and two betas; gamma keeps its id
    want, mismatch = check_ids(prep, data, kept)
    assert mismatch == 0 and (want != 0).sum() == 6


def test_binding_numbers_tokens(hip):
    from trainer import cooccur
    data = zipf_text(np.random.default_rng(9), 3000, 200, seps=(b" ", b"\xe3\x80\x80"))
    lookup = {"w%d" % i: i + 1 for i in range(0, 200, 2)}
    block = dev_bytes(data)
    start, length, hashes, _ = hip.text_tokenize(block)
    ids, mismatch = hip.text_token_ids(block, start, length, hashes, cooccur.kept_table(lookup, hip))
    assert mismatch == 0 and ids.dtype == torch.int32
    np.testing.assert_array_equal(ids.cpu().numpy(), [lookup.get(t, 0) for t in data.decode().split()])


# ---- the two passes end to end
def write_files(hip, corpus, dest, tokenizer, **kw):
    from trainer import cooccur
    cooccur.main(str(corpus), dest / tokenizer, backend=hip, tokenizer=tokenizer, **kw)
    return [(dest / tokenizer / f).read_bytes() for f in ("vocab.csv", "vocab.txt", "interaction.csv")]


def test_device_tokenizer_writes_identical_files_on_the_golden_corpus(hip, tmp_path):
    kw = dict(vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000, count_minimum=10, seed=3, block_bytes=4096)
    want, got = write_files(hip, GOLDEN / "text8_corpus.txt", tmp_path, "python", **kw), write_files(hip, GOLDEN / "text8_corpus.txt", tmp_path, "device", **kw)
    assert got == want and got[1] == (GOLDEN / "text8_cov90_ctx5_vocab.txt").read_bytes() and len(got[2]) > 10000


def test_device_tokenizer_writes_identical_files_on_a_synthetic_corpus(hip, tmp_path):
    rng = np.random.default_rng(12)
    seps = (b" ",) * 12 + (b"\n", b"\t", b"  ", b"\xc2\xa0", b"\xe2\x80\x83", b"\xe3\x80\x80", b"\x1f")
    corpus = tmp_path / "corpus.txt"
    corpus.write_bytes(zipf_text(rng, 200_000, 20_000, seps) + "<UNK> \u65e5\u672c na\u200bme <UNK>".encode())
    kw = dict(vocab_size=5000, coverage=0.95, context_size=5, chunk_tokens=1000, count_minimum=5, seed=1, block_bytes=4096)
    want, got = write_files(hip, corpus, tmp_path, "python", **kw), write_files(hip, corpus, tmp_path, "device", **kw)
    assert got == want and len(got[1].split(b"\n")) > 1000 and len(got[2]) > 100000


# ---- the calls promise to be capturable
def test_tokenize_vocab_merge_captured_into_one_graph(hip, prep):
    from trainer.hip_api import TEXT_TILE_BYTES as T
    n_bytes = 5 * T + 123
    rng = np.random.default_rng(21)
    texts = [zipf_text(rng, n_bytes, 500, seps=(b" ", b"\n", b"\xe2\x80\x83"))[:n_bytes] for _ in range(3)]
    state = [t.clone() for t in hip.text_block_vocab(*[hip.text_tokenize(dev_bytes(texts[0]))[i] for i in (2, 0, 1)], 0)]
    n_state = dev(np.asarray([len(state[0])], np.int64))
    cap_tokens = (n_bytes + 1) // 2
    cap = len(state[0]) + cap_tokens
    new = lambda n, dtype=torch.int64: torch.zeros(n, dtype=dtype, device=DEV)
    block = new(n_bytes, torch.uint8)
    start, length, hashes, counters = new(cap_tokens, torch.int32), new(cap_tokens, torch.int32), new(cap_tokens), new(4)
    block_vocab, n_block = [new(cap_tokens) for _ in range(3)], new(2)
    merged, n_merged = [new(cap) for _ in range(3)], new(2)
    bytes_ = lambda n: torch.empty(n, dtype=torch.uint8, device=DEV)
    ws = (bytes_(prep.glove_text_tokenize_workspace_bytes(n_bytes)), bytes_(prep.glove_text_block_vocab_workspace_bytes(cap_tokens)),
          bytes_(prep.glove_text_vocab_merge_workspace_bytes(len(state[0]), cap_tokens)))
    base = 1 << 20

    def enqueue():
        hip.text_tokenize_enqueue(block, start, length, hashes, counters[0:2], counters[2:4], ws[0])
        hip.text_block_vocab_enqueue(hashes, start, length, counters[0:1], base, *block_vocab, n_block, ws[1])
        hip.text_vocab_merge_enqueue(state, n_state, block_vocab, n_block[0:1], merged, n_merged, ws[2])

    def result():
        torch.cuda.synchronize()
        m = int(n_merged[0].item())
        return [t[:m].cpu().numpy().copy() for t in merged]

    def expected(text):
        s, n, h, _ = tref.tokenize(text)
        want = tref.vocab_merge(bits(state[0]), state[1].cpu().numpy(), state[2].cpu().numpy(), *tref.block_vocab(h, s, n, base))
        return [tref.as_bits(want[0]), want[1], want[2]]

    def load(text):
        block.copy_(dev(np.frombuffer(text, np.uint8)))

    load(texts[1])
    enqueue()                                       # eager, and the warm-up of every kernel
    eager = result()
    for g, w in zip(eager, expected(texts[1])):
        np.testing.assert_array_equal(g, w)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue()
    for text in (texts[2], texts[1]):               # two replays, on a fresh block each
        load(text)
        n_merged.fill_(-1)
        graph.replay()
        for g, w in zip(result(), expected(text)):
            np.testing.assert_array_equal(g, w)
    for g, w in zip(result(), eager):
        np.testing.assert_array_equal(g, w)
