"""Python / NumPy restatement of include/glove_text_hip.h: the tokens of a block of bytes (a bytes regex, no decoding),
their FNV-1a hashes in Python ints, a block's vocabulary, the merge of two vocabularies and the ids of the tokens from a
table of kept words.  NumpyTextBackend wraps the four as the backend trainer.cooccur drives with tokenizer="device" (the
product backend is GloveHip); hashes travel as the int64 bit patterns of their uint64 values, as they do there."""
import re

import numpy as np

# a run of the ten separator bytes, or one of the 19 sequences (the UTF-8 of every other str.isspace() character)
SEPARATOR = re.compile(rb"[\t\n\x0b\x0c\r\x1c-\x1f ]+|\xc2[\x85\xa0]|\xe1\x9a\x80|\xe2\x80[\x80-\x8a\xa8\xa9\xaf]|\xe2\x81\x9f|\xe3\x80\x80")
MAX_TOKEN = 65535
FNV_BASIS, FNV_PRIME, MASK = 0xcbf29ce484222325, 0x100000001b3, 0xFFFFFFFFFFFFFFFF
# every character str.isspace() knows (29), and what the tests put beside them: near misses and multibyte letters
WHITESPACE = [chr(c) for c in range(0x110000) if chr(c).isspace()]
LOOK_ALIKES = ["\u200b", "\u0084", "\u2060", "\ufeff"]


def token_spans(data: bytes):
    """[(start, length)] of the maximal runs of non-separator bytes."""
    spans, at = [], 0
    for m in SEPARATOR.finditer(data):
        if m.start() > at:
            spans.append((at, m.start() - at))
        at = m.end()
    if len(data) > at:
        spans.append((at, len(data) - at))
    return spans


def fnv1a(word: bytes) -> int:
    h = FNV_BASIS
    for c in word[:MAX_TOKEN]:
        h = ((h ^ c) * FNV_PRIME) & MASK
    return h - 1 if h == MASK else h


def tokenize(data):
    """(start int32, length int32, hashes uint64, n_long) of a block (bytes or a uint8 array)."""
    data = bytes(data)
    spans = token_spans(data)
    start = np.asarray([s for s, _ in spans], np.int32)
    length = np.asarray([n for _, n in spans], np.int32)
    hashes = np.asarray([fnv1a(data[s:s + n]) for s, n in spans], np.uint64)
    return start, length, hashes, int((length > MAX_TOKEN).sum())


def block_vocab(hashes, start, length, base_offset=0):
    """(keys uint64 ascending, counts int64, where int64): where = ((base_offset + start of the first occurrence) << 16) |
    min(length, 65535)."""
    hashes = np.asarray(hashes, np.uint64)
    keys, first, counts = np.unique(hashes, return_index=True, return_counts=True)
    where = ((np.int64(base_offset) + np.asarray(start, np.int64)[first]) << 16) | np.minimum(np.asarray(length, np.int64)[first], MAX_TOKEN)
    return keys, counts.astype(np.int64), where.astype(np.int64)


def vocab_merge(keys_a, counts_a, where_a, keys_b, counts_b, where_b):
    """The ascending union; counts of shared keys summed, the smaller `where` kept."""
    keys = np.concatenate([np.asarray(keys_a, np.uint64), np.asarray(keys_b, np.uint64)])
    counts = np.concatenate([np.asarray(counts_a, np.int64), np.asarray(counts_b, np.int64)])
    where = np.concatenate([np.asarray(where_a, np.int64), np.asarray(where_b, np.int64)])
    uk, inv = np.unique(keys, return_inverse=True)
    out_c = np.zeros(len(uk), np.int64)
    np.add.at(out_c, inv, counts)
    out_w = np.full(len(uk), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(out_w, inv, where)
    return uk, out_c, out_w


def token_ids(data, start, length, hashes, kept_keys, kept_id, kept_off, kept_bytes):
    """(ids int32, n_mismatch): kept_id[j] where hashes[t] == kept_keys[j] and the token's bytes are
    kept_bytes[kept_off[j] : kept_off[j + 1]]; 0 otherwise, counted as a mismatch where the hash is kept."""
    data, kept_bytes = bytes(data), bytes(kept_bytes)
    kept_keys = np.asarray(kept_keys, np.uint64)
    ids = np.zeros(len(hashes), np.int32)
    mismatch = 0
    where = np.searchsorted(kept_keys, np.asarray(hashes, np.uint64))
    for t, j in enumerate(where):
        if j < len(kept_keys) and kept_keys[j] == hashes[t]:
            if data[start[t]:start[t] + length[t]] == kept_bytes[kept_off[j]:kept_off[j + 1]]:
                ids[t] = kept_id[j]
            else:
                mismatch += 1
    return ids, mismatch


def as_bits(keys):
    return np.asarray(keys, np.uint64).view(np.int64)


def as_keys(bits):
    return np.ascontiguousarray(bits, np.int64).view(np.uint64)


class NumpyTextBackend:
    """The text operations of a trainer.cooccur backend on numpy arrays (no `device`: bytes stay where they are).
    Combine it with cooc_stream_ref.NumpyBackend for a backend that runs the whole of trainer.cooccur."""

    def text_tokenize(self, block):
        start, length, hashes, n_long = tokenize(block)
        return start, length, as_bits(hashes), n_long

    def text_block_vocab(self, hashes, start, length, base_offset=0):
        keys, counts, where = block_vocab(as_keys(hashes), start, length, base_offset)
        return as_bits(keys), counts, where

    def text_vocab_merge(self, keys_a, counts_a, where_a, keys_b, counts_b, where_b, keys_out=None, counts_out=None,
                         where_out=None):
        keys, counts, where = vocab_merge(as_keys(keys_a), counts_a, where_a, as_keys(keys_b), counts_b, where_b)
        if keys_out is None:
            return as_bits(keys), counts, where
        m = len(keys)
        assert m <= len(keys_out) == len(counts_out) == len(where_out), "the accumulator sized its buffers for both inputs"
        assert not np.shares_memory(keys_out, keys_a) and not np.shares_memory(keys_out, keys_b)
        keys_out[:m], counts_out[:m], where_out[:m] = as_bits(keys), counts, where
        return keys_out[:m], counts_out[:m], where_out[:m]

    def text_token_ids(self, block, start, length, hashes, kept):
        kept_keys, kept_id, kept_off, kept_bytes = kept
        return token_ids(block, start, length, as_keys(hashes), as_keys(kept_keys), kept_id, kept_off, kept_bytes)
