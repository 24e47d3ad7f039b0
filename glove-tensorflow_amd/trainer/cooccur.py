"""`python -m trainer.cooccur` — data prep for a corpus `trainer.text8` cannot hold: corpus -> vocab.txt + interaction.csv.

`trainer.text8` reads the corpus whole and hands it to `glove_cooccurrence_i32` in one call: about 52 B of device
workspace per key slot, 2 x window x tokens slots, and no more than 2^32 of them.  Here the corpus is read in blocks, twice
(pass one counts the vocabulary, pass two maps tokens to ids), and counted chunk by chunk: a chunk of `--chunk-tokens`
positions with a halo of `--context-size` tokens gives its sorted (row, col, distance) keys, and `CoocAccumulator` folds
them into one sorted table of integer counts on the device with the merge kernel of csrc/glove_cooc_stream.hip
(include/glove_cooc_stream_hip.h).  The state holds integers only, so the table does not depend on where the corpus was
cut: it is bit for bit the one-shot call's.

The files are those of `trainer.text8` (`vocab.csv`, `vocab.txt`, the nine-column `interaction.csv`), with one
difference: the count filter (`--count-minimum`) runs on the device, inside `finalize`, and the seeded row permutation is
drawn over the FILTERED rows, where `trainer.text8` permutes all rows and filters afterwards.  The same rows are written,
in another order.  (`trainer.text8 --chunk-tokens` counts through the accumulator too and keeps its own order: its files
are identical to its one-shot run's.)

Vocabulary counting and id mapping are plain Python (`Counter`, `dict`) by default.  `--tokenizer device` does both on
the device (csrc/glove_text.hip, include/glove_text_hip.h) and writes the same files byte for byte: the file's raw bytes go
up block by block; pass one tokenizes a block, makes its vocabulary (distinct 64-bit token hashes with counts and first
occurrences) and merges it into the running one (`VocabAccumulator`); the host chooses the kept words from the counts
alone and reads their strings back from the file; pass two tokenizes again, looks every token's hash up in the kept
table, compares the bytes, and the ids go to `CoocAccumulator` without touching the host (`process_corpus`).  pandas
writes the CSV.

Preprocessing options (Levy, Goldberg & Dagan 2015: `sub`, `del`, `dyn`; include/glove_cooc_options_hip.h): `--subsample T`
and `--delete-unknown` remove tokens from the id stream before the window is laid (`filter_blocks`: a token's fate is a
hash of its position in the whole stream against its word's threshold, so it does not depend on the blocks or chunks),
`--window-weighting` chooses how the state's per-distance counts make a pair's `value`.  At their defaults nothing runs
that did not run before and the files are the same bytes; otherwise `prep.json` says how the files were made.
"""
from __future__ import annotations

import json
import logging
import sys
from argparse import ArgumentParser
from collections import Counter
from pathlib import Path

import numpy as np

from trainer.config import CONTEXT_SIZE, COVERAGE, DATA_DIR, VOCAB_SIZE

logger = logging.getLogger(__name__)
CHUNK_TOKENS = 4 << 20
BLOCK_BYTES = 16 << 20


def iter_token_blocks(path, block_bytes: int = BLOCK_BYTES):
    """The whitespace-separated tokens of a file as lists, one per block of `block_bytes` bytes read; a token cut by a
    block boundary is carried into the next block.  Concatenated, the lists are `text.split()`.  The file is never read
    whole."""
    carry = b""
    with open(path, "rb") as f:
        while True:
            block = f.read(block_bytes)
            if not block:
                break
            block = carry + block
            if block[-1:].isspace():
                carry = b""
            else:                                   # the last token may go on in the next block
                cut = max(block.rfind(c) for c in (b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c"))
                carry, block = block[cut + 1:], block[:cut + 1]
            tokens = block.decode().split()
            if tokens:
                yield tokens
    tokens = carry.decode().split()             # (the split again: str.split knows separators beyond the ASCII ones above)
    if tokens:
        yield tokens


def iter_byte_blocks(path, block_bytes: int = BLOCK_BYTES):
    """The file as (offset, bytes) blocks of about `block_bytes` bytes, cut where `iter_token_blocks` cuts: behind the last
    of the six ASCII separators, the rest carried into the next block.  So no token straddles two blocks, and no
    multi-byte separator does (their bytes are all >= 0x80).  Concatenated, the blocks are the file; `offset` is the file
    offset of a block's first byte.  The file is never read whole."""
    carry, offset = b"", 0
    with open(path, "rb") as f:
        while True:
            block = f.read(block_bytes)
            if not block:
                break
            block = carry + block
            if block[-1:].isspace():
                carry = b""
            else:
                cut = max(block.rfind(c) for c in (b" ", b"\n", b"\t", b"\r", b"\x0b", b"\x0c"))
                carry, block = block[cut + 1:], block[:cut + 1]
            if block:
                yield offset, block
                offset += len(block)
    if carry:
        yield offset, carry


def iter_chunks(id_blocks, chunk_tokens: int, context: int):
    """Cuts a stream of int32 id arrays into (ids[s : e + halo], e - s): chunks of `chunk_tokens` own positions, each
    followed by its halo of min(context, tokens left) — what `CoocAccumulator.add` takes.  Blocks that are device tensors
    (the device tokenizer's) are cut the same way and stay where they are."""
    if chunk_tokens < 1:
        raise ValueError("chunk_tokens must be positive, got %d" % chunk_tokens)
    buf = np.zeros(0, np.int32)
    for ids in id_blocks:
        if hasattr(ids, "new_empty"):
            import torch
            buf = torch.cat([buf if hasattr(buf, "new_empty") else ids.new_empty(0), ids])
        else:
            buf = np.concatenate([buf, np.asarray(ids, np.int32)])
        while len(buf) >= chunk_tokens + context:       # the halo is complete
            yield buf[:chunk_tokens + context], chunk_tokens
            buf = buf[chunk_tokens:]
    while len(buf):
        own = min(chunk_tokens, len(buf))
        yield buf[:own + min(context, len(buf) - own)], own
        buf = buf[own:]


KEEP_ALWAYS = 0xFFFFFFFF
WINDOW_WEIGHTINGS = ("harmonic", "uniform", "dynamic")


def stream_counts(vocab) -> np.ndarray:
    """How often every id occurs in the id stream, from the vocabulary (tokens, counts, ...): a word's own count, and for
    id 0 everything out of vocabulary as well — the tokens no entry of the lookup table matches are numbered 0, whichever
    word sits there ("<UNK>" itself wherever it is the most frequent entry)."""
    tokens, counts = vocab[0], np.asarray(vocab[1], np.int64).copy()
    unk = tokens.index("<UNK>")
    if unk != 0:
        counts[0] += counts[unk]
        counts[unk] = 0
    return counts


def subsample_thresholds(counts, subsample: float = 0.0, delete_unknown: bool = False) -> np.ndarray:
    """The uint32 [V] table `filter_blocks` takes (the keep rule of include/glove_cooc_options_hip.h), made once on the
    host in float64 from the ids' stream counts: a token of id w is kept with probability q(w) = min(1, sqrt(T / f_w)),
    f_w = counts[w] / sum(counts) (word2vec's -sample, hyperwords' `sub`); the entry is 0xFFFFFFFF where q >= 1 (always
    kept), otherwise floor(q 2^32).  T = 0 keeps everything.  delete_unknown: thresholds[0] = 0, id 0 always goes."""
    counts = np.asarray(counts, np.int64)
    subsample = float(subsample)
    if not (np.isfinite(subsample) and 0.0 <= subsample < 1.0):
        raise ValueError("subsample must be finite and in [0, 1), got %r" % (subsample,))
    thresholds = np.full(len(counts), KEEP_ALWAYS, np.uint32)
    total = int(counts.sum())
    if subsample > 0.0 and total > 0:
        seen = counts > 0
        q = np.ones(len(counts), np.float64)
        q[seen] = np.sqrt(np.float64(subsample) / (counts[seen].astype(np.float64) / np.float64(total)))
        drop = q < 1.0
        thresholds[drop] = np.minimum(np.floor(q[drop] * 4294967296.0), np.float64(KEEP_ALWAYS)).astype(np.uint32)
    if delete_unknown and len(thresholds):
        thresholds[0] = 0
    return thresholds


def filter_blocks(id_blocks, thresholds, seed, backend, totals=None):
    """Sits between the id blocks and `iter_chunks`: every block's survivors under the keep rule of
    include/glove_cooc_options_hip.h (`backend.token_filter(ids, pos0, thresholds, seed)`; GloveHip is the product
    backend), removed BEFORE the window is laid — distances shrink across removed tokens.  A token's fate depends on its id
    and its position in the whole stream (the running `pos0` kept here), never on where the blocks were cut.  Host arrays
    go to the backend's device where it has one; device tensors stay where they are.  `totals`, a dict, receives the
    tokens "read" and "kept"."""
    thresholds = np.ascontiguousarray(thresholds, np.uint32)
    if hasattr(backend, "device"):
        import torch
        thresholds = torch.from_numpy(thresholds.view(np.int32).copy()).to(backend.device)
    pos = kept = 0
    for ids in id_blocks:
        if isinstance(ids, np.ndarray) and hasattr(backend, "device"):
            import torch
            ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(backend.device)
        out = backend.token_filter(ids, pos, thresholds, int(seed))
        pos += len(ids)
        kept += len(out)
        if totals is not None:
            totals["read"], totals["kept"] = pos, kept
        if len(out):
            yield out
    if totals is not None:
        totals["read"], totals["kept"] = pos, kept


def _resized(like, n):
    """An uninitialised 1-d array of n elements of `like`'s kind (a torch tensor on its device, or numpy)."""
    return like.new_empty(n) if hasattr(like, "new_empty") else np.empty(n, like.dtype)


class CoocAccumulator:
    """The co-occurrence table of a corpus that arrives in chunks.  The state is one ascending table of
    ((row V + col) context + distance - 1) keys with int64 counts; `add` counts a chunk and merges it in; `finalize` turns
    the state into (row, col, count, value).  Two state buffers swap roles (a merge reads one and writes the other) and
    grow geometrically.

    `backend` has three operations (GloveHip is the product one; the tests bring a NumPy one):
        cooc_chunk_keys(tokens, n_own, V, context) -> (keys, counts)
        cooc_merge(keys_a, counts_a, keys_b, counts_b, keys_out, counts_out) -> (keys, counts)    views of the outputs
        cooc_finalize(keys, counts, V, context, min_count) -> (row, col, count, value)
            (and `weighting=` where another window weighting than the harmonic one is asked for)
    A backend with a `device` gets numpy tokens moved there."""

    def __init__(self, V: int, context: int, backend):
        self.V, self.context, self.backend = int(V), int(context), backend
        self.keys = self.counts = None          # the state: views of the front buffer
        self._front = self._back = None         # (keys, counts) buffers
        self.chunks = 0

    def __len__(self) -> int:
        return 0 if self.keys is None else len(self.keys)

    def add(self, tokens_with_halo, n_own: int):
        """tokens_with_halo [n_own + halo] int32: this chunk's own positions, then min(context, tokens left) more."""
        if isinstance(tokens_with_halo, np.ndarray) and hasattr(self.backend, "device"):
            import torch
            tokens_with_halo = torch.from_numpy(np.ascontiguousarray(tokens_with_halo, np.int32)).to(self.backend.device)
        self.merge_in(*self.backend.cooc_chunk_keys(tokens_with_halo, int(n_own), self.V, self.context))

    def merge_in(self, keys, counts):
        """Folds one ascending (keys, counts) table into the state (trainer.phrases brings a block's bigram table)."""
        self.chunks += 1
        m = len(keys)
        if self.keys is None:                   # the first chunk is the state (copied: `keys` may be the head of a big buffer)
            self._front = (_resized(keys, max(m, 1)), _resized(counts, max(m, 1)))
            self._front[0][:m] = keys
            self._front[1][:m] = counts
            self.keys, self.counts = self._front[0][:m], self._front[1][:m]
            return
        if m == 0:
            return
        need = len(self.keys) + m
        if self._back is None or len(self._back[0]) < need:
            cap = max(need, 2 * len(self._front[0]))
            self._back = (_resized(keys, cap), _resized(counts, cap))
        self.keys, self.counts = self.backend.cooc_merge(self.keys, self.counts, keys, counts, *self._back)
        self._front, self._back = self._back, self._front

    def finalize(self, min_count: int = 0, weighting: str = "harmonic"):
        """(row, col, count, value) in (row, col) order, pairs with count >= min_count only.  The state keeps the
        distances, so the window's weighting is chosen here: "harmonic" (value = sum count / distance), "uniform"
        (value = count) or "dynamic" (value = sum count (context - distance + 1) / context, the expected weight under
        word2vec's uniformly drawn window size)."""
        if self.keys is None:
            raise ValueError("no chunk was added")
        if weighting not in WINDOW_WEIGHTINGS:
            raise ValueError("weighting must be one of %s, got %r" % (", ".join(WINDOW_WEIGHTINGS), weighting))
        if weighting == "harmonic":
            return self.backend.cooc_finalize(self.keys, self.counts, self.V, self.context, int(min_count))
        return self.backend.cooc_finalize(self.keys, self.counts, self.V, self.context, int(min_count), weighting=weighting)


class VocabAccumulator:
    """The vocabulary of a corpus that arrives in blocks of bytes, kept by the backend (on the device for GloveHip).  The
    state is one table of distinct token hashes, ascending, with int64 counts and `where` words (first occurrence in the
    file << 16 | token length); `add` tokenizes a block, makes its table and merges it in.  Two state buffers swap roles and
    grow geometrically, as CoocAccumulator's do.

    `backend` has the operations (GloveHip is the product one; the tests bring a NumPy one):
        text_tokenize(block) -> (start, length, hashes, n_long)
        text_block_vocab(hashes, start, length, base_offset) -> (keys, counts, where)
        text_vocab_merge(keys_a, counts_a, where_a, keys_b, counts_b, where_b, keys_out, counts_out, where_out)
            -> (keys, counts, where)    views of the outputs
    A backend with a `device` gets the bytes moved there."""

    def __init__(self, backend):
        self.backend = backend
        self.state = None                       # (keys, counts, where): views of the front buffers
        self._front = self._back = None
        self.blocks = self.tokens = self.n_long = 0

    def __len__(self) -> int:
        return 0 if self.state is None else len(self.state[0])

    def add(self, block: bytes, offset: int):
        """block: raw bytes that end behind a separator (or with the file); offset: the file offset of its first byte."""
        start, length, hashes, n_long = self.backend.text_tokenize(_block_array(block, self.backend))
        self.blocks += 1
        self.tokens += len(hashes)
        self.n_long += int(n_long)
        new = self.backend.text_block_vocab(hashes, start, length, int(offset))
        m = len(new[0])
        if self.state is None:                  # the first block is the state (copied: views of a bigger buffer)
            self._front = tuple(_resized(a, max(m, 1)) for a in new)
            for buf, a in zip(self._front, new):
                buf[:m] = a
            self.state = tuple(buf[:m] for buf in self._front)
            return
        if m == 0:
            return
        need = len(self.state[0]) + m
        if self._back is None or len(self._back[0]) < need:
            cap = max(need, 2 * len(self._front[0]))
            self._back = tuple(_resized(a, cap) for a in new)
        self.state = tuple(self.backend.text_vocab_merge(*self.state, *new, *self._back))
        self._front, self._back = self._back, self._front

    def counts_and_where(self):
        """(counts, where) of the distinct tokens as numpy int64 arrays (in hash order)."""
        if self.state is None:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        return tuple(np.asarray(a.cpu() if hasattr(a, "cpu") else a, np.int64) for a in self.state[1:])


def _block_array(block: bytes, backend):
    """A block's bytes as the uint8 array the backend takes (a device tensor where it has a `device`)."""
    arr = np.frombuffer(block, np.uint8)
    if hasattr(backend, "device"):
        import torch
        return torch.from_numpy(arr.copy()).to(backend.device)      # (the copy: torch wants a writable buffer)
    return arr


FNV_BASIS, FNV_PRIME, TEXT_MAX_TOKEN = 0xcbf29ce484222325, 0x100000001b3, 65535


def token_hash(word: bytes) -> int:
    """The device tokenizer's hash of a token (include/glove_text_hip.h): 64-bit FNV-1a over its first 65535 bytes,
    all-ones replaced by all-ones - 1."""
    h = FNV_BASIS
    for c in word[:TEXT_MAX_TOKEN]:
        h = ((h ^ c) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h - 1 if h == 0xFFFFFFFFFFFFFFFF else h


def kept_table(lookup: dict, backend=None):
    """The table pass two searches, from the token -> id dict the Python path looks tokens up in: (hashes ascending, as
    the int64 bit patterns of the uint64 values; ids int32; offsets int64 [n + 1]; the words' bytes, concatenated).  Two
    kept words with one hash are a collision the device could not tell apart: ValueError."""
    return kept_table_of_bytes([(tok.encode(), i) for tok, i in lookup.items()], backend)


def kept_table_of_bytes(words, backend=None):
    """`kept_table` from (the word's bytes, its id) pairs: what trainer.phrases keeps, whose words need not decode."""
    words = [(token_hash(word), word, i) for word, i in words]
    words.sort(key=lambda w: w[0])
    keys = np.asarray([w[0] for w in words], np.uint64)
    if len(keys) > 1 and (keys[1:] == keys[:-1]).any():
        raise ValueError("%d kept words share their 64-bit hash with another kept word: run with --tokenizer python"
                         % int(2 * (keys[1:] == keys[:-1]).sum()))
    ids = np.asarray([w[2] for w in words], np.int32)
    off = np.zeros(len(words) + 1, np.int64)
    np.cumsum(np.asarray([len(w[1]) for w in words], np.int64), out=off[1:])
    data = np.frombuffer(b"".join(w[1] for w in words), np.uint8)
    arrays = (keys.view(np.int64), ids, off, data)
    if hasattr(backend, "device"):
        import torch
        return tuple(torch.from_numpy(a.copy()).to(backend.device) for a in arrays)
    return arrays


def device_vocabulary(path, vocab_size, coverage, backend, block_bytes: int = BLOCK_BYTES):
    """Pass one of the device tokenizer: text8.vocabulary_from_counts(count_vocabulary(path)), the strings of the kept
    tokens read back from the file at the offsets the device returns."""
    from trainer import text8
    acc = VocabAccumulator(backend)
    for offset, block in iter_byte_blocks(path, block_bytes):
        acc.add(block, offset)
    if acc.n_long:
        raise ValueError("%d tokens are longer than %d bytes, beyond what the device tokenizer hashes: run with "
                         "--tokenizer python" % (acc.n_long, TEXT_MAX_TOKEN))
    counts, where = acc.counts_and_where()
    logger.info("%d tokens, %d distinct, in %d blocks.", acc.tokens, len(counts), acc.blocks)
    with open(path, "rb") as f:
        def read_token(w):
            f.seek(w >> 16)
            return f.read(w & 0xFFFF).decode()
        return text8.vocabulary_from_arrays(counts, where, read_token, vocab_size, coverage)


def device_id_blocks(path, lookup, backend, block_bytes: int = BLOCK_BYTES):
    """Pass two of the device tokenizer: the ids of every block's tokens, as the backend's arrays (device tensors for
    GloveHip: they feed CoocAccumulator.add through iter_chunks without touching the host)."""
    kept = kept_table(lookup, backend)
    for _, block in iter_byte_blocks(path, block_bytes):
        data = _block_array(block, backend)
        start, length, hashes, n_long = backend.text_tokenize(data)
        ids, n_mismatch = backend.text_token_ids(data, start, length, hashes, kept)
        if n_long:
            raise ValueError("%d tokens are longer than %d bytes: run with --tokenizer python" % (n_long, TEXT_MAX_TOKEN))
        if n_mismatch:
            raise ValueError("%d tokens share a 64-bit hash with a kept word of other bytes (a hash collision): run with "
                             "--tokenizer python" % n_mismatch)
        if len(ids):
            yield ids


def count_vocabulary(path, block_bytes: int = BLOCK_BYTES) -> Counter:
    """Pass one: the running token counts of the corpus (first occurrences in corpus order, as Counter(text.split()))."""
    counter = Counter()
    for tokens in iter_token_blocks(path, block_bytes):
        counter.update(tokens)
    return counter


def process_corpus(path, vocab_size=VOCAB_SIZE, coverage=COVERAGE, context_size=CONTEXT_SIZE, chunk_tokens=CHUNK_TOKENS,
                   count_minimum=10, seed=0, backend=None, block_bytes: int = BLOCK_BYTES, tokenizer: str = "python",
                   subsample: float = 0.0, subsample_seed: int = 0, delete_unknown: bool = False,
                   window_weighting: str = "harmonic"):
    """The data `trainer.text8.save_data` writes, from a corpus file of any length.

    subsample = T > 0 keeps a token of word w with probability min(1, sqrt(T / f_w)) and delete_unknown removes the
    out-of-vocabulary tokens (id 0), both BEFORE the window is laid (`filter_blocks`); window_weighting chooses how a
    pair's distances make its `value` (`CoocAccumulator.finalize`).  The vocabulary is the raw corpus's in every case.
    With all four at their defaults no filter runs and the data are what they were without them; otherwise the result
    also holds "prep": the options, the tokens read and the tokens kept.

    tokenizer="python" counts the vocabulary and maps tokens to ids on the host (`Counter`, `dict`); "device" does both on
    the backend (include/glove_text_hip.h) and returns the same data.  Why it is the same whenever it returns (it raises
    ValueError where the device counts a token longer than 65535 bytes or a hash mismatch, naming the count): the device
    keeps one entry per distinct 64-bit token hash, so two distinct words can share an entry only if their hashes collide.
    If the merged entry is kept, the table of pass two holds the bytes of the word that occurred first, and pass two sees
    that the other word's bytes differ: a mismatch, counted.  If it is not kept, both words are out of vocabulary in
    either path, and an entry below the cutoff moves neither the cutoff nor the ranks of the kept entries.
    Invalid UTF-8 is the one input on which the paths differ: Python raises UnicodeDecodeError at the block that holds it,
    the device path only where a kept word does not decode."""
    from trainer import text8
    if tokenizer not in ("python", "device"):
        raise ValueError("tokenizer must be 'python' or 'device', got %r" % (tokenizer,))
    if window_weighting not in WINDOW_WEIGHTINGS:
        raise ValueError("window_weighting must be one of %s, got %r" % (", ".join(WINDOW_WEIGHTINGS), window_weighting))
    subsample = float(subsample)
    if not (np.isfinite(subsample) and 0.0 <= subsample < 1.0):
        raise ValueError("subsample must be finite and in [0, 1), got %r" % (subsample,))
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    if tokenizer == "device":
        vocab = device_vocabulary(path, vocab_size, coverage, backend, block_bytes)
    else:
        vocab = text8.vocabulary_from_counts(count_vocabulary(path, block_bytes), vocab_size, coverage)
    logger.info("vocab created, size: %s.", len(vocab[0]))
    lookup = {tok: i for i, tok in enumerate(vocab[0])}
    acc = CoocAccumulator(len(vocab[0]), context_size, backend)
    if tokenizer == "device":
        id_blocks = device_id_blocks(path, lookup, backend, block_bytes)
    else:
        id_blocks = (np.fromiter((lookup.get(t, 0) for t in tokens), dtype=np.int32, count=len(tokens))
                     for tokens in iter_token_blocks(path, block_bytes))
    totals = {}
    if subsample > 0.0 or delete_unknown:
        thresholds = subsample_thresholds(stream_counts(vocab), subsample, delete_unknown)
        id_blocks = filter_blocks(id_blocks, thresholds, subsample_seed, backend, totals)
    for piece, n_own in iter_chunks(id_blocks, chunk_tokens, context_size):
        acc.add(piece, n_own)
        logger.info("chunk %d: %d keys in the state.", acc.chunks, len(acc))
    if acc.keys is None:
        acc.add(np.zeros(0, np.int32), 0)       # an empty corpus
    arrays = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in acc.finalize(count_minimum, window_weighting)]
    logger.info("after the count filter: %d pairs.", len(arrays[0]))
    table = text8.interaction_columns(*arrays, vocab, seed)
    data = {"vocabulary": vocab, "interaction": text8.create_glove_table(table, count_minimum)}
    if subsample > 0.0 or subsample_seed != 0 or delete_unknown or window_weighting != "harmonic":
        read = int(np.asarray(vocab[1], np.int64).sum())
        data["prep"] = {"subsample": subsample, "subsample_seed": int(subsample_seed), "delete_unknown": bool(delete_unknown),
                        "window_weighting": window_weighting, "tokens_read": int(totals.get("read", read)),
                        "tokens_kept": int(totals.get("kept", read))}
        logger.info("kept %d of %d tokens.", data["prep"]["tokens_kept"], data["prep"]["tokens_read"])
    return data


def main(corpus, dest, vocab_size=VOCAB_SIZE, coverage=COVERAGE, context_size=CONTEXT_SIZE, chunk_tokens=CHUNK_TOKENS,
         count_minimum=10, seed=0, backend=None, block_bytes: int = BLOCK_BYTES, tokenizer: str = "python",
         subsample: float = 0.0, subsample_seed: int = 0, delete_unknown: bool = False, window_weighting: str = "harmonic",
         **kwargs):
    """Writes vocab.csv, vocab.txt and interaction.csv to `dest`; with any of the four preprocessing options set, also
    prep.json (the options, the tokens read and kept), so the files say how they were made."""
    from trainer import text8
    data = process_corpus(corpus, vocab_size, coverage, context_size, chunk_tokens, count_minimum, seed, backend=backend,
                          block_bytes=block_bytes, tokenizer=tokenizer, subsample=subsample, subsample_seed=subsample_seed,
                          delete_unknown=delete_unknown, window_weighting=window_weighting)
    text8.save_data(data, dest)
    if "prep" in data:
        (Path(dest) / "prep.json").write_text(json.dumps(data["prep"], indent=2, sort_keys=True) + "\n")
    return data


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    parser = ArgumentParser(description="Prepare a corpus of any length (vocabulary + co-occurrence) on the GPU, chunk by chunk.")
    d = " (default: %(default)s)"
    parser.add_argument("--corpus", required=True, help="whitespace-separated text file")
    parser.add_argument("--dest", default=DATA_DIR, help="directory receiving vocab.csv, vocab.txt and interaction.csv" + d)
    parser.add_argument("--vocab-size", type=int, default=VOCAB_SIZE, help="maximum size of vocab" + d)
    parser.add_argument("--coverage", type=float, default=COVERAGE, help="token coverage to set token count cutoff" + d)
    parser.add_argument("--context-size", type=int, default=CONTEXT_SIZE, help="size of context window" + d)
    parser.add_argument("--chunk-tokens", type=int, default=CHUNK_TOKENS, help="corpus positions counted per chunk" + d)
    parser.add_argument("--count-minimum", type=int, default=10, help="pairs seen less often are dropped" + d)
    parser.add_argument("--seed", type=int, default=0, help="seed of the row shuffle" + d)
    parser.add_argument("--tokenizer", choices=("python", "device"), default="python",
                        help="where the corpus is split into tokens, counted and numbered: on the host, or on the GPU from "
                             "the file's bytes (the same files)" + d)
    parser.add_argument("--subsample", type=float, default=0.0, metavar="T",
                        help="keep a token of word w with probability min(1, sqrt(T / f_w)), f_w its share of all tokens, "
                             "before the window is laid; 0 keeps every token" + d)
    parser.add_argument("--subsample-seed", type=int, default=0, help="seed of the subsampling decisions" + d)
    parser.add_argument("--delete-unknown", action="store_true",
                        help="remove the out-of-vocabulary tokens (id 0) before the window is laid")
    parser.add_argument("--window-weighting", choices=WINDOW_WEIGHTINGS, default="harmonic",
                        help="a pair's value from its counts per distance k: sum count / k, count, or "
                             "sum count (window - k + 1) / window" + d)
    args = parser.parse_args()
    logger.info("call: %s.", " ".join(sys.argv))
    try:
        main(**args.__dict__)
    except KeyboardInterrupt:
        pass
