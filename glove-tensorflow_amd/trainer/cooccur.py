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

Vocabulary counting and id mapping are plain Python (`Counter`, `dict`) and pandas writes the CSV.
"""
from __future__ import annotations

import logging
import sys
from argparse import ArgumentParser
from collections import Counter

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


def iter_chunks(id_blocks, chunk_tokens: int, context: int):
    """Cuts a stream of int32 id arrays into (ids[s : e + halo], e - s): chunks of `chunk_tokens` own positions, each
    followed by its halo of min(context, tokens left) — what `CoocAccumulator.add` takes."""
    if chunk_tokens < 1:
        raise ValueError("chunk_tokens must be positive, got %d" % chunk_tokens)
    buf = np.zeros(0, np.int32)
    for ids in id_blocks:
        buf = np.concatenate([buf, np.asarray(ids, np.int32)])
        while len(buf) >= chunk_tokens + context:       # the halo is complete
            yield buf[:chunk_tokens + context], chunk_tokens
            buf = buf[chunk_tokens:]
    while len(buf):
        own = min(chunk_tokens, len(buf))
        yield buf[:own + min(context, len(buf) - own)], own
        buf = buf[own:]


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
        keys, counts = self.backend.cooc_chunk_keys(tokens_with_halo, int(n_own), self.V, self.context)
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

    def finalize(self, min_count: int = 0):
        """(row, col, count, value) in (row, col) order, pairs with count >= min_count only."""
        if self.keys is None:
            raise ValueError("no chunk was added")
        return self.backend.cooc_finalize(self.keys, self.counts, self.V, self.context, int(min_count))


def count_vocabulary(path, block_bytes: int = BLOCK_BYTES) -> Counter:
    """Pass one: the running token counts of the corpus (first occurrences in corpus order, as Counter(text.split()))."""
    counter = Counter()
    for tokens in iter_token_blocks(path, block_bytes):
        counter.update(tokens)
    return counter


def process_corpus(path, vocab_size=VOCAB_SIZE, coverage=COVERAGE, context_size=CONTEXT_SIZE, chunk_tokens=CHUNK_TOKENS,
                   count_minimum=10, seed=0, backend=None, block_bytes: int = BLOCK_BYTES):
    """The data `trainer.text8.save_data` writes, from a corpus file of any length."""
    from trainer import text8
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    vocab = text8.vocabulary_from_counts(count_vocabulary(path, block_bytes), vocab_size, coverage)
    logger.info("vocab created, size: %s.", len(vocab[0]))
    lookup = {tok: i for i, tok in enumerate(vocab[0])}
    acc = CoocAccumulator(len(vocab[0]), context_size, backend)
    id_blocks = (np.fromiter((lookup.get(t, 0) for t in tokens), dtype=np.int32, count=len(tokens))
                 for tokens in iter_token_blocks(path, block_bytes))
    for piece, n_own in iter_chunks(id_blocks, chunk_tokens, context_size):
        acc.add(piece, n_own)
        logger.info("chunk %d: %d keys in the state.", acc.chunks, len(acc))
    if acc.keys is None:
        acc.add(np.zeros(0, np.int32), 0)       # an empty corpus
    arrays = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in acc.finalize(count_minimum)]
    logger.info("after the count filter: %d pairs.", len(arrays[0]))
    table = text8.interaction_columns(*arrays, vocab, seed)
    return {"vocabulary": vocab, "interaction": text8.create_glove_table(table, count_minimum)}


def main(corpus, dest, vocab_size=VOCAB_SIZE, coverage=COVERAGE, context_size=CONTEXT_SIZE, chunk_tokens=CHUNK_TOKENS,
         count_minimum=10, seed=0, backend=None, **kwargs):
    from trainer import text8
    data = process_corpus(corpus, vocab_size, coverage, context_size, chunk_tokens, count_minimum, seed, backend=backend)
    return text8.save_data(data, dest)


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
    args = parser.parse_args()
    logger.info("call: %s.", " ".join(sys.argv))
    try:
        main(**args.__dict__)
    except KeyboardInterrupt:
        pass
