"""`python -m trainer.phrases` — phrase detection (word2vec's word2phrase) before counting: corpus -> corpus of the same
length in which the single space inside a detected collocation is a delimiter byte, so that `trainer.cooccur` numbers
"new_york" as one word.

    python -m trainer.phrases --corpus corpus.txt --output phrased.txt [--min-count 5 --threshold 100 --passes 2]
    python -m trainer.cooccur --corpus phrased.txt --tokenizer device ...

The rule is word2phrase.c's (include/glove_phrases_hip.h states it): words seen at least `min_count` times are kept; a
pair of kept words separated by exactly one space is a bigram; a bigram seen n_ab >= min_count times with
(n_ab - min_count) / n_a / n_b * N > threshold is accepted; reading left to right, an accepted pair is joined unless the
pair before it was.  Running the tool on its own output (`--passes`) makes phrases of three and four words.

The file is read three times per pass, in blocks, never whole, and everything per token runs on the backend (GloveHip is
the product one: csrc/glove_text.hip, csrc/glove_phrases.hip):
  1. the vocabulary (`cooccur.VocabAccumulator`); the host chooses the kept words from the counts and reads their bytes back;
  2. per block: ids, the block's bigram table, merged into the running one (`cooccur.CoocAccumulator.merge_in`); at the end
     the accepted phrases are selected from it;
  3. per block: ids, the join, and the bytes are written.
Reads 2 and 3 cut the file where `cooccur.iter_byte_blocks` cuts it and put in front of every block the bytes from the
previous block's last token on (`halo_blocks`), so every adjacent pair and its separator lie in exactly one block; one int32
carries "the last pair was joined" from block to block.  The result does not depend on the block size.

Besides the corpus, OUT.phrases.txt lists the last pass's phrases (phrase, bigram count, joins, score; best score first)
and OUT.phrases.json the options and every pass's counts (and the earlier passes' phrases).
"""
from __future__ import annotations

import json
import logging
import math
import os
import sys
from argparse import ArgumentParser

import numpy as np

from trainer.cooccur import (BLOCK_BYTES, TEXT_MAX_TOKEN, CoocAccumulator, VocabAccumulator, iter_byte_blocks,
                             kept_table_of_bytes)

logger = logging.getLogger(__name__)
SEPARATOR_BYTES = frozenset(b"\t\n\x0b\x0c\r\x1c\x1d\x1e\x1f ")


def check_options(corpus, output, min_count, threshold, delimiter, passes) -> int:
    """The delimiter's byte, or ValueError for options the tool refuses (nothing is opened)."""
    if int(min_count) != min_count or min_count < 1:
        raise ValueError("min_count must be an integer >= 1, got %r" % (min_count,))
    if not (math.isfinite(threshold) and threshold > 0):
        raise ValueError("threshold must be finite and > 0, got %r" % (threshold,))
    if int(passes) != passes or passes < 1:
        raise ValueError("passes must be an integer >= 1, got %r" % (passes,))
    raw = delimiter.encode() if isinstance(delimiter, str) else bytes(delimiter)
    if len(raw) != 1 or raw[0] >= 0x80 or raw[0] in SEPARATOR_BYTES:
        raise ValueError("delimiter must be one byte below 0x80 that separates no tokens, got %r" % (delimiter,))
    written = [os.path.realpath(p) for p in pass_outputs(output, passes)]
    if os.path.realpath(corpus) in written:
        raise ValueError("the output (or a pass's intermediate file) %s is the corpus itself" % corpus)
    return raw[0]


def pass_outputs(output, passes: int) -> list:
    """The file every pass writes: OUT.pass1 ... for the earlier ones, OUT for the last."""
    return ["%s.pass%d" % (output, k) for k in range(1, passes)] + [str(output)]


def _to_backend(array, backend):
    """A writable copy of a numpy array where the backend works: a device tensor where it has a `device`."""
    array = np.array(array)
    if hasattr(backend, "device"):
        import torch
        return torch.from_numpy(array).to(backend.device)
    return array


def _to_host(array) -> np.ndarray:
    return np.asarray(array.cpu() if hasattr(array, "cpu") else array)


def halo_blocks(byte_blocks, kept, backend):
    """(data, start, length, ids, last) per (offset, bytes) block as `iter_byte_blocks` cuts them: data = the bytes from
    the previous block's last token on, then the block, on the backend, with its tokens and their ids from the `kept` table;
    last = where data's last token starts (its length without a token).  data[:last] is the block's own share of the file:
    the rest comes again in front of the next block, so a block that adds no token hands everything on."""
    halo = b""
    for _, block in byte_blocks:
        raw = halo + block
        data = _to_backend(np.frombuffer(raw, np.uint8), backend)
        start, length, hashes, n_long = backend.text_tokenize(data)
        if n_long:
            raise ValueError("%d tokens are longer than %d bytes, beyond what the device tokenizer hashes" % (n_long, TEXT_MAX_TOKEN))
        ids, n_mismatch = backend.text_token_ids(data, start, length, hashes, kept)
        if n_mismatch:
            raise ValueError("%d tokens share a 64-bit hash with a kept word of other bytes (a hash collision)" % n_mismatch)
        last = int(start[-1]) if len(start) else len(raw)
        yield data, start, length, ids, last
        halo = raw[last:]


def kept_words(path, min_count, backend, block_bytes):
    """Read one: (words, unigram, tokens, types).  words[id] = the bytes of kept word id (words[0] = b"": every other
    token), ids by count descending, ties by first occurrence; unigram[id] = its count (unigram[0]: all other tokens)."""
    acc = VocabAccumulator(backend)
    for offset, block in iter_byte_blocks(path, block_bytes):
        acc.add(block, offset)
    if acc.n_long:
        raise ValueError("%d tokens are longer than %d bytes, beyond what the device tokenizer hashes" % (acc.n_long, TEXT_MAX_TOKEN))
    counts, where = acc.counts_and_where()
    order = np.lexsort((where, -counts))
    order = order[counts[order] >= min_count]
    words = [b""]
    with open(path, "rb") as f:
        for w in where[order].tolist():
            f.seek(w >> 16)
            words.append(f.read(w & 0xFFFF))
    unigram = np.concatenate([np.asarray([acc.tokens - int(counts[order].sum())], np.int64), counts[order]])
    return words, unigram, acc.tokens, len(counts)


def accepted_phrases(byte_blocks, kept, unigram, tokens, min_count, threshold, backend):
    """Read two: (keys, counts, scores) of the accepted bigrams on the backend, keys ascending, and the number of distinct
    bigrams: every block's bigram table merged into one, then selected."""
    acc = CoocAccumulator(len(unigram), 1, backend)
    for data, start, length, ids, _ in halo_blocks(byte_blocks, kept, backend):
        acc.merge_in(*backend.phrase_bigram_keys(data, start, length, ids))
    if acc.keys is None:                        # an empty file
        return tuple(_to_backend(np.zeros(0, t), backend) for t in (np.int64, np.int64, np.float64)), 0
    return backend.phrase_select(acc.keys, acc.counts, _to_backend(unigram, backend), int(tokens), int(min_count),
                                 float(threshold)), len(acc)


def join_blocks(byte_blocks, kept, phrase_keys, delimiter: int, backend, write):
    """Read three: every block joined on the backend and handed to `write` as bytes, each byte of the file once.
    -> joined [len(phrase_keys)] on the backend: how often every phrase was joined."""
    carry = _to_backend(np.zeros(1, np.int32), backend)
    joined = _to_backend(np.zeros(len(phrase_keys), np.int64), backend)
    held = None                                 # the block before, until it is known whether it was the last
    for data, start, length, ids, last in halo_blocks(byte_blocks, kept, backend):
        if held is not None:
            write(held[0][:held[1]])
        backend.phrase_join(data, start, length, ids, phrase_keys, delimiter, carry, joined)
        held = (_to_host(data).tobytes(), last)
    if held is not None:
        write(held[0])
    return joined


def one_pass(corpus, output, min_count, threshold, delimiter: int, backend, block_bytes):
    """corpus -> output by the rule above.  -> (the pass's counts, its phrases as (phrase bytes, bigram count, joins, score)
    rows, best score first, ties by key)."""
    words, unigram, tokens, types = kept_words(corpus, min_count, backend, block_bytes)
    kept = kept_table_of_bytes([(word, i) for i, word in enumerate(words) if i], backend)
    (keys, counts, scores), bigram_types = accepted_phrases(iter_byte_blocks(corpus, block_bytes), kept, unigram, tokens,
                                                            min_count, threshold, backend)
    with open(output, "wb") as out:
        joined = join_blocks(iter_byte_blocks(corpus, block_bytes), kept, keys, delimiter, backend, out.write)
    keys, counts, scores, joined = (_to_host(a) for a in (keys, counts, scores, joined))
    rows = [(words[k >> 32] + bytes([delimiter]) + words[k & 0xFFFFFFFF], c, j, s)
            for k, c, j, s in sorted(zip(keys.tolist(), counts.tolist(), joined.tolist(), scores.tolist()),
                                     key=lambda r: (-r[3], r[0]))]
    joins = int(joined.sum())
    report = {"tokens": int(tokens), "types": int(types), "kept_types": len(words) - 1, "bigram_types": int(bigram_types),
              "phrases": len(rows), "joins": joins, "tokens_out": int(tokens) - joins}
    return report, rows


def process_corpus(corpus, output, min_count=5, threshold=100.0, delimiter="_", passes=1, block_bytes: int = BLOCK_BYTES,
                   backend=None):
    """Writes `output` (the corpus with its phrases joined, `passes` times over), `output`.phrases.txt and
    `output`.phrases.json; returns what the JSON holds.  Refuses (ValueError, before the corpus is opened): min_count < 1,
    a threshold that is not finite or <= 0, a delimiter that is not one byte below 0x80 or that is a separator byte,
    passes < 1, an output that is the corpus.  Tokens longer than 65535 bytes and hash collisions are errors, as in
    trainer.cooccur."""
    corpus, output = os.fspath(corpus), os.fspath(output)
    delim = check_options(corpus, output, min_count, threshold, delimiter, passes)
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    files = pass_outputs(output, passes)
    result = {"options": {"min_count": int(min_count), "threshold": float(threshold), "delimiter": chr(delim), "passes": int(passes)},
              "passes": []}
    source = corpus
    for k, dest in enumerate(files):
        report, rows = one_pass(source, dest, min_count, threshold, delim, backend, block_bytes)
        logger.info("pass %d: %d tokens, %d kept types, %d bigram types, %d phrases, %d joins.", k + 1, report["tokens"],
                    report["kept_types"], report["bigram_types"], report["phrases"], report["joins"])
        if dest != files[-1]:                   # the last pass's phrases are the text file
            report["table"] = [[p.decode("utf-8", "surrogateescape"), c, j, s] for p, c, j, s in rows]
        result["passes"].append(report)
        source = dest
    for dest in files[:-1]:
        os.remove(dest)
    with open(output + ".phrases.txt", "wb") as f:
        for phrase, count, joins, score in rows:
            f.write(phrase + b"\t%d\t%d\t%.6f\n" % (count, joins, score))
    with open(output + ".phrases.json", "w") as f:
        f.write(json.dumps(result, indent=2, sort_keys=True) + "\n")
    return result


def main(argv=None, backend=None):
    """The command line: `argv` as sys.argv[1:] (default: the process's), `backend` as process_corpus takes it."""
    parser = ArgumentParser(description="Join the collocations of a corpus into phrases (word2phrase) on the GPU.")
    d = " (default: %(default)s)"
    parser.add_argument("--corpus", required=True, help="whitespace-separated text file")
    parser.add_argument("--output", required=True, help="the rewritten corpus; OUTPUT.phrases.txt and OUTPUT.phrases.json go beside it")
    parser.add_argument("--min-count", type=int, default=5, help="words and bigrams seen less often are left alone" + d)
    parser.add_argument("--threshold", type=float, default=100.0, help="a bigram is a phrase where its score exceeds this" + d)
    parser.add_argument("--delimiter", default="_", help="the byte that replaces the space inside a phrase" + d)
    parser.add_argument("--passes", type=int, default=1, help="runs over the tool's own output: 2 makes phrases of up to four words" + d)
    parser.add_argument("--block-bytes", type=int, default=BLOCK_BYTES, help="bytes of the file on the device at a time" + d)
    args = parser.parse_args(argv)
    logger.info("call: %s.", " ".join(sys.argv if argv is None else argv))
    return process_corpus(backend=backend, **args.__dict__)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
