#!/usr/bin/env python3
"""Measures the two host passes of `python -m trainer.cooccur` over a corpus file, with --tokenizer python and with
--tokenizer device (include/glove_text_hip.h), on the same file and machine, one after the other:

  pass one   the vocabulary: count the tokens, choose the kept words (python: Counter over str.split(); device:
             tokenize, block vocabulary, merge, then the kept strings read back from the file);
  pass two   the ids of every token (python: dict lookups into a numpy array per block; device: tokenize, look the
             hashes up, compare the bytes; the ids stay on the device, where CoocAccumulator takes them).

The corpus is synthetic: --tokens Zipf tokens over --types types (default 5 M over 50 k, the shape of DESIGN.md §3g).
Host clock around work that ends in a synchronise; the median of --repeats runs after a warm-up, and the spread
(min - max).  The vocabularies and the ids of the two paths are compared.  One JSON line per measurement."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer import cooccur, text8  # noqa: E402
from trainer.hip_api import GloveHip  # noqa: E402


def write_corpus(path, n_tokens, types, seed=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, types + 1)
    words = np.asarray([b"w%d" % i for i in range(types)], dtype=object)
    with open(path, "wb") as f:
        for s in range(0, n_tokens, 1 << 20):
            picks = rng.choice(types, size=min(1 << 20, n_tokens - s), p=p / p.sum())
            f.write(b" ".join(words[picks]) + b"\n")


def timed(fn, repeats):
    out = fn()                                      # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    return out, times[len(times) // 2], times[0], times[-1]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tokens", type=int, default=5_000_000)
    ap.add_argument("--types", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--block-bytes", type=int, default=cooccur.BLOCK_BYTES)
    args = ap.parse_args()
    hip = GloveHip("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "corpus.txt"
        write_corpus(path, args.tokens, args.types)

        def python_vocab():
            return text8.vocabulary_from_counts(cooccur.count_vocabulary(path, args.block_bytes), text8.VOCAB_SIZE, text8.COVERAGE)

        def device_vocab():
            return cooccur.device_vocabulary(path, text8.VOCAB_SIZE, text8.COVERAGE, hip, args.block_bytes)

        def python_ids(lookup):
            return [np.fromiter((lookup.get(t, 0) for t in tokens), dtype=np.int32, count=len(tokens))
                    for tokens in cooccur.iter_token_blocks(path, args.block_bytes)]

        def device_ids(lookup):
            return list(cooccur.device_id_blocks(path, lookup, hip, args.block_bytes))

        results = {}
        for name, vocab_fn, ids_fn in (("python", python_vocab, python_ids), ("device", device_vocab, device_ids)):
            vocab, med, lo, hi = timed(vocab_fn, args.repeats)
            results[name, 1] = (med, lo, hi, vocab)
            lookup = {tok: i for i, tok in enumerate(vocab[0])}
            ids, med, lo, hi = timed(lambda: ids_fn(lookup), args.repeats)
            results[name, 2] = (med, lo, hi, ids)
        same_vocab = results["python", 1][3][0] == results["device", 1][3][0] and \
            bool((results["python", 1][3][1] == results["device", 1][3][1]).all())
        same_ids = bool(np.array_equal(np.concatenate(results["python", 2][3]),
                                       torch.cat(results["device", 2][3]).cpu().numpy()))
        for pass_ in (1, 2):
            p, d = results["python", pass_], results["device", pass_]
            spread = max(p[2] - p[1], d[2] - d[1])
            rate = lambda t: round(args.tokens / t / 1e6, 2)
            print(json.dumps({"what": "pass_%d" % pass_, "tokens": args.tokens, "types": args.types, "vocab": len(results["python", 1][3][0]),
                              "python_s": round(p[0], 3), "python_s_min_max": [round(p[1], 3), round(p[2], 3)],
                              "python_Mtokens_per_s": rate(p[0]),
                              "device_s": round(d[0], 3), "device_s_min_max": [round(d[1], 3), round(d[2], 3)],
                              "device_Mtokens_per_s": rate(d[0]), "python_over_device": round(p[0] / d[0], 2),
                              "larger_spread_s": round(spread, 3), "device_faster_beyond_spread": bool(p[0] - d[0] > spread),
                              "same_result": same_vocab if pass_ == 1 else same_ids}), flush=True)
        assert same_vocab and same_ids
