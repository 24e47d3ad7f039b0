#!/usr/bin/env python3
"""Measures reads two and three of `python -m trainer.phrases` (the bigram table with the selection, and the join) on the
device against the same rule in plain Python (dicts over split lines, a left-to-right flag), on the same corpus and
machine, one after the other; file I/O is excluded (the blocks are read before the clock starts, the output goes to a
list), the upload of a block and the download of its joined bytes are not.  Then the three entry points of
include/glove_phrases_hip.h alone, on the corpus as one resident block, between device events.

The corpus is synthetic: --tokens Zipf tokens over --types types (default 5 M over 50 k, the shape of DESIGN.md §3h) on
single spaces, lines of 1000 tokens, and --collocations word pairs of their own planted at 2 % of the positions.  Host
clock around work that ends in a synchronise; the median of --repeats runs after a warm-up, and the spread (min - max).
The two paths' outputs are compared.  One JSON line per measurement."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer import cooccur, phrases  # noqa: E402
from trainer.hip_api import GloveHip  # noqa: E402

LINE = 1000


def write_corpus(path, n_tokens, types, collocations, seed=0):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, types + 1)
    words = np.asarray([b"w%d" % i for i in range(types)] + [b"c%da c%db" % (i, i) for i in range(collocations)], dtype=object)
    with open(path, "wb") as f:
        for s in range(0, n_tokens, 1 << 20):
            n = min(1 << 20, n_tokens - s)
            picks = rng.choice(types, size=n, p=p / p.sum())
            planted = rng.random(n) < 0.02
            picks[planted] = types + rng.integers(0, collocations, int(planted.sum()))
            for at in range(0, n, LINE):
                f.write(b" ".join(words[picks[at:at + LINE]]) + b"\n")


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


def kernel_ms(fn, repeats):
    fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def python_bigrams(lines, unigram, tokens, min_count, threshold):
    """{(a, b): score} of the accepted bigrams: the corpus holds single spaces and newlines only, so a line's split is its
    tokens and every pair inside a line is plain."""
    bigram = {}
    for line in lines:
        words = line.split(b" ")
        for pair in zip(words, words[1:]):
            bigram[pair] = bigram.get(pair, 0) + 1
    accepted = {}
    for (a, b), n_ab in bigram.items():
        n_a, n_b = unigram.get(a, 0), unigram.get(b, 0)
        if n_ab >= min_count and n_a >= min_count and n_b >= min_count:
            score = float(n_ab - min_count) / float(n_a) / float(n_b) * float(tokens)
            if score > threshold:
                accepted[a, b] = score
    return accepted


def python_join(lines, accepted, delimiter=b"_"):
    out = []
    for line in lines:
        words = line.split(b" ")
        if not words[0]:
            out.append(line)
            continue
        parts, prev = [words[0]], False
        for pair in zip(words, words[1:]):
            prev = not prev and pair in accepted
            parts.append(delimiter if prev else b" ")
            parts.append(pair[1])
        out.append(b"".join(parts))
    return b"\n".join(out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tokens", type=int, default=5_000_000)
    ap.add_argument("--types", type=int, default=50_000)
    ap.add_argument("--collocations", type=int, default=500)
    ap.add_argument("--min-count", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=100.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--block-bytes", type=int, default=cooccur.BLOCK_BYTES)
    args = ap.parse_args()
    hip = GloveHip("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "corpus.txt"
        write_corpus(path, args.tokens, args.types, args.collocations)
        words, unigram, tokens, _ = phrases.kept_words(path, args.min_count, hip, args.block_bytes)
        kept = cooccur.kept_table_of_bytes([(w, i) for i, w in enumerate(words) if i], hip)
        blocks = list(cooccur.iter_byte_blocks(path, args.block_bytes))
        text = path.read_bytes()
    lines = text.split(b"\n")
    counts = dict(zip(words[1:], unigram[1:].tolist()))

    def device_two():
        return phrases.accepted_phrases(blocks, kept, unigram, tokens, args.min_count, args.threshold, hip)

    (table, bigram_types), two, two_lo, two_hi = timed(device_two, args.repeats)

    def device_three():
        out = []
        phrases.join_blocks(blocks, kept, table[0], ord("_"), hip, out.append)
        return b"".join(out)

    joined, three, three_lo, three_hi = timed(device_three, args.repeats)
    accepted, py_two, py_two_lo, py_two_hi = timed(lambda: python_bigrams(lines, counts, tokens, args.min_count, args.threshold), args.repeats)
    py_joined, py_three, py_three_lo, py_three_hi = timed(lambda: python_join(lines, accepted), args.repeats)
    keys = table[0].cpu().tolist()
    same_table = {(words[k >> 32], words[k & 0xFFFFFFFF]): s for k, s in zip(keys, table[2].cpu().tolist())} == accepted
    same_text = joined == py_joined
    rate = lambda t: round(tokens / t / 1e6, 2)
    for what, d, p, same in (("read_2_bigrams_and_select", (two, two_lo, two_hi), (py_two, py_two_lo, py_two_hi), same_table),
                             ("read_3_join", (three, three_lo, three_hi), (py_three, py_three_lo, py_three_hi), same_text)):
        spread = max(p[2] - p[1], d[2] - d[1])
        print(json.dumps({"what": what, "tokens": tokens, "types": args.types, "kept_types": len(words) - 1,
                          "bigram_types": bigram_types, "phrases": len(keys), "joins": sum(a != b for a, b in zip(text, joined)),
                          "python_s": round(p[0], 4), "python_s_min_max": [round(p[1], 4), round(p[2], 4)],
                          "python_Mtokens_per_s": rate(p[0]),
                          "device_s": round(d[0], 4), "device_s_min_max": [round(d[1], 4), round(d[2], 4)],
                          "device_Mtokens_per_s": rate(d[0]), "python_over_device": round(p[0] / d[0], 2),
                          "larger_spread_s": round(spread, 4), "device_faster_beyond_spread": bool(p[0] - d[0] > spread),
                          "same_result": same}), flush=True)
    # the entry points alone: the whole corpus as one resident block (a corpus beyond 2^31 - 1 bytes takes its first block)
    byte_blocks = [(0, text)] if len(text) < 2 ** 31 else blocks[:1]
    data, start, length, ids, _ = next(phrases.halo_blocks(byte_blocks, kept, hip))
    n = int(start.numel())
    sizes = torch.tensor([n, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64).to(hip.device)
    out_keys = torch.empty(n, dtype=torch.int64, device=hip.device)
    out_counts = torch.empty_like(out_keys)
    ms = kernel_ms(lambda: hip.phrase_bigram_keys_enqueue(data, start, length, ids, sizes[0:1], out_keys, out_counts, sizes[1:3]), args.repeats)
    m = int(sizes[1].item())
    print(json.dumps({"what": "glove_phrase_bigram_keys_i32", "tokens": n, "bytes": int(data.numel()), "keys": m, "ms": round(ms[0], 3),
                      "ms_min_max": [round(ms[1], 3), round(ms[2], 3)], "Mtokens_per_s": round(n / ms[0] / 1e3, 1)}), flush=True)
    sel = [torch.empty(max(m, 1), dtype=t, device=hip.device) for t in (torch.int64, torch.int64, torch.float64)]
    uni = torch.from_numpy(unigram).to(hip.device)
    sizes[3] = m
    ms = kernel_ms(lambda: hip.phrase_select_enqueue(out_keys[:max(m, 1)], out_counts[:max(m, 1)], sizes[3:4], uni, tokens, args.min_count,
                                                     args.threshold, *sel, sizes[4:6]), args.repeats)
    print(json.dumps({"what": "glove_phrase_select", "keys": m, "accepted": int(sizes[4].item()), "ms": round(ms[0], 3),
                      "ms_min_max": [round(ms[1], 3), round(ms[2], 3)], "Mkeys_per_s": round(m / ms[0] / 1e3, 1)}), flush=True)
    carry = torch.zeros(1, dtype=torch.int32, device=hip.device)
    tally = torch.zeros(int(table[0].numel()), dtype=torch.int64, device=hip.device)
    sizes[3] = int(table[0].numel())
    # a joined block has no single spaces left to join: every run starts from the block's own bytes, restored outside the events
    ms_runs = []
    original = data.clone()
    for _ in range(args.repeats + 1):               # (the first run warms up)
        data.copy_(original)
        carry.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip.phrase_join_enqueue(data, start, length, ids, sizes[0:1], table[0], sizes[3:4], ord("_"), carry, tally, sizes[6:8])
        b.record()
        b.synchronize()
        ms_runs.append(a.elapsed_time(b))
    ms_runs = sorted(ms_runs[1:])
    print(json.dumps({"what": "glove_phrase_join_u8", "tokens": n, "phrases": int(table[0].numel()), "joins": int(sizes[6].item()),
                      "ms": round(ms_runs[len(ms_runs) // 2], 3), "ms_min_max": [round(ms_runs[0], 3), round(ms_runs[-1], 3)],
                      "Mtokens_per_s": round(n / ms_runs[len(ms_runs) // 2] / 1e3, 1)}), flush=True)
    assert same_table and same_text
