#!/usr/bin/env python3
"""Measures counting a corpus chunk by chunk (include/glove_cooc_stream_hip.h) on the corpus of tools/bench_cooc.py
(17 M Zipf tokens, V = 10 k, window 5):

  (a) the merge alone, a state of --state-keys keys against a chunk of --chunk-keys: median time of glove_cooc_merge_u64
      (device events) and bytes moved over time, 16 B per entry read and written; beside it the same result from library
      calls on the same buffers (torch.cat, sort, unique_consecutive, a segmented sum);
  (b) the whole table, streamed at --chunk-tokens, against the one-shot glove_cooccurrence_i32 on the same tokens
      (host clock around work that ends in a synchronise; the results are compared bit for bit);
  (c) the peak device memory of each run of (b) (torch.cuda.max_memory_allocated).

One JSON line per measurement."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from trainer.cooccur import CoocAccumulator  # noqa: E402
from trainer.hip_api import GloveHip, load_prep_library  # noqa: E402

dev = torch.device("cuda:0")


def ascending_keys(n, mean_gap, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(1, 2 * mean_gap, (n,), dtype=torch.int64, device=dev, generator=g).cumsum_(0)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return sorted(times)[len(times) // 2], min(times), max(times)


def bench_merge(hip, n_state, n_chunk, repeats):
    lib = load_prep_library()
    span_gap = 4
    keys_a = ascending_keys(n_state, span_gap, 1)
    keys_b = ascending_keys(n_chunk, max(1, span_gap * n_state // n_chunk), 2)
    counts_a, counts_b = torch.ones_like(keys_a), torch.full_like(keys_b, 3)
    sizes = torch.tensor([n_state, n_chunk, 0, 0], dtype=torch.int64).to(dev)
    keys_o = torch.empty(n_state + n_chunk, dtype=torch.int64, device=dev)
    counts_o = torch.empty_like(keys_o)
    ws = torch.empty(lib.glove_cooc_merge_workspace_bytes(n_state, n_chunk), dtype=torch.uint8, device=dev)
    run = lambda: hip.cooc_merge_enqueue(keys_a, counts_a, sizes[0:1], keys_b, counts_b, sizes[1:2], keys_o, counts_o, sizes[2:4], ws)
    med, lo, hi = timed(run, repeats)
    n_out = int(sizes[2].item())
    moved = 16 * (n_state + n_chunk + n_out)

    def library():
        keys = torch.cat([keys_a, keys_b])
        counts = torch.cat([counts_a, counts_b])
        keys, order = torch.sort(keys)
        uk, inverse = torch.unique_consecutive(keys, return_inverse=True)
        return uk, torch.zeros_like(uk).index_add_(0, inverse, counts[order])
    lmed, llo, lhi = timed(library, max(1, repeats // 2))
    uk, uc = library()
    same = bool(torch.equal(uk, keys_o[:n_out]) and torch.equal(uc, counts_o[:n_out]))
    print(json.dumps({"what": "merge", "state_keys": n_state, "chunk_keys": n_chunk, "out_keys": n_out, "twins": n_state + n_chunk - n_out,
                      "merge_ms": round(med, 3), "merge_ms_min_max": [round(lo, 3), round(hi, 3)],
                      "bytes_moved": moved, "TB_per_s": round(moved / med / 1e9, 3),
                      "library_ms": round(lmed, 3), "library_ms_min_max": [round(llo, 3), round(lhi, 3)],
                      "library_over_merge": round(lmed / med, 2), "same_result": same}), flush=True)
    assert same


def bench_table(hip, chunk_lengths, repeats):
    n, V, ctx = 17_005_207, 10_000, 5
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    cdf = torch.arange(1, V + 1, dtype=torch.float64, device=dev).pow(-1.0).cumsum(0)
    tok = torch.searchsorted(cdf / cdf[-1], torch.rand(n, dtype=torch.float64, device=dev, generator=g)).clamp_(max=V - 1).int()
    del cdf

    def one_shot():
        return hip.cooccurrence(tok, V, ctx)

    def streamed(chunk):
        acc = CoocAccumulator(V, ctx, hip)
        for s in range(0, n, chunk):
            e = min(s + chunk, n)
            acc.add(tok[s:min(e + ctx, n)], e - s)
        return acc.finalize(0)

    want = None
    for name, fn in [("one_shot", one_shot)] + [("streamed_%d" % c, (lambda c=c: streamed(c))) for c in chunk_lengths]:
        times = []
        for it in range(repeats + 1):                   # the first run warms up
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            peak = torch.cuda.max_memory_allocated() - base
            if want is None:
                want = [t.clone() for t in got]
            same = all(torch.equal(a, b) for a, b in zip(got, want))
            del got
        times = sorted(times[1:])
        print(json.dumps({"what": name, "tokens": n, "V": V, "context": ctx, "pairs": int(want[0].numel()),
                          "ms": round(times[len(times) // 2], 1), "ms_min_max": [round(times[0], 1), round(times[-1], 1)],
                          "peak_device_bytes": int(peak), "same_as_one_shot": same}), flush=True)
        assert same


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--state-keys", type=int, nargs="*", default=[10 ** 7, 10 ** 8, 5 * 10 ** 8])
    ap.add_argument("--chunk-keys", type=int, default=10 ** 7)
    ap.add_argument("--chunk-tokens", type=int, nargs="*", default=[1 << 20, 4 << 20, 17_005_207])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    hip = GloveHip(dev)
    for n_state in args.state_keys:
        bench_merge(hip, n_state, args.chunk_keys, args.repeats)
        torch.cuda.empty_cache()
    if args.chunk_tokens:
        bench_table(hip, args.chunk_tokens, max(2, args.repeats // 2))
