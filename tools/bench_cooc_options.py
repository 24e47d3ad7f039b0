#!/usr/bin/env python3
"""Measures the preprocessing options of the corpus-to-counts stage (include/glove_cooc_options_hip.h):

  (a) the token filter alone on --tokens Zipf ids over --vocab words with the subsampling table of T = --subsample:
      median time of glove_token_filter_i32 (device events) and its useful bytes over time, 4 B read per token and 4 B
      written per survivor; beside it `ids[mask]` in torch with the mask made beforehand, which favours torch (the
      filter decides and compacts, torch only compacts); the results are compared bit for bit;
  (b) trainer.cooccur end to end (device tokenizer) on a generated corpus file of --corpus-tokens tokens, with and without
      the filter: tokens read per second, host clock around the whole call.

One JSON line per measurement."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer import cooccur  # noqa: E402
from trainer.hip_api import GloveHip, load_prep_library  # noqa: E402

dev = torch.device("cuda:0")


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


def zipf_ids(n, V, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cdf = torch.arange(1, V + 1, dtype=torch.float64, device=dev).pow(-1.0).cumsum(0)
    return torch.searchsorted(cdf / cdf[-1], torch.rand(n, dtype=torch.float64, device=dev, generator=g)).clamp_(max=V - 1).int()


def bench_filter(hip, n, V, T, seed, repeats):
    lib = load_prep_library()
    ids = zipf_ids(n, V, 0)
    counts = torch.bincount(ids, minlength=V).cpu().numpy()
    table = cooccur.subsample_thresholds(counts, T)
    thr = torch.from_numpy(table.view(np.int32).copy()).to(dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.zeros(2, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.glove_token_filter_workspace_bytes(n), dtype=torch.uint8, device=dev)
    run = lambda: hip.token_filter_enqueue(ids, 0, thr, seed, out, n_out, ws)
    med, lo, hi = timed(run, repeats)
    kept = int(n_out[0].item())
    useful = 4 * (n + kept)
    from_filter = out[:kept].clone()
    # torch: only the compaction is timed, the mask is made beforehand.  The mask comes from filtering the POSITIONS
    # 0 .. n - 1 under a table that gives position i its token's threshold: the same hash of the same positions, so the
    # same decisions, and the survivors are the kept positions.
    positions = torch.arange(n, dtype=torch.int32, device=dev)
    per_position = thr[ids.long()]
    pos_out = torch.empty(n, dtype=torch.int32, device=dev)
    hip.token_filter_enqueue(positions, 0, per_position, seed, pos_out, n_out, ws)
    assert int(n_out[0].item()) == kept
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[pos_out[:kept].long()] = True
    del positions, per_position, pos_out
    tmed, tlo, thi = timed(lambda: ids[mask], max(1, repeats // 2))
    same = bool(torch.equal(ids[mask], from_filter))
    print(json.dumps({"what": "token_filter", "tokens": n, "V": V, "subsample": T, "kept": kept, "kept_share": round(kept / n, 4),
                      "filter_ms": round(med, 3), "filter_ms_min_max": [round(lo, 3), round(hi, 3)], "useful_bytes": useful,
                      "useful_TB_per_s": round(useful / med / 1e9, 3), "torch_masked_select_ms": round(tmed, 3),
                      "torch_ms_min_max": [round(tlo, 3), round(thi, 3)], "torch_over_filter": round(tmed / med, 2),
                      "same_result": same}), flush=True)
    assert same


def write_corpus(path, n, V, seed):
    """n Zipf tokens "w<id>" separated by single spaces, a newline every 1000 tokens."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, V + 1)
    words = np.asarray(["w%d" % i for i in range(V)], dtype=object)
    with open(path, "w") as f:
        for s in range(0, n, 1 << 20):
            ids = rng.choice(V, size=min(1 << 20, n - s), p=p / p.sum())
            lines = [" ".join(words[ids[i:i + 1000]]) for i in range(0, len(ids), 1000)]
            f.write("\n".join(lines) + "\n")


def bench_end_to_end(hip, n, V, T, repeats):
    with tempfile.TemporaryDirectory() as tmp:
        corpus = Path(tmp) / "corpus.txt"
        write_corpus(corpus, n, V, 1)
        for name, options in (("cooccur_plain", {}), ("cooccur_filtered", dict(subsample=T, delete_unknown=True))):
            times = []
            for it in range(repeats + 1):                   # the first run warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                data = cooccur.process_corpus(str(corpus), None, 0.95, 5, cooccur.CHUNK_TOKENS, 10, 0, backend=hip,
                                              tokenizer="device", **options)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            times = sorted(times[1:])
            med = times[len(times) // 2]
            prep = data.get("prep", {"tokens_read": n, "tokens_kept": n})
            print(json.dumps({"what": name, "tokens": n, "V": V, "options": options, "tokens_kept": prep["tokens_kept"],
                              "pairs": int(len(data["interaction"]["count"])), "s": round(med, 3),
                              "s_min_max": [round(times[0], 3), round(times[-1], 3)],
                              "M_tokens_per_s": round(n / med / 1e6, 2)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tokens", type=int, default=64 << 20)
    ap.add_argument("--vocab", type=int, default=400_000)
    ap.add_argument("--subsample", type=float, default=1e-5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--corpus-tokens", type=int, default=16 << 20, help="0 skips the end-to-end runs")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    hip = GloveHip(dev)
    bench_filter(hip, args.tokens, args.vocab, args.subsample, args.seed, args.repeats)
    torch.cuda.empty_cache()
    if args.corpus_tokens:
        bench_end_to_end(hip, args.corpus_tokens, args.vocab, args.subsample, max(2, args.repeats // 4))
