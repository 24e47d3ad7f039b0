#!/usr/bin/env python3
"""ms per call of the 3CosMul top-k (glove_cosmul_topk_f32) against the 3CosAdd top-k (glove_analogy_topk_f32), the baseline:
1,024 questions at V = 400 k, d = 300 (row stride 320), k = 1, the SAME table and questions, one process, the two arms
alternating inside every round, HIP events around runs of --reps calls that end in a synchronise.  One JSON line: the median,
the least and the largest of the rounds per arm, and the ratio of the medians.

  python tools/bench_cosmul.py [--vocab 400000] [--dim 300] [--questions 1024] [--top-k 1] [--epsilon 0.001] [--rounds 7]
                               [--reps 3] [--time-limit 300]

A call through the binding takes its workspace from torch's caching allocator (warm after the first call: no allocation is
timed).  The run ends itself after --time-limit seconds."""
from __future__ import annotations

import argparse
import json
import signal
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=400_000)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--questions", type=int, default=1024)
    ap.add_argument("--top-k", type=int, default=1)
    ap.add_argument("--epsilon", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
    ap.add_argument("--time-limit", type=int, default=300, help="seconds after which the run ends itself")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_cosmul.py needs a GPU (nothing is timed on the CPU)")
    signal.alarm(a.time_limit)                      # SIGALRM's default action ends the process
    from trainer.hip_api import GloveHip, row_width
    dev = torch.device("cuda:0")
    hip = GloveHip(dev)
    V, n, k = a.vocab, a.questions, a.top_k
    d = row_width(V, a.dim)
    g = torch.Generator(device="cpu").manual_seed(0)
    W = torch.zeros(V, d)
    W[:, :a.dim] = torch.randn(V, a.dim, generator=g)
    W = W.to(dev)
    abc = torch.randint(0, V, (n, 3), generator=g, dtype=torch.int32).to(dev)      # (a question may repeat a word)
    arms = {"3cosadd": lambda: hip.analogy_topk(W, abc, k, batch=n),
            "3cosmul": lambda: hip.analogy_cosmul_topk(W, abc, k, a.epsilon, batch=n)}
    res = {arm: [] for arm in arms}
    for call in arms.values():                      # warm-up: code objects, the allocator's blocks
        call()
    torch.cuda.synchronize()
    for rnd in range(a.rounds + 1):                 # round 0 is one more warm-up; the arms alternate inside every round
        for arm, call in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                res[arm].append(e0.elapsed_time(e1) / a.reps)
    out = dict(V=V, d=a.dim, row_floats=d, questions=n, top_k=k, epsilon=a.epsilon, rounds=a.rounds, calls_per_window=a.reps,
               ms_per_call={arm: dict(median=round(statistics.median(r), 3), min=round(min(r), 3), max=round(max(r), 3))
                            for arm, r in res.items()})
    out["ratio_3cosmul_to_3cosadd"] = round(statistics.median(res["3cosmul"]) / statistics.median(res["3cosadd"]), 3)
    out["gemm_tflops_at_median"] = {arm: round(2.0 * mult * n * V * d / (statistics.median(res[arm]) * 1e-3) / 1e12, 1)
                                    for arm, mult in (("3cosadd", 1), ("3cosmul", 3))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
