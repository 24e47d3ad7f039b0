#!/usr/bin/env python3
"""us per step of RowWiseAdagrad against LazyAdam and Adagrad forced to its two-launch form (step_form = 1) — the three steps
that share the passes and differ in the apply launch — on the SAME resident plans, one process, interleaved rounds, HIP events
around runs of steps that end in a synchronise.  One JSON line per shape, with the per-touched-id byte accounting of the three
apply launches computed from the shape (what the algorithm needs, not what a counter saw).

  python tools/bench_rowwise_adagrad.py [--shapes c4,c5] [--batches 4] [--rounds 7] [--reps 3] [--arms rowwise,lazyadam,adagrad]

Under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_rowwise_adagrad.py --arms rowwise --rounds 2` the per-kernel
times of the RowWiseAdagrad step come with it (tools/prof_summary.py condenses them)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

SHAPES = {"c4": dict(V=400_000, d=300, B=1 << 20), "c5": dict(V=2_000_000, d=128, B=1 << 20)}
ARMS = {"rowwise": "RowWiseAdagrad", "lazyadam": "LazyAdam", "adagrad": "Adagrad"}


def apply_bytes_per_id(optimizer: str, d: int) -> int:
    """Bytes the apply launch moves per touched id beside what all three share (the id record and the id's partial rows): the
    row W read and written, each table-shaped slot read and written, 8 B per per-row float (bias and its slot(s); RowWiseAdagrad:
    the row's one accumulator too)."""
    row = 4 * d
    if optimizer == "RowWiseAdagrad":
        return 2 * row + 8 * 3                  # W; bias, its accumulator, the row's accumulator
    if optimizer == "Adagrad":
        return 4 * row + 8 * 2                  # W, A; bias, its accumulator
    return 6 * row + 8 * 3                      # LazyAdam: W, m, v; bias, its m and v


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,c5")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="passes over the batches per timed window")
    ap.add_argument("--arms", default="rowwise,lazyadam,adagrad")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowwise_adagrad.py needs a GPU (nothing is timed on the CPU)")
    from trainer.hip_api import STEP_TWO_LAUNCH, DeviceTables, GloveHip, auto_chunk_cap, make_hyper, row_width
    from trainer.synthetic import zipf_sampled
    dev = torch.device("cuda:0")
    hip = GloveHip(dev)
    for name in a.shapes.split(","):
        V, d, B = (SHAPES[name][k] for k in ("V", "d", "B"))
        dpad = row_width(V, d)
        cap = auto_chunk_cap(B, V, dpad)
        row, col, w, y = zipf_sampled(V, B * a.batches, seed=1, device=dev)
        plans = [hip.build_plan(*(x[i * B:(i + 1) * B].contiguous() for x in (row, col, w, y)), V, chunk_cap=cap).compact(hip.lib, dpad)
                 for i in range(a.batches)]
        del row, col, w, y
        ids = statistics.mean(p.host_counts[1] + p.host_counts[3] for p in plans)
        ws = torch.empty(max(hip.lib.glove_step_workspace_bytes(B, p.cap_chunks, dpad) for p in plans), dtype=torch.uint8, device=dev)
        loss = torch.zeros(4, device=dev)
        runs = {}
        for arm in a.arms.split(","):
            opt = ARMS[arm]
            t = DeviceTables(V, d, opt, device=dev, seed=1)
            if opt == "Adagrad":
                h = make_hyper(learning_rate=0.05, batch_size=B, step_form=STEP_TWO_LAUNCH)
                step = lambda p, t=t, h=h: hip.step_adagrad(p, t, h, loss, ws)
            else:
                h = make_hyper(learning_rate=0.05 if opt == "RowWiseAdagrad" else 0.001, batch_size=B, optimizer=opt)
                step = lambda p, t=t, h=h: hip.step_sparse(p, t, h, None, loss, ws)
            assert t.R_ver is None and t.R_tag is None
            for p in plans:                     # warm-up: every plan once
                step(p)
            torch.cuda.synchronize()
            runs[arm] = (step, t, [])
        for rnd in range(a.rounds + 1):         # round 0 is one more warm-up; the arms alternate inside every round
            for arm, (step, t, res) in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    for p in plans:
                        step(p)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    res.append(e0.elapsed_time(e1) * 1e3 / (a.reps * len(plans)))
        out = dict(shape=name, V=V, d=d, row_floats=dpad, B=B, chunk_cap=cap, batches=len(plans), rounds=a.rounds,
                   steps_per_window=a.reps * len(plans), distinct_ids_per_step=round(ids), us_per_step={}, apply_bytes_per_id={},
                   apply_MB_per_step={}, state_MB={})
        for arm, (_, t, res) in runs.items():
            opt = ARMS[arm]
            out["us_per_step"][arm] = dict(median=round(statistics.median(res), 1), min=round(min(res), 1), max=round(max(res), 1))
            out["apply_bytes_per_id"][arm] = apply_bytes_per_id(opt, dpad)
            out["apply_MB_per_step"][arm] = round(apply_bytes_per_id(opt, dpad) * ids / 1e6, 1)
            out["state_MB"][arm] = round(sum(4 * x.numel() for s in (t.s1, t.s2) for x in s.values()) / 1e6, 1)
        print(json.dumps(out), flush=True)
        del runs, plans, ws
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
