#!/usr/bin/env python3
"""ms per step of the sharded forms under Adam against sharded Adagrad, the plain single-GPU Adam step and the data-parallel
dense Adam step, on one rank with every collective of a form issued through RCCL (a process group of one rank: the exchange
exercised); and the bytes/s of the touched-rows apply's sweep over the unlisted rows (decay_unmarked_kernel) against
dense_adam_kernel on the same tables in the same process.  One JSON line per shape.

  python tools/bench_sharded_optimizers.py [--shapes c4,c5] [--steps 20] [--warmup 5] [--batches 4]

Under `rocprofv3 --kernel-trace --stats -- python tools/bench_sharded_optimizers.py ...` the per-kernel times come with it
(tools/prof_summary.py condenses them: profiles/r06_*_sharded_adam_kernel_stats.txt; the JSON lines of a run:
profiles/r06_sharded_optimizers_bench.txt)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import torch  # noqa: E402

SHAPES = {"c4": dict(V=400_000, d=300, B=1 << 20), "c5": dict(V=2_000_000, d=128, B=1 << 20)}


def timed(fn, steps, warmup, reps=3):
    """Median over `reps` runs of `steps` calls (after `warmup`) of the ms per call, by events on the current stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return statistics.median(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,c5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    args = ap.parse_args(argv)
    import torch.distributed as dist
    from trainer.hip_api import DeviceTables, make_hyper
    from trainer.stepper import HipBackend, RowShardedStepper, ShardedStepper, Stepper
    from trainer.synthetic import zipf_sampled
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29561")
    os.environ.update(RANK="0", WORLD_SIZE="1")
    dist.init_process_group("nccl", device_id=torch.device("cuda:0"))
    dev = "cuda:0"
    try:
        for name in args.shapes.split(","):
            V, d, B = SHAPES[name]["V"], SHAPES[name]["d"], SHAPES[name]["B"]
            row, col, w, y = zipf_sampled(V, B * args.batches, seed=1, device=dev)
            batches = [tuple(x[i * B:(i + 1) * B].contiguous() for x in (row, col, w, y)) for i in range(args.batches)]
            kw = dict(l2_reg=0.01, reg_mult=2.0, learning_rate=0.001)
            res = dict(shape=name, V=V, d=d, B=B, ms_per_step={})

            def form(label, opt, make):
                backend = HipBackend(dev)
                tables = DeviceTables(V, d, opt, device=dev, seed=0)
                st, items = make(backend, tables, dict(kw, optimizer=opt))
                k = [0]

                def one():
                    st.step(items[k[0] % len(items)])
                    k[0] += 1
                res["ms_per_step"][label] = round(timed(one, args.steps, args.warmup), 4)
                del st, items, tables, backend
                torch.cuda.synchronize()
                torch.cuda.empty_cache()

            def plans_for(backend):
                return [backend.build_plan(*bt, V, 0) for bt in batches]

            def sharded(backend, tables, hkw):
                st = ShardedStepper(backend, tables, hkw, B, 1, 0, dist, collectives=True, exercise_exchange=True)
                return st, [st.add_batch(*bt) for bt in batches]

            def row_sharded(exchange):
                def make(backend, tables, hkw):
                    st = RowShardedStepper(backend, tables, hkw, B, 1, dist, exchange=exchange, collectives=True)
                    plans = plans_for(backend)
                    st.prepare(plans)
                    return st, plans
                return make

            def plain(backend, tables, hkw):
                return Stepper(backend, tables, hkw, B), plans_for(backend)

            def data_parallel(backend, tables, hkw):
                st = Stepper(backend, tables, hkw, B, world=1, dist=dist, exchange="dense", collectives=True)
                return st, plans_for(backend)

            form("sharded_adagrad_both_tables", "Adagrad", sharded)
            form("sharded_adam_both_tables", "Adam", sharded)
            form("sharded_adam_rows_lists", "Adam", row_sharded("rows"))
            form("sharded_adam_rows_dense", "Adam", row_sharded("dense"))
            form("plain_adam_one_gpu", "Adam", plain)
            form("data_parallel_dense_adam_rccl", "Adam", data_parallel)
            # the sweep against dense_adam_kernel on the same tables: an apply of one empty list sweeps every row; the dense apply on a
            # zero gradient moves the same rows
            backend = HipBackend(dev)
            hip = backend.hip
            tables = DeviceTables(V, d, "Adam", device=dev, seed=0)
            G = hip.dense_grad_buffer(tables)
            mark = torch.zeros(tables.V_row + tables.V, dtype=torch.int32, device=dev)
            empty = torch.zeros(1, tables.d + 4, device=dev)
            lst = [hip.packed_list(empty, with_header=False, n=0)]
            h = make_hyper(batch_size=B, optimizer="Adam", **kw)
            tail = torch.zeros(4, device=dev)
            t_sweep = timed(lambda: hip.apply_packed(lst, tables, h, G, mark, tail, None, 0), args.steps, args.warmup)
            t_dense = timed(lambda: hip.dense_adam(tables, h, G, None), args.steps, args.warmup)
            # each kernel at the bytes it moves: the sweep 24 B per float (w, m, v read and written; + one 4-B mark per row),
            # dense_adam_kernel 28 B (it reads G as well; a zero gradient is not written back)
            floats = 2 * V * tables.d + 2 * V
            rows = 2 * V
            res["sweep_us"], res["dense_adam_us"] = round(1e3 * t_sweep, 2), round(1e3 * t_dense, 2)
            res["sweep_GBps"] = round((24 * floats + 4 * rows) / (t_sweep * 1e-3) / 1e9, 1)
            res["dense_adam_GBps"] = round(28 * floats / (t_dense * 1e-3) / 1e9, 1)
            res["sweep_over_dense_bytes_per_s"] = round(res["sweep_GBps"] / res["dense_adam_GBps"], 3)
            ms = res["ms_per_step"]
            # the acceptance bound: sharded Adagrad + the sweep of both tables at the measured rate
            res["bound_ms_adagrad_plus_sweep"] = round(ms["sharded_adagrad_both_tables"] + t_sweep, 4)
            del tables, G, mark, backend
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
