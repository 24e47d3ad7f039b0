#!/usr/bin/env python3
"""Times the three calls of include/glove_factor_dense_hip.h and the whole of trainer.postprocess.postprocess_table on a
table of the C4 vocabulary (V = 400 k rows, d = 300 in its row stride), beside torch on the same GPU in the same process:
the Gram matrix from X.double().T @ X.double() and from X.T @ X, the product from torch.matmul.

Every line is checked against its neighbour, warmed, then timed with device events around --reps calls, alternating,
--rounds times, a window of --window-ms at the least; the table shows each line's median round and its spread, and two
figures to hold it against, both bounds and not targets: the time the bytes the call must move take at the measured
HBM copy rate (6.29 TB/s), and the time its multiply-adds take at the measured f32 MFMA rate (155 TFLOP/s) — the whole
d x d matrix for the Gram call, of which the kernel computes the upper triangle's blocks."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer.hip_api import GloveHip, load_factor_library, row_width  # noqa: E402
from trainer.postprocess import postprocess_table  # noqa: E402

HBM_BYTES_PER_S, MFMA_F32_FLOPS = 6.29e12, 155e12

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--vocab", type=int, default=400000)
cli.add_argument("--embedding-size", type=int, default=300)
cli.add_argument("--reduce-to", type=int, default=150, help="columns of the second transform line")
cli.add_argument("--reps", type=int, default=3)
cli.add_argument("--window-ms", type=float, default=200.0)
cli.add_argument("--rounds", type=int, default=5)
cli.add_argument("--no-torch", action="store_true", help="time the library calls alone")
args = cli.parse_args()

dev = "cuda:0"
hip = GloveHip(dev)
V, d_model = args.vocab, args.embedding_size
d = row_width(V, d_model)
g = torch.Generator(device=dev).manual_seed(0)
X = torch.zeros(V, d, device=dev)
X[:, :d_model] = torch.randn(V, d_model, generator=g, device=dev) + 3.0 * torch.randn(d_model, generator=g, device=dev)
ws = torch.empty(load_factor_library().glove_gram_workspace_bytes(V, d), dtype=torch.uint8, device=dev)
mean = (hip.col_sums(X, ws) / V).float()
m = (args.reduce_to + 3) // 4 * 4
T_full = torch.randn(d, d, generator=g, device=dev)
T_red = torch.randn(m, d, generator=g, device=dev)
shift_full, shift_red = T_full @ mean, T_red @ mean
Y_full, Y_red = torch.empty(V, d, device=dev), torch.empty(V, m, device=dev)
print("# V = %d, d = %d (row stride %d), reduce to %d (%d rows of T); workspace %.1f MB" % (V, d_model, d, args.reduce_to, m, ws.numel() / 1e6),
      file=sys.stderr)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


# name -> (call, bytes it must move, multiply-adds x 2)
table_bytes = V * d * 4
lines = {
    "glove_col_sums_f64": (lambda: hip.col_sums(X, ws), table_bytes, 0),
    "glove_gram_f64": (lambda: hip.gram(X, mean, ws), table_bytes, 2 * V * d * d),
    "glove_rows_transform_f32, m = %d" % d: (lambda: hip.rows_transform(X, T_full, shift_full, Y_full), 2 * table_bytes, 2 * V * d * d),
    "glove_rows_transform_f32, m = %d" % m: (lambda: hip.rows_transform(X, T_red, shift_red, Y_red), table_bytes + V * m * 4, 2 * V * d * m),
}
if not args.no_torch:
    Xc = X - mean
    lines["torch: Xc.double().T @ Xc.double()"] = (lambda: Xc.double().T @ Xc.double(), table_bytes, 2 * V * d * d)
    lines["torch: Xc.T @ Xc (float32)"] = (lambda: Xc.T @ Xc, table_bytes, 2 * V * d * d)
    lines["torch: X @ T.T - shift, m = %d" % d] = (lambda: torch.matmul(X, T_full.T) - shift_full, 2 * table_bytes, 2 * V * d * d)
    lines["torch: X @ T.T - shift, m = %d" % m] = (lambda: torch.matmul(X, T_red.T) - shift_red, table_bytes + V * m * 4, 2 * V * d * m)
    G, G64, G32 = hip.gram(X, mean, ws), Xc.double().T @ Xc.double(), (Xc.T @ Xc).double()
    Y, Yt = hip.rows_transform(X, T_red, shift_red), torch.matmul(X, T_red.T) - shift_red
    torch.cuda.synchronize()
    print("# Gram matrix, largest difference from torch float64 over the largest entry: ours %.3g, torch float32 %.3g"
          % ((G - G64).abs().max().item() / G64.abs().max().item(), (G32 - G64).abs().max().item() / G64.abs().max().item()), file=sys.stderr)
    print("# transform, largest difference from torch.matmul %.3g (largest entry %.3g)" % ((Y - Yt).abs().max().item(), Yt.abs().max().item()),
          file=sys.stderr)
    del G, G64, G32, Y, Yt
assert torch.equal(hip.gram(X, mean, ws), hip.gram(X, mean, ws))
reps = {name: max(args.reps, int(args.window_ms / timed(fn, 2)) + 1) for name, (fn, _, _) in lines.items()}       # (also the warm-up)
times = {name: [] for name in lines}
for _ in range(args.rounds):
    for name, (fn, _, _) in lines.items():
        times[name].append(timed(fn, reps[name]))
print("| call | V | d | ms per call, median (min - max) | bound: bytes at 6.29 TB/s, ms | bound: flops at 155 TF, ms |")
print("|---|---|---|---|---|---|")
for name, t in times.items():
    _, nbytes, flops = lines[name]
    print("| %s | %d | %d | %.3f (%.3f - %.3f) | %.3f | %.3f |" % (name, V, d, statistics.median(t), min(t), max(t),
                                                                 nbytes / HBM_BYTES_PER_S * 1e3, flops / MFMA_F32_FLOPS * 1e3))

# the whole driver, host phases included (upload, eigh on the host, download): seconds per phase of the median run
W = X[:, :d_model].cpu().numpy()
runs = []
for _ in range(1 + max(3, args.rounds)):
    t0 = time.perf_counter()
    out = postprocess_table(W, remove=max(1, round(d_model / 100)), reduce_to=args.reduce_to, backend=hip)
    runs.append((time.perf_counter() - t0, out["seconds"]))
runs = sorted(runs[1:], key=lambda r: r[0])                  # (the first run is the warm-up)
total, phases = runs[len(runs) // 2]
print("| postprocess_table, remove %d, reduce to %d | %d | %d | %.1f (%.1f - %.1f) | %s |  |" % (
    max(1, round(d_model / 100)), args.reduce_to, V, d, total * 1e3, runs[0][0] * 1e3, runs[-1][0] * 1e3,
    ", ".join("%s %.1f" % (k, v * 1e3) for k, v in phases.items())))
