#!/usr/bin/env python3
"""Times one glove_csr_spmm_f32 (include/glove_factor_hip.h) — the sparse-times-dense product of trainer.svd's range finder
— on a synthetic Zipf table of the C4 vocabulary (V = 400 k rows and columns, l = 312 dense columns), beside
torch.sparse.mm on the same CSR on the same GPU.

Row i holds about c / (i + 1) nonzeros (at most V), c chosen so that they sum to --nnz; the columns are drawn from the
same Zipf law with replacement (a column may repeat in a row).  Both lines are checked against each other, warmed, then
timed with device events around --reps calls, alternating, --rounds times, a window of --window-ms at the least; the table
shows each line's median round and its spread, and the useful bytes per second of the median,
nnz (4 l + 8) + 2 n_rows 4 l: a partner row, a column and a value per nonzero, and a result row written and (by the
second launch, for the rows cut into chunks) read."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from trainer.hip_api import GloveHip, load_factor_library  # noqa: E402

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--nnz", type=int, required=True, help="nonzeros of the table (C4 at V = 400 k: some 10^8; 2 10^7 fits any run)")
cli.add_argument("--vocab", type=int, default=400000)
cli.add_argument("--columns", type=int, default=312, help="dense columns l (300 + 10 oversampled, at the row stride)")
cli.add_argument("--reps", type=int, default=3)
cli.add_argument("--window-ms", type=float, default=200.0)
cli.add_argument("--rounds", type=int, default=5)
cli.add_argument("--no-torch", action="store_true", help="time the library call alone")
args = cli.parse_args()

dev = "cuda:0"
hip = GloveHip(dev)
V, l = args.vocab, args.columns
g = torch.Generator(device=dev).manual_seed(0)
rank = torch.arange(1, V + 1, dtype=torch.float64, device=dev)
lo, hi = 1.0, float(args.nnz)                               # c by bisection: sum_i min(V, floor(c / i)) = nnz, about
for _ in range(60):
    c = (lo + hi) / 2
    lo, hi = (c, hi) if torch.clamp((c / rank).floor(), max=V).sum().item() < args.nnz else (lo, c)
lens = torch.clamp((hi / rank).floor(), max=V).long()
nnz = int(lens.sum())
row_ptr = torch.zeros(V + 1, dtype=torch.int64, device=dev)
row_ptr[1:] = torch.cumsum(lens, 0)
cdf = torch.cumsum(1.0 / rank, 0)
col = torch.searchsorted(cdf / cdf[-1], torch.rand(nnz, generator=g, device=dev, dtype=torch.float64)).clamp_(max=V - 1).to(torch.int32)
val = torch.rand(nnz, generator=g, device=dev) + 0.5
B = torch.randn(V, l, generator=g, device=dev)
ws = torch.empty(load_factor_library().glove_csr_spmm_workspace_bytes(V, nnz, l), dtype=torch.uint8, device=dev)
print("# V = %d, l = %d, nnz = %d; longest row %d, median row %d, rows beyond one chunk %d; workspace %.0f MB"
      % (V, l, nnz, lens.max().item(), lens.median().item(), (lens > 512).sum().item(), ws.numel() / 1e6), file=sys.stderr)


def ours():
    return hip.csr_spmm(row_ptr, col, val, V, V, B, ws)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


lines = {"glove_csr_spmm_f32": ours}
if not args.no_torch:
    A = torch.sparse_csr_tensor(row_ptr, col.long(), val, size=(V, V))
    lines["torch.sparse.mm"] = lambda: torch.sparse.mm(A, B)
    Y1, Y2 = ours(), lines["torch.sparse.mm"]()
    torch.cuda.synchronize()
    print("# largest difference between the two results %.3g (largest entry %.3g)" % ((Y1 - Y2).abs().max().item(), Y2.abs().max().item()),
          file=sys.stderr)
    del Y1, Y2
assert torch.equal(ours(), ours())
reps = max(args.reps, int(args.window_ms / min(timed(fn, 2) for fn in lines.values())) + 1)            # (also the warm-up)
times = {name: [] for name in lines}
for _ in range(args.rounds):
    for name, fn in lines.items():
        times[name].append(timed(fn, reps))
useful = nnz * (4 * l + 8) + 2 * V * 4 * l
print("| call | V | l | nnz | ms per call, median (min - max) | useful TB/s |")
print("|---|---|---|---|---|---|")
for name, t in times.items():
    m = statistics.median(t)
    print("| %s | %d | %d | %d | %.3f (%.3f - %.3f) | %.2f |" % (name, V, l, nnz, m, min(t), max(t), useful / m / 1e9))
