#!/usr/bin/env python3
"""Times one spherical k-means iteration (glove_kmeans_assign_f32 + glove_kmeans_update_f32): every row of a table of V
words, d = 300, into K clusters — (V, K) = (50 k, 500), (400 k, 500), (400 k, 4096) — beside the same iteration in plain
torch ops on the same GPU.

The torch line is matmul of the unit rows with the unit centroids in blocks of --torch-block points (an n x K matrix at
once is 6.5 GB at the largest size), argmax, index_add_ of the unit rows and a normalisation; it keeps the unit rows in
memory, which the kernels do not.  Both lines are warmed, then timed with device events around --reps iterations,
alternating, --rounds times, a window of 0.2 s at the least; the table shows each line's median round and its spread.  The two are checked against each
other first: the same assignment except near ties, the same centroids within float32 tolerance."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from trainer.hip_api import GloveHip, row_width  # noqa: E402

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--sizes", default="50000:500,400000:500,400000:4096", help="comma-separated V:K")
cli.add_argument("--dim", type=int, default=300)
cli.add_argument("--reps", type=int, default=5, help="iterations per timed window at the least (more where a window would stay under --window-ms)")
cli.add_argument("--window-ms", type=float, default=200.0)
cli.add_argument("--rounds", type=int, default=5)
cli.add_argument("--torch-block", type=int, default=65536)
args = cli.parse_args()

hip = GloveHip("cuda:0")
dev = "cuda:0"


def torch_iteration(X, cents, block):
    """X: unit rows [n, d].  -> (assign, cos, new centroids, counts)."""
    Cn = cents * torch.rsqrt(torch.clamp((cents * cents).sum(1, keepdim=True), min=1e-12))
    assign = torch.empty(X.shape[0], dtype=torch.int64, device=X.device)
    cos = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    for s in range(0, X.shape[0], block):
        best = torch.max(X[s:s + block] @ Cn.T, dim=1)
        assign[s:s + block], cos[s:s + block] = best.indices, best.values
    sums = torch.zeros_like(cents).index_add_(0, assign, X)
    counts = torch.bincount(assign, minlength=cents.shape[0])
    new = sums * torch.rsqrt(torch.clamp((sums * sums).sum(1, keepdim=True), min=1e-12))
    return assign, cos, torch.where(counts[:, None] > 0, new, cents), counts


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


print("| V | d (stride) | K | kernels, ms per iteration (min - max) | torch ops, ms per iteration (min - max) | assign / update share of the kernels |")
print("|---|---|---|---|---|---|")
for size in args.sizes.split(","):
    V, K = (int(x) for x in size.split(":"))
    d = row_width(V, args.dim)
    g = torch.Generator(device="cpu").manual_seed(0)
    W = torch.zeros(V, d)
    W[:, :args.dim] = torch.randn(V, args.dim, generator=g)
    W = W.to(dev)
    ids = torch.arange(V, dtype=torch.int32, device=dev)
    cents = W[torch.randperm(V, generator=g)[:K].to(dev)].contiguous()
    X = W * torch.rsqrt(torch.clamp((W * W).sum(1, keepdim=True), min=1e-12))
    ws = hip.kmeans_workspace(V, V, d, K, dev)

    def ours():
        a, c = hip.kmeans_assign(W, ids, cents, ws)
        return (a, c) + hip.kmeans_update(W, ids, a, cents, ws)

    theirs = lambda: torch_iteration(X, cents, args.torch_block)
    a1, c1, n1, k1 = ours()
    a2, c2, n2, k2 = theirs()
    torch.cuda.synchronize()
    differ = (a1.long() != a2)
    near = (c1 - c2).abs().max().item()
    same_counts = differ.sum().item() == 0
    print("# V=%d K=%d: %d of %d assignments differ (largest cosine difference %.3g); centroids differ by %.3g at the most%s"
          % (V, K, differ.sum().item(), V, near, (n1 - n2).abs().max().item() if same_counts else float("nan"),
             "" if same_counts else " (not compared: the assignments differ)"), file=sys.stderr)
    t_ours, t_theirs, t_assign = [], [], []
    reps = max(args.reps, int(args.window_ms / min(timed(ours, 2), timed(theirs, 2))) + 1)       # (also the warm-up)
    for _ in range(args.rounds):
        t_ours.append(timed(ours, reps))
        t_theirs.append(timed(theirs, reps))
        t_assign.append(timed(lambda: hip.kmeans_assign(W, ids, cents, ws), reps))
    mo, mt, ma = statistics.median(t_ours), statistics.median(t_theirs), statistics.median(t_assign)
    print("| %d | %d (%d) | %d | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.0f %% / %.0f %% |"
          % (V, args.dim, d, K, mo, min(t_ours), max(t_ours), mt, min(t_theirs), max(t_theirs), 100 * ma / mo, 100 * (1 - ma / mo)))
    del W, X, ws
