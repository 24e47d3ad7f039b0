#!/usr/bin/env python3
"""Times trainer.retrofit's two schedules on a synthetic lexicon over a table of the C4 vocabulary (V = 400 k rows, d = 300
in its row stride): 100 k keys whose degrees follow a power law with a mean of about 8 (neighbours drawn among the keys,
not symmetrised) plus one planted hub of 4,096 neighbours, 10 sweeps.  Beside them, on the same lexicon:
  (a) the Jacobi sweep written with what the libraries had before: GloveHip.csr_spmm plus torch elementwise operations, on
      the same GPU in the same process;
  (b) Faruqui's loop (retrofit.py: in place, key by key) restated in NumPy on the CPU, keys in vocabulary order.

Every GPU line is checked against its neighbour, warmed, then timed with device events around --reps runs of 10 sweeps,
alternating, --rounds times; the table shows each line's median round and its spread.  The hub row's share is the time of
the one-row call on the hub (a single lane group walking 4,096 partner rows) over the time of a sweep.  Figures to hold the
sweeps against, bounds and not targets: the bytes a sweep must move (every gathered row, every updated row read from Q^ and
written once; the Jacobi sweep also copies the rows without neighbours) at the measured HBM copy rate (6.29 TB/s)."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer.hip_api import GloveHip, row_width  # noqa: E402
from trainer.retrofit import level_schedule, retrofit_table  # noqa: E402

HBM_BYTES_PER_S = 6.29e12

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--vocab", type=int, default=400000)
cli.add_argument("--embedding-size", type=int, default=300)
cli.add_argument("--keys", type=int, default=100000)
cli.add_argument("--mean-degree", type=float, default=8.0)
cli.add_argument("--max-degree", type=int, default=256)
cli.add_argument("--hub", type=int, default=4096, help="neighbours of the one planted hub (0: none)")
cli.add_argument("--iterations", type=int, default=10)
cli.add_argument("--alpha", type=float, default=1.0)
cli.add_argument("--reps", type=int, default=3)
cli.add_argument("--rounds", type=int, default=5)
cli.add_argument("--no-cpu", action="store_true", help="leave the NumPy loop out")
args = cli.parse_args()


def power_law_degrees(rng, n, mean, cap):
    """n degrees in [1, cap] with p(k) ~ k^-a, a bisected so that the distribution's mean is `mean`."""
    k = np.arange(1, cap + 1, dtype=np.float64)
    lo, hi = 0.0, 6.0
    for _ in range(60):
        a = (lo + hi) / 2
        p = k ** -a
        p /= p.sum()
        lo, hi = (a, hi) if (p * k).sum() > mean else (lo, a)
    return rng.choice(np.arange(1, cap + 1), n, p=p), a


def synthetic_lexicon(V, n_keys, mean, cap, hub, seed=0):
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(V, n_keys, replace=False))
    deg, a = power_law_degrees(rng, n_keys, mean, cap)
    hub_key = int(keys[n_keys // 2]) if hub else -1
    if hub:
        deg[n_keys // 2] = hub
    lens = np.zeros(V, np.int64)
    lens[keys] = deg
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = keys[rng.integers(0, n_keys, int(row_ptr[-1]))].astype(np.int32)       # with repetition, like a merged lexicon's would not: harmless
    return row_ptr, col, keys, hub_key, a


dev = "cuda:0"
hip = GloveHip(dev)
V, d_model, T = args.vocab, args.embedding_size, args.iterations
d = row_width(V, d_model)
row_ptr_h, col_h, keys, hub_key, exponent = synthetic_lexicon(V, args.keys, args.mean_degree, args.max_degree, args.hub)
nnz = len(col_h)
t0 = time.perf_counter()
rows_h, offsets = level_schedule(row_ptr_h, col_h, V)
t_schedule = time.perf_counter() - t0
sizes = np.diff(offsets)
print("# V = %d, d = %d (row stride %d); %d keys, %d edges (mean degree %.2f, p(k) ~ k^-%.2f up to %d), hub of %d at id %d"
      % (V, d_model, d, len(keys), nnz, nnz / len(keys), exponent, args.max_degree, args.hub, hub_key), file=sys.stderr)
print("# level schedule: %d levels (launches per sequential sweep), the largest of %d rows, the median of %d; %.2f s on the host"
      % (len(sizes), sizes.max(), int(np.median(sizes)), t_schedule), file=sys.stderr)

g = torch.Generator(device=dev).manual_seed(0)
Q_hat = torch.zeros(V, d, device=dev)
Q_hat[:, :d_model] = torch.randn(V, d_model, generator=g, device=dev)
rp, ci, listed = (torch.from_numpy(x).to(dev) for x in (row_ptr_h, col_h, rows_h))
lists = [listed[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]
alpha = args.alpha


def sequential():
    Q = Q_hat.clone()
    for _ in range(T):
        for rows in lists:
            hip.retrofit_rows(rp, ci, None, rows, Q_hat, Q, Q, alpha)
    return Q


def jacobi():
    Q, other = Q_hat.clone(), torch.empty_like(Q_hat)
    for _ in range(T):
        hip.retrofit_rows(rp, ci, None, None, Q_hat, Q, other, alpha)
        Q, other = other, Q
    return Q


# (a) the same Jacobi sweep from csr_spmm and torch: S = A Q; Q' = (alpha w Q^ + S) / (alpha w + w) on the rows with neighbours
ones = torch.ones(nnz, device=dev)
w = torch.from_numpy(np.diff(row_ptr_h).astype(np.float32)).to(dev)[:, None]
has = w > 0
den = torch.where(has, alpha * w + w, torch.ones_like(w))


def jacobi_spmm_torch():
    Q = Q_hat.clone()
    for _ in range(T):
        S = hip.csr_spmm(rp, ci, ones, V, V, Q)
        Q = torch.where(has, (alpha * w * Q_hat + S) / den, Q)
    return Q


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


J, Jt, S = jacobi(), jacobi_spmm_torch(), sequential()
torch.cuda.synchronize()
print("# Jacobi: largest difference between the one-launch sweep and csr_spmm + torch %.3g (largest entry %.3g)"
      % ((J - Jt).abs().max().item(), Jt.abs().max().item()), file=sys.stderr)
print("# sequential from Jacobi after %d sweeps: largest difference %.3g" % (T, (S - J).abs().max().item()), file=sys.stderr)
assert torch.equal(S, sequential()) and torch.equal(J, jacobi())           # bitwise repeatable
moved = int(len(rows_h))
gathered = nnz * d * 4
seq_bytes = gathered + 3 * moved * d * 4
jac_bytes = gathered + 3 * moved * d * 4 + 2 * (V - moved) * d * 4
lines = {
    "sequential (level schedule, in place), %d sweeps" % T: (sequential, T * seq_bytes),
    "jacobi (one launch per sweep), %d sweeps" % T: (jacobi, T * jac_bytes),
    "(a) jacobi from csr_spmm + torch, %d sweeps" % T: (jacobi_spmm_torch, None),
}
for fn, _ in lines.values():
    timed(fn, 1)                                            # (the warm-up)
times = {name: [] for name in lines}
for _ in range(args.rounds):
    for name, (fn, _) in lines.items():
        times[name].append(timed(fn, args.reps))
# the clone the three lines start with, timed alone and taken off
t_clone = statistics.median(timed(lambda: Q_hat.clone(), 10) for _ in range(args.rounds))
hub_ms = None
if args.hub:
    hub_list = torch.tensor([hub_key], dtype=torch.int32, device=dev)
    scratch = Q_hat.clone()
    timed(lambda: hip.retrofit_rows(rp, ci, None, hub_list, Q_hat, Q_hat, scratch, alpha), 3)
    hub_ms = statistics.median(timed(lambda: hip.retrofit_rows(rp, ci, None, hub_list, Q_hat, Q_hat, scratch, alpha), 20)
                               for _ in range(args.rounds))
print("| line | V | d | ms for %d sweeps, median (min - max), the starting copy of %.3f ms taken off | ms per sweep | bound: bytes at 6.29 TB/s, ms per sweep |" % (T, t_clone))
print("|---|---|---|---|---|---|")
for name, t in times.items():
    med = statistics.median(t) - t_clone
    nbytes = lines[name][1]
    print("| %s | %d | %d | %.3f (%.3f - %.3f) | %.3f | %s |" % (name, V, d, med, min(t) - t_clone, max(t) - t_clone, med / T,
                                                           "" if nbytes is None else "%.3f" % (nbytes / T / HBM_BYTES_PER_S * 1e3)))
if hub_ms is not None:
    seq_sweep = (statistics.median(times[list(lines)[0]]) - t_clone) / T
    jac_sweep = (statistics.median(times[list(lines)[1]]) - t_clone) / T
    print("| the hub row alone (one lane group, %d partner rows) | %d | %d | %.3f per call | %.0f %% of a sequential sweep, %.0f %% of a Jacobi sweep |  |"
          % (args.hub, V, d, hub_ms, 100 * hub_ms / seq_sweep, 100 * hub_ms / jac_sweep))

# the whole driver, host phases included (the schedule, upload, download): seconds per phase of the median run
W = Q_hat[:, :d_model].cpu().numpy()
for schedule in ("sequential", "jacobi"):
    runs = []
    for _ in range(4):
        t0 = time.perf_counter()
        out = retrofit_table(W, row_ptr_h, col_h, iterations=T, alpha=alpha, schedule=schedule, backend=hip)
        runs.append((time.perf_counter() - t0, out["seconds"]))
    runs = sorted(runs[1:], key=lambda r: r[0])              # (the first run is the warm-up)
    total, phases = runs[len(runs) // 2]
    print("| retrofit_table, %s, %d sweeps | %d | %d | %.1f (%.1f - %.1f) | %s |  |" % (
        schedule, T, V, d, total * 1e3, runs[0][0] * 1e3, runs[-1][0] * 1e3, ", ".join("%s %.1f" % (k, v * 1e3) for k, v in phases.items())))

# (b) Faruqui's loop in NumPy on the CPU: in place, key by key in vocabulary order, float32
if not args.no_cpu:
    Wc = W.copy()
    key_list = [(int(i), col_h[row_ptr_h[i]:row_ptr_h[i + 1]]) for i in keys]
    t0 = time.perf_counter()
    for _ in range(T):
        for i, nb in key_list:
            Wc[i] = (np.float32(alpha * len(nb)) * W[i] + Wc[nb].sum(axis=0)) / np.float32(alpha * len(nb) + len(nb))
    t_cpu = time.perf_counter() - t0
    err = np.abs(Wc - S[:, :d_model].cpu().numpy()).max()
    print("| (b) Faruqui's loop in NumPy on the CPU (one thread's worth of Python), %d sweeps | %d | %d | %.0f | %.0f | largest difference from the sequential schedule %.3g |"
          % (T, V, d_model, t_cpu * 1e3, t_cpu * 1e3 / T, err))
