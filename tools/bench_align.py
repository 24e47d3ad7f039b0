#!/usr/bin/env python3
"""Times the calls of include/glove_factor_align_hip.h and include/glove_eval_cross_hip.h at the sizes trainer.align meets
(d = 300 in its row stride, 200 k anchors, 200 k candidates), beside torch on the same GPU in the same process: the
cross-covariance from Xa.double().T @ Ya.double() and from Xa.T @ Ya on gathered, scaled copies; one batch of 1,024
queries from torch.topk(Qn @ Tn.T [- penalties]); and the whole CSLS evaluation of 1,500 queries, end to end.

Every line is checked against its neighbour, warmed, then timed with device events around --reps calls, alternating,
--rounds times, a window of --window-ms at the least; the table shows each line's median round and its spread, and the
time its multiply-adds take at the measured f32 MFMA rate (155 TFLOP/s): a bound, not a target."""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from trainer.align import clamped_inv_norms, translation_precision  # noqa: E402
from trainer.hip_api import GloveHip, load_factor_library, row_width  # noqa: E402

MFMA_F32_FLOPS = 155e12

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--vocab", type=int, default=200000, help="rows of both tables: the candidates, --restrict-vocab")
cli.add_argument("--embedding-size", type=int, default=300)
cli.add_argument("--anchors", type=int, default=200000)
cli.add_argument("--batch", type=int, default=1024)
cli.add_argument("--queries", type=int, default=1500, help="queries of the end-to-end CSLS evaluation")
cli.add_argument("--knn", type=int, default=10)
cli.add_argument("--reps", type=int, default=3)
cli.add_argument("--window-ms", type=float, default=200.0)
cli.add_argument("--rounds", type=int, default=5)
cli.add_argument("--no-eval", action="store_true", help="leave the end-to-end evaluation out")
args = cli.parse_args()

dev = "cuda:0"
hip = GloveHip(dev)
V, d_model, n, B, k = args.vocab, args.embedding_size, args.anchors, args.batch, args.knn
d = row_width(V, d_model)
g = torch.Generator(device=dev).manual_seed(0)


def table():
    W = torch.zeros(V, d, device=dev)
    W[:, :d_model] = torch.randn(V, d_model, generator=g, device=dev) + 0.5 * torch.randn(d_model, generator=g, device=dev)
    return W


X, Y = table(), table()
xid = torch.randint(0, V, (n,), generator=g, device=dev, dtype=torch.int32)
yid = torch.randint(0, V, (n,), generator=g, device=dev, dtype=torch.int32)
xs, ys = clamped_inv_norms(X), clamped_inv_norms(Y)
ws = torch.empty(load_factor_library().glove_cross_gram_workspace_bytes(n, d), dtype=torch.uint8, device=dev)
qid = torch.randint(0, V, (B,), generator=g, device=dev, dtype=torch.int32)
q_pen, t_pen = hip.csls_penalty(X, qid, Y, k), torch.rand(V, generator=g, device=dev) * 0.2
print("# V = %d, d = %d (row stride %d), %d anchors, batch %d, knn %d; cross-gram workspace %.1f MB" % (V, d_model, d, n, B, k, ws.numel() / 1e6),
      file=sys.stderr)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


# the torch lines get what the library calls get (tables, ids, scales) and gather, scale and normalise inside the call
Xa, Ya = X[xid.long()] * xs[xid.long(), None], Y[yid.long()] * ys[yid.long(), None]


def torch_gram(dtype):
    a, b = X[xid.long()] * xs[xid.long(), None], Y[yid.long()] * ys[yid.long(), None]
    return a.to(dtype).T @ b.to(dtype)


def torch_topk(pens):
    Qn, Tn = X[qid.long()] * xs[qid.long(), None], Y * ys[:, None]
    s = Qn @ Tn.T
    if pens:
        s = 2.0 * s - q_pen[:, None] - t_pen[None, :]
    return torch.topk(s, k, dim=1)


lines = {
    "glove_cross_gram_f64, both scales": (lambda: hip.cross_gram(X, xid, Y, yid, xs, ys, ws), 2 * n * d * d),
    "glove_cross_gram_f64, null scales": (lambda: hip.cross_gram(X, xid, Y, yid, None, None, ws), 2 * n * d * d),
    "torch: gather, scale, Xa.double().T @ Ya.double()": (lambda: torch_gram(torch.float64), 2 * n * d * d),
    "torch: Xa.double().T @ Ya.double() on gathered copies": (lambda: Xa.double().T @ Ya.double(), 2 * n * d * d),
    "torch: Xa.T @ Ya (float32) on gathered copies": (lambda: Xa.T @ Ya, 2 * n * d * d),
    "cross_topk, %d queries, k = %d, cosine" % (B, k): (lambda: hip.cross_topk(X, qid, Y, k, batch=B), 2 * B * V * d),
    "cross_topk, %d queries, k = %d, CSLS" % (B, k): (lambda: hip.cross_topk(X, qid, Y, k, q_pen, t_pen, batch=B), 2 * B * V * d),
    "torch: topk(Qn @ Tn.T), normalising inside": (lambda: torch_topk(False), 2 * B * V * d),
    "torch: topk(2 Qn @ Tn.T - penalties), normalising inside": (lambda: torch_topk(True), 2 * B * V * d),
}
M, M64, M32 = hip.cross_gram(X, xid, Y, yid, xs, ys, ws), Xa.double().T @ Ya.double(), (Xa.T @ Ya).double()
torch.cuda.synchronize()
top = M64.abs().max().item()
e_ours, e_f32 = (M - M64).abs().max().item() / top, (M32 - M64).abs().max().item() / top
print("# cross-covariance, largest difference from torch float64 over the largest entry: ours %.3g, torch float32 %.3g (ratio %.1f)"
      % (e_ours, e_f32, e_f32 / max(e_ours, 1e-300)), file=sys.stderr)
for pens in (False, True):
    ours = hip.cross_topk(X, qid, Y, k, *((q_pen, t_pen) if pens else (None, None)), batch=B)
    theirs = torch_topk(pens)
    print("# top-%d %s: largest score difference from torch %.3g, ids equal at %.4f of the positions"
          % (k, "CSLS" if pens else "cosine", (ours[0] - theirs.values).abs().max().item(),
             (ours[1].long() == theirs.indices).float().mean().item()), file=sys.stderr)
assert torch.equal(M, hip.cross_gram(X, xid, Y, yid, xs, ys, ws))
del M, M64, M32
reps = {name: max(args.reps, int(args.window_ms / timed(fn, 2)) + 1) for name, (fn, _) in lines.items()}       # (also the warm-up)
times = {name: [] for name in lines}
for _ in range(args.rounds):
    for name, (fn, _) in lines.items():
        times[name].append(timed(fn, reps[name]))
print("| call | rows | d | ms per call, median (min - max) | bound: flops at 155 TF, ms |")
print("|---|---|---|---|---|")
for name, t in times.items():
    rows = n if "gram" in name or "Xa" in name else V
    print("| %s | %d | %d | %.3f (%.3f - %.3f) | %.3f |" % (name, rows, d, statistics.median(t), min(t), max(t),
                                                            lines[name][1] / MFMA_F32_FLOPS * 1e3))

if not args.no_eval:
    # the whole CSLS evaluation: both penalties (the target side's is V queries against V rows) and the scoring, host phases included
    A, T = X[:, :d_model].cpu().numpy(), Y[:, :d_model].cpu().numpy()
    src = np.random.default_rng(0).choice(V, args.queries, replace=False)
    pairs = np.stack([src, np.random.default_rng(1).integers(0, V, args.queries)], axis=1)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = translation_precision(A, T, pairs, method="csls", knn=k, top_k=(1, 5, 10), backend=hip, batch=B)
        runs.append((time.perf_counter() - t0, out["seconds"]))
    runs = sorted(runs[1:], key=lambda r: r[0])                  # (the first run is the warm-up)
    total, phases = runs[0]
    print("| translation_precision, CSLS, %d queries, knn %d | %d | %d | %.0f (of 2 runs: %.0f, %.0f) | %s |" % (
        args.queries, k, V, d, total * 1e3, runs[0][0] * 1e3, runs[-1][0] * 1e3,
        ", ".join("%s %.0f" % (kk, v * 1e3) for kk, v in phases.items())))
