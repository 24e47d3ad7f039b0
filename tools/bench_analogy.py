#!/usr/bin/env python3
"""Times the word-analogy top-k (glove_analogy_topk_f32): 1,024 questions at V = 400 k, d = 300 (row stride 320), k = 1.

The whole call is timed with device events around it (warm, mean of --reps calls).  One call is one enqueue of five or six
kernels, so no event can be put between them from outside: the shares of the similarity GEMM and of the selection come
from the kernels' device-side durations in a torch.profiler trace of a further call, taken in a pass of its own."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from trainer.hip_api import GloveHip, row_width  # noqa: E402

cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
cli.add_argument("--vocab", type=int, default=400_000)
cli.add_argument("--dim", type=int, default=300)
cli.add_argument("--questions", type=int, default=1024)
cli.add_argument("--top-k", type=int, default=1)
cli.add_argument("--reps", type=int, default=5)
args = cli.parse_args()

hip = GloveHip("cuda:0")
V, n, k = args.vocab, args.questions, args.top_k
d = row_width(V, args.dim)
g = torch.Generator(device="cpu").manual_seed(0)
W = torch.zeros(V, d)
W[:, :args.dim] = torch.randn(V, args.dim, generator=g)
W = W.to("cuda:0")
abc = torch.randint(0, V, (n, 3), generator=g, dtype=torch.int32).to("cuda:0")      # (a question may repeat a word)
hip.analogy_topk(W, abc, k, batch=n)            # warm: code objects, the allocator's blocks
torch.cuda.synchronize()
start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
start.record()
for _ in range(args.reps):
    hip.analogy_topk(W, abc, k, batch=n)
stop.record()
torch.cuda.synchronize()
ms = start.elapsed_time(stop) / args.reps
flops = 2.0 * n * V * d
print("V=%d d=%d (stride %d) n=%d k=%d: %.2f ms per call (%d calls, events; includes the workspace allocation), "
      "%.1f us per question, GEMM alone would be %.1f TFLOP/s at that time"
      % (V, args.dim, d, n, k, ms, args.reps, 1e3 * ms / n, flops / (ms * 1e-3) / 1e12))

from torch.profiler import ProfilerActivity, profile  # noqa: E402

with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
    hip.analogy_topk(W, abc, k, batch=n)
    torch.cuda.synchronize()
kernels = {}
for ev in prof.events():
    if "cuda" in str(ev.device_type).lower() and ev.name:
        for key in ("cosine_mfma", "topk_select", "analogy_query", "inv_norm"):
            if key in ev.name:
                kernels[key] = kernels.get(key, 0.0) + (ev.device_time if hasattr(ev, "device_time") else ev.cuda_time)
if not kernels:
    sys.exit("the profiler recorded none of the call's kernels: shares not measured")
total = sum(kernels.values())
print("device time of one call's kernels: %.2f ms; " % (total / 1e3)
      + ", ".join("%s %.2f ms (%.1f %%)" % (name, us / 1e3, 100 * us / total) for name, us in sorted(kernels.items(), key=lambda x: -x[1])))
