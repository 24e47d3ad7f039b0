"""Generates tests/golden/eval_kernel_bits.json: the exact bits the evaluation kernels put out (PREDICT top-k, 3CosAdd,
3CosMul, the pair cosine, k-means assign and update) on seeded inputs, as digests.

    python tests/golden/make_eval_bits.py [--lib-dir DIR] [--out FILE]       # needs the GPU

The parity tests of these kernels compare with float64 at rtol 1e-5 and would not see a changed summation order; this
file pins it.  Per case and output tensor it holds the SHA-256 of the raw bytes, the shape and the first four values as
hex (for a first look at a mismatch), and beside the cases what `hipcc --version` says.  --lib-dir: where libglove_hip.so
and libglove_eval_hip.so are taken from (default: the tree's own lib/), so that the file can be recorded from a build of
the commit BEFORE a change to the kernels.  tests/test_gpu_eval_bits.py recomputes CASES on the tree under test and
asserts equal digests: the file is regenerated only when the bits are meant to change.

The cases are the smallest shapes that cross every edge of the GEMMs' tile loop (csrc/glove_sim_gemm.h): V = 300 is
three vocabulary tiles of 128, the last partial; d = 8 is below one slab of 32 columns, 52 one slab and a partial one,
300 the workload's width (row shape 32 x 3), 1024 the widest; n = 130 is two query tiles (three of 3CosMul's); the
k-means case with K = 129 crosses a centroid tile.  The k-means inputs are those of tests/test_gpu_kmeans.py:case.
kmeans_update runs on the assignments of two of the k-means cases after two changes that make it take every path:
the members of the last cluster go to cluster 0 (an empty cluster keeps its old row), and so do the first 100 points —
the assignments themselves hold no cluster of more than 64 members (42 and 55 at the most), and only such a cluster
is summed in two levels.  The generator asserts both."""
import argparse
import hashlib
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
OUT = HERE / "eval_kernel_bits.json"
DEV = "cuda:0"
V, WIDTHS, K_TOP = 300, (8, 52, 300, 1024), 9
KMEANS = ((300, 8, 300, 1), (300, 8, 257, 2), (1000, 52, 777, 33), (5000, 64, 5000, 129), (600, 1024, 130, 31))
KMEANS_UPDATE = (KMEANS[2], KMEANS[3])


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def table(d):
    """(W [V,d], rng): the rng goes on to draw the case's ids."""
    rng = np.random.default_rng(7000 + d)
    return rng.standard_normal((V, d)).astype(np.float32), rng


def kmeans_inputs(V, d, n, K):
    rng = np.random.default_rng(3000 + V + d + K)
    W = rng.standard_normal((V, d)).astype(np.float32)
    ids = (rng.permutation(V) if n == V else rng.integers(0, V, n)).astype(np.int32)
    C = (W[rng.choice(V, K, replace=False)] + 0.5 * rng.standard_normal((K, d))).astype(np.float32)
    return _dev(W, ids, C)


def topk_cosine(hip, d, n):
    W, rng = table(d)
    W, q = _dev(W, rng.integers(0, V, n).astype(np.int32))
    return dict(zip(("sims", "idx"), hip.topk_cosine(W, q, K_TOP)))


def analogy(hip, d, cosmul):
    W, rng = table(d)
    W, abc = _dev(W, rng.integers(0, V, (130, 3)).astype(np.int32))
    out = hip.analogy_cosmul_topk(W, abc, K_TOP, eps=1e-3) if cosmul else hip.analogy_topk(W, abc, K_TOP)
    return dict(zip(("sims", "idx"), out))


def pair_cosine(hip, d):
    W, rng = table(d)
    W, pairs = _dev(W, rng.integers(0, V, (517, 2)).astype(np.int32))
    return {"cos": hip.pair_cosine(W, pairs)}


def kmeans_assign(hip, shape):
    W, ids, C = kmeans_inputs(*shape)
    return dict(zip(("assign", "cos"), hip.kmeans_assign(W, ids, C)))


def kmeans_update(hip, shape):
    W, ids, C = kmeans_inputs(*shape)
    K = shape[3]
    assign = hip.kmeans_assign(W, ids, C)[0].clone()
    assign[assign == K - 1] = 0
    assign[:100] = 0
    cents, counts = hip.kmeans_update(W, ids, assign, C)
    assert int(counts.max()) > 64 and int(counts[K - 1]) == 0, counts
    return {"centroids": cents, "counts": counts}


def _cases():
    cases = {}
    for d in WIDTHS:
        for n in (5, 130):
            cases["topk_cosine/d%d/n%d" % (d, n)] = lambda hip, d=d, n=n: topk_cosine(hip, d, n)
        cases["analogy_topk/d%d" % d] = lambda hip, d=d: analogy(hip, d, False)
        cases["analogy_cosmul_topk/d%d" % d] = lambda hip, d=d: analogy(hip, d, True)
        cases["pair_cosine/d%d" % d] = lambda hip, d=d: pair_cosine(hip, d)
    for shape in KMEANS:
        cases["kmeans_assign/V%d_d%d_n%d_K%d" % shape] = lambda hip, shape=shape: kmeans_assign(hip, shape)
    for shape in KMEANS_UPDATE:
        cases["kmeans_update/V%d_d%d_n%d_K%d" % shape] = lambda hip, shape=shape: kmeans_update(hip, shape)
    return cases


CASES = _cases()           # name -> f(GloveHip) -> {output name: tensor}


def digest(t) -> dict:
    a = t.detach().cpu().contiguous().numpy()
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "shape": list(a.shape), "dtype": str(a.dtype),
            "head": [x.tobytes().hex() for x in a.reshape(-1)[:4]]}


def run_case(hip, name) -> dict:
    return {out: digest(t) for out, t in CASES[name](hip).items()}


def main():
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    cli.add_argument("--lib-dir", type=Path, default=None, help="libglove_hip.so and libglove_eval_hip.so of another build")
    cli.add_argument("--out", type=Path, default=OUT)
    args = cli.parse_args()
    sys.path[:0] = [p for p in (str(REPO),) if p not in sys.path]
    from trainer import hip_api
    if args.lib_dir:
        hip = hip_api.GloveHip(DEV, lib_path=args.lib_dir / "libglove_hip.so")
        hip_api._eval_lib = hip_api.load_eval_library(args.lib_dir / "libglove_eval_hip.so")   # what the methods will find loaded
    else:
        hip = hip_api.GloveHip(DEV)
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    except (OSError, subprocess.CalledProcessError):
        hipcc = ["unknown"]
    doc = {"hipcc": hipcc, "cases": {name: run_case(hip, name) for name in CASES}}
    args.out.write_text(json.dumps(doc, indent=1, sort_keys=True) + "\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
