"""`python tools/vectors_timing.py [--rows 400000] [--d 300] [--precision 6] [--block-rows 65536] [--block-bytes 64Mi]
[--host-rows N] [--repeats 3] [--out DIR]`

Times trainer.vectors on an MI355X on a synthetic table (seeded standard normals, words w0 w1 ...): export and import end to
end, file I/O included (a host clock around work that ends in a device synchronise), and the kernels alone (device events
around the enqueues of glove_vectors_format_f32, and of glove_vectors_lines_u8 + glove_vectors_parse_f32, on resident blocks,
after a warm-up pass, `repeats` times: the median and the spread are printed).  Beside them the host path on the same box:
the same file written with "%.*f" % and read with float(), the way a Python tool without this library does it
(--host-rows: on the first N rows only, where the whole table would take too long; the figure then says so).  The two files
and the two tables are compared: bytes and bits.  Prints one JSON line; needs a GPU (no fallback)."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def host_write(path, words, W, p):
    with open(path, "wb") as f:
        for w, row in zip(words, W):
            f.write((w + "".join(" %.*f" % (p, x) for x in row.tolist()) + "\n").encode())


def host_read(path):
    words, rows = [], []
    with open(path, "rb") as f:
        for line in f:
            fields = line.split()
            words.append(fields[0].decode())
            rows.append(np.array([float(t) for t in fields[1:]], np.float32))
    return words, np.stack(rows)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def note(text):
    print(text, file=sys.stderr, flush=True)


def summary(ms):
    return {"median_s": statistics.median(ms) / 1e3, "min_s": min(ms) / 1e3, "max_s": max(ms) / 1e3, "repeats": len(ms)}


def main(argv=None):
    from trainer import vectors
    from trainer.hip_api import GloveHip
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    cli.add_argument("--rows", type=int, default=400000)
    cli.add_argument("--d", type=int, default=300)
    cli.add_argument("--precision", type=int, default=6)
    cli.add_argument("--block-rows", type=int, default=65536)
    cli.add_argument("--block-bytes", default="64Mi")
    cli.add_argument("--host-rows", type=int, default=None)
    cli.add_argument("--repeats", type=int, default=3)
    cli.add_argument("--out", default=None, help="directory for the files (default: a temporary one)")
    args = cli.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("vectors_timing needs cuda:0 (no CPU fallback)")
    hip, dev = GloveHip("cuda:0"), torch.device("cuda:0")
    V, d, p = args.rows, args.d, args.precision
    W = np.random.default_rng(0).standard_normal((V, d), dtype=np.float32)
    words = ["w%d" % i for i in range(V)]
    out = {"rows": V, "d": d, "precision": p, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory(dir=args.out) as tmp:
        path, host_path = Path(tmp, "device.txt"), Path(tmp, "host.txt")
        vectors.export_vectors(words[:1000], W[:1000], path, "glove", p, args.block_rows, hip)         # warm-up: code objects, allocator
        vectors.import_vectors(path, "text", vectors.byte_count(args.block_bytes), hip)
        note("warmed up")
        # ---- end to end on the device backend
        torch.cuda.synchronize()
        t = time.perf_counter()
        exported = vectors.export_vectors(words, W, path, "glove", p, args.block_rows, hip)
        torch.cuda.synchronize()
        out["export_end_to_end_s"] = time.perf_counter() - t
        out["export_phases_s"], out["file_bytes"] = exported["seconds"], exported["bytes"]
        t = time.perf_counter()
        imported = vectors.import_vectors(path, "text", vectors.byte_count(args.block_bytes), hip)
        torch.cuda.synchronize()
        out["import_end_to_end_s"] = time.perf_counter() - t
        out["import_phases_s"], out["fallback_tokens"] = imported["seconds"], imported["fallback_tokens"]
        note("end to end: export %.2f s, import %.2f s" % (out["export_end_to_end_s"], out["import_end_to_end_s"]))
        # ---- the kernels alone, on resident blocks
        encoded = [w.encode() for w in words]
        blocks = []
        for r0 in range(0, V, args.block_rows):
            enc = encoded[r0:r0 + args.block_rows]
            off = np.zeros(len(enc) + 1, np.int64)
            np.cumsum([len(e) for e in enc], out=off[1:])
            n = len(enc)
            blocks.append((torch.from_numpy(W[r0:r0 + n]).to(dev), torch.from_numpy(np.frombuffer(b"".join(enc), np.uint8).copy()).to(dev),
                           torch.from_numpy(off).to(dev), torch.empty(int(off[-1]) + n * (d * (p + 13) + 1), dtype=torch.uint8, device=dev),
                           torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)))
        sizes = torch.zeros(2, dtype=torch.int64, device=dev)

        def format_all():
            for Wb, wb, off, text, row_off, host_row in blocks:
                hip.vectors_format_enqueue(Wb, d, p, wb, off, text, row_off, host_row, sizes)
        format_all()
        out["format_kernels"] = summary([event_ms(format_all) for _ in range(args.repeats)])
        del blocks
        texts = []
        with open(path, "rb") as f:
            for block in vectors.iter_line_blocks(f, vectors.byte_count(args.block_bytes)):
                blk = torch.from_numpy(np.frombuffer(block, np.uint8).copy()).to(dev)
                cap = block.count(b"\n") + 1
                texts.append((blk, torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                              torch.empty((cap, (d + 3) // 4 * 4), dtype=torch.float32, device=dev),
                              torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(4096, dtype=torch.int64, device=dev),
                              torch.empty(4096, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)))

        def parse_all():
            for blk, start, fields, vec, word_len, fb_index, fb_span, n in texts:
                hip.vectors_lines_enqueue(blk, start, fields, n[0:2])
                hip.vectors_parse_enqueue(blk, start, n[0:1], d, vec, word_len, fb_index, fb_span, n[2:4])
        parse_all()
        out["parse_kernels"] = summary([event_ms(parse_all) for _ in range(args.repeats)])
        del texts
        note("kernels: format %s, parse %s" % (out["format_kernels"], out["parse_kernels"]))
        # ---- the host path: % and float()
        H = V if args.host_rows is None else min(args.host_rows, V)
        out["host_rows"] = H
        t = time.perf_counter()
        host_write(host_path, words[:H], W[:H], p)
        out["host_export_end_to_end_s"] = time.perf_counter() - t
        note("host export %.1f s" % out["host_export_end_to_end_s"])
        t = time.perf_counter()
        host_words, host_W = host_read(host_path)
        out["host_import_end_to_end_s"] = time.perf_counter() - t
        # ---- the same bytes, the same bits
        with open(path, "rb") as f:
            out["files_equal"] = f.read(host_path.stat().st_size) == host_path.read_bytes() and (H < V or f.read(1) == b"")
        R = imported["R"]
        out["tables_equal"] = bool(imported["words"][1:H + 1] == host_words
                                   and np.array_equal(R[1:H + 1].view(np.uint32), host_W.view(np.uint32)))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
