"""`python -m trainer.vectors export --job-dir J --output F [--embeddings row|col|sum] [--format glove|word2vec|word2vec-bin]
[--precision 6] [--block-rows N]`
`python -m trainer.vectors import --vectors F --job-dir J [--format auto|text|word2vec-bin] [--optimizer NAME] [--block-bytes N]`

The file every other tool exchanges word vectors in — `word v1 ... vd` per line: GloVe's own vectors.txt, word2vec and
fastText .vec (the same lines behind a `V d` header), gensim's load_word2vec_format, spaCy — written from and read into a
job directory.  The reference has neither direction.  The text runs block by block through the GPU
(include/glove_vectors_hip.h): a value is written as "%.*f" % (precision, x) and read as np.float32(float(token)), both bit
for bit.

export writes the newest checkpoint of J in vocabulary order, "<UNK>" left out as in trainer.export_embeddings.  `glove` is
the plain lines (GloVe writes %lf: precision 6), `word2vec` puts the `V d` header in front, `word2vec-bin` is the header and
then `word` + a space + d little-endian float32 + a newline per word: written on the host from the table's bytes, lossless.

import writes a job directory at step 0 the way trainer.svd does: params.json, vocab.txt, `model.ckpt-0` (R = the vectors,
C = 0, zero biases, the optimizer's slots at their initial values: --embeddings row and sum both score the file) and
vectors.json (source, format, d, records, duplicates dropped, fallback tokens, seconds per phase).  trainer.analogy,
trainer.wordsim, trainer.categorize, trainer.classes and trainer.export_embeddings open it unchanged.  Continuing TRAINING
from an imported directory is not supported: a file holds one table, and a GloVe model is two tables and two biases.
Row 0 is "<UNK>": the file's own "<UNK>" record if it has one, else zeros; the file's words follow in file order; a
repeated word keeps its first record.  Format `auto`: a first line of exactly two integer fields is a word2vec header;
behind such a header the file is binary when its next line does not read as text; a binary file without one needs the flag.
The separators are the bytes 20, 0A and 0D only (words of glove.840B.300d contain tabs and no-break spaces); d is the first
record's field count minus one and any record with another count is an error that names its line, as is a word that is not
UTF-8 and a number float() refuses.  --job-dir is used as given: no date suffix.

Both directions are backend-neutral like trainer.svd: `backend` has three operations on torch tensors that live on
`backend.device` (GloveHip is the product one; the tests bring a NumPy one):
    vectors_lines(block u8 [n]) -> (line_start i32 [m], line_fields i32 [m])
    vectors_parse(block, line_start, d) -> (vec f32 [m, ld], word_len i32 [m], fb_index i64 [k] ascending, fb_span i64 [k])
    vectors_format(W f32 [n, ld], d, precision, word_bytes u8, word_off i64 [n + 1], cap_out) -> (out u8, row_off i64 [n + 1], host_row u8 [n])
"""
from __future__ import annotations

import argparse
import json
import logging
import re
import time
from pathlib import Path

import numpy as np
import torch

from trainer import config

logger = logging.getLogger(__name__)

SKIPPED_TOKEN = "<UNK>"
EXPORT_FORMATS = ("glove", "word2vec", "word2vec-bin")
IMPORT_FORMATS = ("auto", "text", "word2vec-bin")
EMBEDDINGS = ("row", "col", "sum")
MAX_BLOCK_BYTES = 2 ** 31 - 1
FIELD = re.compile(rb"[^ \n\r]+")
SIZES = {"Ki": 1 << 10, "Mi": 1 << 20, "Gi": 1 << 30}


def byte_count(text: str) -> int:
    """`64Mi`, `1Gi`, `4096`."""
    text = str(text)
    for suffix, unit in SIZES.items():
        if text.endswith(suffix):
            return int(text[:-2]) * unit
    return int(text)


def _backend(backend):
    if backend is None:
        from trainer.hip_api import GloveHip
        backend = GloveHip("cuda:0")
    return backend, torch.device(getattr(backend, "device", "cpu"))


class _Phases:
    """Seconds per phase; a phase ends when the device has finished it."""

    def __init__(self, device):
        self.device, self.seconds, self._t = device, {}, time.perf_counter()

    def done(self, name: str):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.seconds[name] = self.seconds.get(name, 0.0) + now - self._t
        self._t = now


# ---- export
def _percent(x, precision: int) -> str:
    return "%.*f" % (precision, float(x))


def format_block(words, W: np.ndarray, precision: int, backend, dev) -> bytes:
    """The lines of the rows W [n, d] (float32) with their words: the backend's text, the rows it left to the host spliced in."""
    n, d = W.shape
    encoded = [w.encode("utf8") for w in words]
    word_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(e) for e in encoded], out=word_off[1:])
    word_bytes = np.frombuffer(b"".join(encoded) or b"\0", np.uint8).copy()
    cap_out = int(word_off[-1]) + n * (d * (precision + 13) + 1)
    out, row_off, host_row = backend.vectors_format(
        torch.from_numpy(np.ascontiguousarray(W, np.float32)).to(dev), d, precision, torch.from_numpy(word_bytes).to(dev),
        torch.from_numpy(word_off).to(dev), cap_out)
    text = out.cpu().numpy().tobytes()
    host_rows = np.flatnonzero(host_row.cpu().numpy())
    if not len(host_rows):
        return text
    row_off = row_off.cpu().numpy()
    pieces, pos = [], 0
    for r in host_rows.tolist():            # a NaN, an infinity or |x| >= 2^31 in the row: Python's % writes it
        pieces.append(text[pos:int(row_off[r])])
        pieces.append(encoded[r] + "".join(" " + _percent(x, precision) for x in W[r]).encode() + b"\n")
        pos = int(row_off[r])
    pieces.append(text[pos:])
    return b"".join(pieces)


def export_vectors(words, W, output, fmt: str = "glove", precision: int = 6, block_rows: int = 65536, backend=None) -> dict:
    """Writes the rows of W [n, d] with their words to `output`; returns the bytes written and the seconds per phase."""
    if fmt not in EXPORT_FORMATS:
        raise ValueError("--format must be one of %s, got %r" % (", ".join(EXPORT_FORMATS), fmt))
    if not 0 <= int(precision) <= 9:
        raise ValueError("--precision must lie in [0, 9], got %r" % (precision,))
    if block_rows < 1:
        raise ValueError("--block-rows must be positive, got %r" % (block_rows,))
    W = np.ascontiguousarray(W, np.float32)
    n, d = W.shape
    if len(words) != n:
        raise ValueError("%d words for %d rows" % (len(words), n))
    for w in words:
        if not w or FIELD.fullmatch(w.encode("utf8")) is None:
            raise ValueError("the word %r is empty or holds a space or a line break: its line could not be read back" % w)
    target = Path(output)
    target.parent.mkdir(parents=True, exist_ok=True)
    size = 0
    with open(target, "wb") as f:
        if fmt != "glove":
            size += f.write(b"%d %d\n" % (n, d))
        if fmt == "word2vec-bin":
            phases = _Phases(torch.device("cpu"))
            raw = W.astype("<f4", copy=False)
            for w, row in zip(words, raw):
                size += f.write(w.encode("utf8") + b" " + row.tobytes() + b"\n")
            phases.done("write")
        else:
            backend, dev = _backend(backend)
            phases = _Phases(dev)
            for r0 in range(0, n, block_rows):
                text = format_block(words[r0:r0 + block_rows], W[r0:r0 + block_rows], int(precision), backend, dev)
                phases.done("format")
                size += f.write(text)
                phases.done("write")
    return {"bytes": size, "rows": n, "d": d, "seconds": phases.seconds}


def export_main(args, backend=None) -> dict:
    from trainer.data_utils import read_vocab
    from trainer.train_utils import CheckpointManager
    if args.embeddings not in EMBEDDINGS:
        raise ValueError("--embeddings must be one of %s, got %r" % (", ".join(EMBEDDINGS), args.embeddings))
    params = json.loads(Path(args.job_dir, "params.json").read_text())
    latest = CheckpointManager(params["job_dir"]).latest()
    if latest is None:
        raise ValueError("%s holds no checkpoint" % params["job_dir"])
    tables = torch.load(latest, map_location="cpu", weights_only=False)["tables"]
    W = {"row": lambda: tables["R"], "col": lambda: tables["C"], "sum": lambda: tables["R"] + tables["C"]}[args.embeddings]()
    vocab = read_vocab(params["vocab_txt"])
    if len(vocab) != W.shape[0]:
        raise ValueError("%d vocabulary lines for a table of %d rows" % (len(vocab), W.shape[0]))
    keep = [i for i, w in enumerate(vocab) if w != SKIPPED_TOKEN]
    out = export_vectors([vocab[i] for i in keep], W.float().numpy()[keep], args.output, args.format, args.precision,
                         args.block_rows, backend)
    logger.info("%d x %d vectors (%s, %s) of %s -> %s, %d bytes", out["rows"], out["d"], args.embeddings, args.format, latest,
                args.output, out["bytes"])
    return out


# ---- import
def _header(line: bytes):
    """(V, d) where the line is a word2vec header: exactly two integer fields."""
    fields = FIELD.findall(line)
    if len(fields) == 2 and all(f.isdigit() for f in fields):
        return int(fields[0]), int(fields[1])
    return None


def _reads_as_text(line: bytes, d: int) -> bool:
    fields = FIELD.findall(line)
    if len(fields) != d + 1:
        return False
    try:
        fields[0].decode("utf8")
        for f in fields[1:]:
            float(f)
    except ValueError:
        return False
    return True


def sniff(path, fmt: str = "auto"):
    """(format: text or word2vec-bin, header (V, d) or None, bytes of the header line)."""
    if fmt not in IMPORT_FORMATS:
        raise ValueError("--format must be one of %s, got %r" % (", ".join(IMPORT_FORMATS), fmt))
    with open(path, "rb") as f:
        first = f.readline(1 << 20)
        header = _header(first) if first.endswith(b"\n") else None
        if fmt == "word2vec-bin":
            if header is None:
                raise ValueError("%s line 1: a word2vec binary file starts with a line of two integers" % path)
            return fmt, header, len(first)
        if header is None:
            return "text", None, 0
        if fmt == "auto" and header[0] > 0:
            nxt = f.readline(max(1 << 20, 64 * header[1]))
            if not _reads_as_text(nxt, header[1]):
                return "word2vec-bin", header, len(first)
        return "text", header, len(first)


def iter_line_blocks(f, block_bytes: int):
    """The rest of the open file in blocks of about block_bytes that end behind a 0A (the last one may not); a line longer
    than that makes a longer block, and one that does not fit 2^31 - 1 bytes is an error."""
    block_bytes = max(1, min(int(block_bytes), MAX_BLOCK_BYTES))
    carry = b""
    while True:
        chunk = f.read(max(block_bytes - len(carry), min(block_bytes, 1 << 16)))
        if not chunk:
            if carry:
                yield carry
            return
        buf = carry + chunk if carry else chunk
        if len(buf) > MAX_BLOCK_BYTES:
            raise ValueError("a line is longer than 2^31 - 1 bytes")
        cut = buf.rfind(b"\n") + 1
        if cut == 0:
            carry = buf
            continue
        yield buf[:cut] if cut < len(buf) else buf
        carry = buf[cut:]


class _Vocabulary:
    """Row 0 is "<UNK>"; the file's words follow in file order; a repeated word keeps its first record."""

    def __init__(self):
        self.words, self.seen, self.unk, self.duplicates, self.kept = [SKIPPED_TOKEN], {SKIPPED_TOKEN}, None, 0, []

    def add(self, words, vec: np.ndarray):
        keep = []
        for r, w in enumerate(words):
            if w == SKIPPED_TOKEN and self.unk is None:
                self.unk = vec[r].copy()
            elif w in self.seen:
                self.duplicates += 1
            else:
                self.seen.add(w)
                self.words.append(w)
                keep.append(r)
        self.kept.append(vec[keep] if len(keep) != len(words) else vec)

    def table(self, d: int) -> np.ndarray:
        head = np.zeros((1, d), np.float32) if self.unk is None else self.unk.reshape(1, d)
        return np.ascontiguousarray(np.concatenate([head] + [k.reshape(-1, d) for k in self.kept]), np.float32)


def _read_text(path, skip: int, header, block_bytes: int, backend, vocab: _Vocabulary) -> dict:
    backend, dev = _backend(backend)
    phases = _Phases(dev)
    d, records, fallbacks = (header[1] if header else None), 0, 0
    lines_before = 1 if skip else 0                    # 0A bytes in front of the block
    with open(path, "rb") as f:
        f.seek(skip)
        for block in iter_line_blocks(f, block_bytes):
            def line_of(offset):
                return lines_before + block.count(b"\n", 0, int(offset)) + 1
            phases.done("read")
            dev_block = torch.from_numpy(np.frombuffer(block, np.uint8).copy()).to(dev)
            line_start, line_fields = backend.vectors_lines(dev_block)
            starts, fields = line_start.cpu().numpy(), line_fields.cpu().numpy()
            phases.done("records")
            if len(starts):
                if d is None:
                    d = int(fields[0]) - 1
                    if d < 1:
                        raise ValueError("%s line %d: a word and no numbers" % (path, line_of(starts[0])))
                bad = np.flatnonzero(fields != d + 1)
                if len(bad):
                    raise ValueError("%s line %d: expected %d fields (a word and %d numbers), got %d"
                                     % (path, line_of(starts[bad[0]]), d + 1, d, fields[bad[0]]))
                vec, word_len, fb_index, fb_span = backend.vectors_parse(dev_block, line_start, d)
                vec, lens = vec.cpu().numpy(), word_len.cpu().numpy()
                phases.done("numbers")
                ld = vec.shape[1]
                with np.errstate(over="ignore"):
                    for index, span in zip(fb_index.cpu().tolist(), fb_span.cpu().tolist()):
                        token = FIELD.match(block, span >> 16).group()          # (a span holds the first 65535 bytes' length at most)
                        try:
                            vec[index // ld, index % ld] = np.float32(float(token))
                        except ValueError:
                            raise ValueError("%s line %d: %r is no number" % (path, line_of(span >> 16), token[:40])) from None
                fallbacks += len(fb_index)
                words = []
                for s, n in zip(starts.tolist(), lens.tolist()):
                    try:
                        words.append(block[s:s + n].decode("utf8"))
                    except UnicodeDecodeError:
                        raise ValueError("%s line %d: the word %r is not UTF-8" % (path, line_of(s), block[s:s + n][:40])) from None
                vocab.add(words, vec[:, :d])
                records += len(starts)
                phases.done("words")
            lines_before += block.count(b"\n")
    if d is None:
        raise ValueError("%s holds no record" % path)
    return {"d": d, "records": records, "fallback_tokens": fallbacks, "seconds": phases.seconds}


def _read_word2vec_bin(path, skip: int, header, vocab: _Vocabulary) -> dict:
    phases = _Phases(torch.device("cpu"))
    V, d = header
    if d < 1:
        raise ValueError("%s line 1: the header names %d columns" % (path, d))
    data = Path(path).read_bytes()
    phases.done("read")
    pos, words, rows = skip, [], np.empty((V, d), np.float32)
    for r in range(V):
        while data[pos:pos + 1] in (b"\n", b"\r"):        # (the newline behind the record before)
            pos += 1
        sp = data.find(b" ", pos)
        if sp < 0 or sp + 1 + 4 * d > len(data):
            raise ValueError("%s: record %d of %d is cut short" % (path, r + 1, V))
        try:
            words.append(data[pos:sp].decode("utf8"))
        except UnicodeDecodeError:
            raise ValueError("%s record %d: the word %r is not UTF-8" % (path, r + 1, data[pos:sp][:40])) from None
        rows[r] = np.frombuffer(data, "<f4", d, sp + 1)
        pos = sp + 1 + 4 * d
    vocab.add(words, rows)
    phases.done("words")
    return {"d": d, "records": V, "fallback_tokens": 0, "seconds": phases.seconds}


def import_vectors(path, fmt: str = "auto", block_bytes: int = 64 << 20, backend=None) -> dict:
    """Reads a vector file: {"words": ["<UNK>", the file's words ...], "R": float32 [V, d], "format", "d", "records",
    "duplicates", "unk_in_file", "fallback_tokens", "seconds"}."""
    fmt, header, skip = sniff(path, fmt)
    vocab = _Vocabulary()
    if fmt == "word2vec-bin":
        out = _read_word2vec_bin(path, skip, header, vocab)
    else:
        out = _read_text(path, skip, header, block_bytes, backend, vocab)
    if header is not None and (header[1] != out["d"] or header[0] != out["records"]):
        raise ValueError("%s: the header names %d x %d, the file holds %d records of %d numbers"
                         % (path, header[0], header[1], out["records"], out["d"]))
    return dict(out, words=vocab.words, R=vocab.table(out["d"]), format="word2vec" if fmt == "text" and header else fmt,
                duplicates=vocab.duplicates, unk_in_file=vocab.unk is not None)


def import_main(args, backend=None) -> dict:
    from trainer.config_utils import build_parser, init_params
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager, get_optimizer
    optimizer = get_optimizer(args.optimizer)["class_name"]
    out = import_vectors(args.vectors, args.format, byte_count(args.block_bytes), backend)
    t0 = time.perf_counter()
    job = Path(args.job_dir)
    job.mkdir(parents=True, exist_ok=True)
    vocab_txt = job / "vocab.txt"
    vocab_txt.write_bytes("\n".join(out["words"]).encode("utf8"))
    V, d = out["R"].shape
    # params.json the way trainer.estimator builds it: its parser's defaults under the flags the two commands share
    params = vars(build_parser().parse_args([
        "--vocab-txt", str(vocab_txt), "--job-dir", str(job), "--disable-datetime-path", "--embedding-size", str(d),
        "--optimizer", args.optimizer])).copy()
    params = init_params(params)
    tables = DeviceTables(V, d, optimizer, device="cpu", seed=0)           # slots and scalars at step 0
    tables.embeddings("R").copy_(torch.from_numpy(out["R"]))
    tables.embeddings("C").zero_()
    tables.br.zero_()
    tables.bc.zero_()
    record = {"source": str(args.vectors), "format": out["format"], "d": d, "vocab_size": V, "records": out["records"],
              "duplicates_dropped": out["duplicates"], "unk_in_file": out["unk_in_file"], "fallback_tokens": out["fallback_tokens"],
              "optimizer": optimizer}
    CheckpointManager(params["job_dir"]).save(tables, extra={"vectors": record})
    seconds = dict(out["seconds"], write_job_dir=time.perf_counter() - t0)
    Path(params["job_dir"], "vectors.json").write_text(json.dumps(dict(record, seconds=seconds), indent=2))
    logger.info("%d records of %d numbers (%s; %d duplicates dropped, %d fallback tokens) of %s -> %s", out["records"], d,
                out["format"], out["duplicates"], out["fallback_tokens"], args.vectors, params["job_dir"])
    return out


def build_cli() -> argparse.ArgumentParser:
    cli = argparse.ArgumentParser(description="write / read `word v1 ... vd` vector files", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = cli.add_subparsers(dest="command", required=True)
    ex = sub.add_parser("export", formatter_class=argparse.ArgumentDefaultsHelpFormatter, help="job directory -> vector file")
    ex.add_argument("--job-dir", default=config.JOB_DIR, help="job directory of a finished or running training")
    ex.add_argument("--output", required=True, help="file to write")
    ex.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    ex.add_argument("--format", choices=EXPORT_FORMATS, default="glove", help="plain lines; lines behind a `V d` header; the header and raw float32")
    ex.add_argument("--precision", type=int, default=6, help="digits behind the point, 0 .. 9 (GloVe's %%lf: 6)")
    ex.add_argument("--block-rows", type=int, default=65536, help="rows formatted per GPU call")
    im = sub.add_parser("import", formatter_class=argparse.ArgumentDefaultsHelpFormatter, help="vector file -> job directory at step 0")
    im.add_argument("--vectors", required=True, help="file to read")
    im.add_argument("--job-dir", default=config.JOB_DIR, help="where params.json, vocab.txt, model.ckpt-0 and vectors.json go (used as given)")
    im.add_argument("--format", choices=IMPORT_FORMATS, default="auto", help="auto: by the first two lines")
    im.add_argument("--optimizer", default=config.OPTIMIZER, help="optimizer whose initial slots the checkpoint holds")
    im.add_argument("--block-bytes", default="64Mi", help="bytes of text per GPU call (Ki / Mi / Gi suffixes; at most 2^31 - 1)")
    return cli


def main(argv=None, backend=None) -> dict:
    args = build_cli().parse_args(argv)
    return (export_main if args.command == "export" else import_main)(args, backend)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    try:
        main()
    except KeyboardInterrupt:
        pass
