"""Restatement of include/glove_vectors_hip.h in Python integers: the records of a block of bytes, the decimal -> float32
rule with its fallbacks, the float32 -> fixed decimal rule with its host rows; a reference reader and writer of the three
file formats that use nothing but float() and %; and the NumPy backend trainer.vectors runs on without a GPU."""
import re

import numpy as np
import torch

SEPARATORS = b" \n\r"
FIELD = re.compile(rb"[^ \n\r]+")
NUMBER = re.compile(rb"([+-]?)([0-9]*)(?:\.([0-9]*))?(?:[eE]([+-]?[0-9]+))?")
MAX_DIGITS, MAX_E10, MAX_SPAN = 15, 22, 65535
POW10 = [float("1e%d" % k) for k in range(MAX_E10 + 1)]         # exact doubles


# ---- fields and records
def records(data: bytes) -> list:
    """[[(offset, length) of every field] of every record], in order."""
    out, base = [], 0
    for line in data.split(b"\n"):
        fields = [(base + m.start(), m.end() - m.start()) for m in FIELD.finditer(line)]
        if fields:
            out.append(fields)
        base += len(line) + 1
    return out


# ---- decimal -> float32
def parse_token(token: bytes):
    """np.float32 by the fast path, or None for a fallback token."""
    m = NUMBER.fullmatch(token)
    if not m:
        return None
    sign, whole, frac, exp = m.groups()
    frac = frac or b""
    if not whole + frac:
        return None
    digits = (whole + frac).lstrip(b"0")
    if len(digits) > MAX_DIGITS:
        return None
    mant = int(digits) if digits else 0
    if mant == 0:
        value = 0.0
    else:
        e10 = int(exp or 0) - len(frac)
        if not -MAX_E10 <= e10 <= MAX_E10:
            return None
        value = float(mant) * POW10[e10] if e10 >= 0 else float(mant) / POW10[-e10]
    return np.float32(-value if sign == b"-" else value)


# ---- float32 -> fixed decimal
def format_value(x, p: int):
    """The text of the float32 x at precision p in integers, or None where the row goes to the host."""
    bits = int(np.asarray(x, np.float32).view(np.uint32))
    e, frac = (bits >> 23) & 255, bits & 0x7FFFFF
    if e == 255:
        return None
    m, ex = (frac | 0x800000, e - 150) if e else (frac, -149)
    if ex >= 8:
        return None
    n = m * 10 ** p
    assert n < 1 << 54
    if ex >= 0:
        q = n << ex
    elif -ex >= 64:
        q = 0
    else:
        s = -ex
        q, r, half = n >> s, n & ((1 << s) - 1), 1 << (s - 1)
        if r > half or (r == half and q & 1):
            q += 1
    assert q < 1 << 64
    text = ("-" if bits >> 31 else "") + str(q // 10 ** p)
    if p:
        text += "." + str(q % 10 ** p).zfill(p)
    return text.encode()


# ---- the reference reader and writer: float() and % only
def write_vectors(words, W, fmt="glove", precision=6) -> bytes:
    W = np.asarray(W, np.float32)
    head = b"%d %d\n" % W.shape if fmt != "glove" else b""
    if fmt == "word2vec-bin":
        return head + b"".join(w.encode() + b" " + row.astype("<f4").tobytes() + b"\n" for w, row in zip(words, W))
    return head + b"".join(
        (w + "".join(" %.*f" % (precision, float(x)) for x in row) + "\n").encode() for w, row in zip(words, W))


def read_text(data: bytes, header=False):
    """(words, float32 [n, d]) of a text file: str.split on the three separators, np.float32(float(token))."""
    recs = records(data)[1 if header else 0:]
    words = [data[o:o + n].decode() for o, n in (r[0] for r in recs)]
    W = np.asarray([[np.float32(float(data[o:o + n])) for o, n in r[1:]] for r in recs], np.float32)
    return words, W


def read_word2vec_bin(data: bytes):
    end = data.index(b"\n")
    V, d = (int(x) for x in data[:end].split())
    pos, words, rows = end + 1, [], []
    for _ in range(V):
        while data[pos:pos + 1] in (b"\n", b"\r"):
            pos += 1
        sp = data.index(b" ", pos)
        words.append(data[pos:sp].decode())
        rows.append(np.frombuffer(data, "<f4", d, sp + 1))
        pos = sp + 1 + 4 * d
    return words, np.asarray(rows, np.float32).reshape(V, d)


def imported_tables(words, W):
    """What trainer.vectors import makes of a file's records: (vocabulary, R, duplicates dropped)."""
    d = W.shape[1]
    vocab, rows, seen, unk, dup = ["<UNK>"], [np.zeros(d, np.float32)], {"<UNK>"}, False, 0
    for w, row in zip(words, W):
        if w == "<UNK>" and not unk:
            rows[0], unk = row, True
        elif w in seen:
            dup += 1
        else:
            seen.add(w)
            vocab.append(w)
            rows.append(row)
    return vocab, np.asarray(rows, np.float32).reshape(len(vocab), d), dup


# ---- the three operations of a backend, on torch tensors on the CPU
def _round_up4(n):
    return (n + 3) // 4 * 4


def lines(data: bytes):
    recs = records(data)
    return (np.asarray([r[0][0] for r in recs], np.int32).reshape(-1), np.asarray([len(r) for r in recs], np.int32).reshape(-1))


def parse(data: bytes, line_start, d: int, ld=None):
    """(vec float32 [m, ld] with zeros at fallbacks, word_len, fb_index sorted, fb_span in that order)."""
    ld = _round_up4(d) if ld is None else ld
    vec = np.zeros((len(line_start), ld), np.float32)
    word_len, fb = np.zeros(len(line_start), np.int32), []
    for r, s in enumerate(np.asarray(line_start).tolist()):
        end = data.find(b"\n", s)
        fields = [(s + m.start(), m.end() - m.start()) for m in FIELD.finditer(data[s:len(data) if end < 0 else end])]
        word_len[r] = fields[0][1]
        for j, (o, n) in enumerate(fields[1:d + 1]):
            v = parse_token(data[o:o + n])
            if v is None:
                fb.append((r * ld + j, (o << 16) | min(n, MAX_SPAN)))
            else:
                vec[r, j] = v
    fb.sort()
    return (vec, word_len, np.asarray([i for i, _ in fb], np.int64).reshape(-1), np.asarray([s for _, s in fb], np.int64).reshape(-1))


def format_rows(W, d: int, precision: int, word_bytes: bytes, word_off):
    """(out bytes, row_off int64 [n + 1], host_row uint8 [n])."""
    W = np.asarray(W, np.float32)
    out, row_off, host = [], [0], []
    for r in range(W.shape[0]):
        texts = [format_value(x, precision) for x in W[r, :d]]
        host.append(int(any(t is None for t in texts)))
        row = b"" if host[-1] else bytes(word_bytes[int(word_off[r]):int(word_off[r + 1])]) + b"".join(b" " + t for t in texts) + b"\n"
        out.append(row)
        row_off.append(row_off[-1] + len(row))
    return b"".join(out), np.asarray(row_off, np.int64), np.asarray(host, np.uint8).reshape(-1)


class NumpyVectorsBackend:
    """What trainer.vectors asks of a backend (GloveHip's vectors_lines / vectors_parse / vectors_format), by the rules above."""
    device = "cpu"

    def vectors_lines(self, block):
        start, fields = lines(block.numpy().tobytes())
        return torch.from_numpy(start), torch.from_numpy(fields)

    def vectors_parse(self, block, line_start, d):
        return tuple(torch.from_numpy(a) for a in parse(block.numpy().tobytes(), line_start.numpy(), d))

    def vectors_format(self, W, d, precision, word_bytes, word_off, cap_out):
        out, row_off, host = format_rows(W.numpy(), d, precision, word_bytes.numpy().tobytes(), word_off.numpy())
        assert len(out) <= cap_out
        return torch.from_numpy(np.frombuffer(out, np.uint8).copy()), torch.from_numpy(row_off), torch.from_numpy(host)
