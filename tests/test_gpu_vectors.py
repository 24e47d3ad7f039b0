"""The word-vector kernels of libglove_prep_hip.so (include/glove_vectors_hip.h) on the GPU against tests/vectors_ref.py, bit
for bit: the records of a block at every tile edge, the parsed numbers and the fallback set, the formatted text and the rows
left to the host, capacities with canaries behind them, and trainer.vectors end to end on the device backend."""
import json

import numpy as np
import pytest
import torch

import vectors_ref as ref
from test_vectors import FALLBACKS, WORDS, format_values, job_tables, make_job, number_tokens, same_bits

pytestmark = pytest.mark.gpu
T = 4096                                    # GLOVE_VECTORS_TILE_BYTES
CANARY = 0x5A


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def dev_bytes(data: bytes):
    return dev(np.frombuffer(data, np.uint8).copy()) if data else torch.empty(0, dtype=torch.uint8, device="cuda:0")


def random_text(n_bytes, seed):
    """Words, numbers, blank lines, CRLF and runs of spaces, cut to n_bytes (so the last line has no newline, or half a token)."""
    rng = np.random.default_rng(seed)
    pieces, size = [], 0
    tokens = [b"w", b"word", b"0.125", b"-1.5e-3", "café".encode(), b"na\xc2\xa0me\t1", b"x" * 40]
    seps = [b" ", b" ", b" ", b"  ", b"\n", b"\n", b"\r\n", b"\n\n", b" \r \n", b"     "]
    while size < n_bytes:
        p = tokens[rng.integers(len(tokens))] + seps[rng.integers(len(seps))]
        pieces.append(p)
        size += len(p)
    return b"".join(pieces)[:n_bytes]


def edge_text():
    """A word, a number, a 0D 0A pair and a run of spaces each straddling a tile edge; records longer than one tile and than
    three; empty and blank lines; a last line without a newline."""
    buf = bytearray()

    def pad_to(offset):
        while len(buf) + 8 < offset:
            buf.extend(b"p 1 2\n")
        buf.extend(b" " * (offset - len(buf) - 1) + b"\n")
    pad_to(T - 4); buf.extend(b"straddle 1 2\n")                      # a word over the edge at T
    pad_to(2 * T - 6); buf.extend(b"w 0.123456 7\n")                  # a number over the edge at 2T
    pad_to(3 * T - 6); buf.extend(b"w 1 2\r\nv 3 4\n")                # 0D at 3T - 1, 0A at 3T
    pad_to(4 * T - 8); buf.extend(b"w 1" + b" " * 9 + b"2\n")         # a run of spaces over the edge at 4T
    pad_to(5 * T - 3); buf.extend(b"\n\n\n \r \n\n")                  # blank lines over the edge at 5T
    buf.extend(b"long1 " + b" ".join(b"%.6f" % (k / 7) for k in range(600)) + b"\n")           # 5.4 KB: longer than a tile
    buf.extend(b"\n  \nlong3 " + b" ".join(b"%.6f" % (-k / 3) for k in range(1800)) + b"\r\n")   # 17 KB: longer than three
    buf.extend(b"x" * (T + 100) + b" 1\n")                            # a word longer than a tile
    buf.extend(b"last 1 2")
    return bytes(buf)


# ---- lines
def check_lines(hip, data):
    start, fields = hip.vectors_lines(dev_bytes(data))
    want_start, want_fields = ref.lines(data)
    assert start.dtype == torch.int32 and fields.dtype == torch.int32
    np.testing.assert_array_equal(start.cpu().numpy(), want_start)
    np.testing.assert_array_equal(fields.cpu().numpy(), want_fields)
    return len(want_start)


@pytest.mark.parametrize("n_bytes", [0, 1, T - 1, T, T + 1, 3 * T + 7])
def test_lines_at_every_block_size(hip, n_bytes):
    for seed in range(3):
        check_lines(hip, random_text(n_bytes, seed))
    check_lines(hip, b"\n" * n_bytes)
    check_lines(hip, b" " * n_bytes)
    check_lines(hip, b"a" * n_bytes)
    check_lines(hip, (b"a\n" * n_bytes)[:n_bytes])           # the most records a block can hold


def test_lines_across_tile_edges(hip):
    data = edge_text()
    assert check_lines(hip, data) > 3000
    recs = ref.records(data)
    assert max(len(r) for r in recs) == 1801 and data[3 * T - 1:3 * T + 1] == b"\r\n" and data[T - 1:T + 1] == b"ad"
    assert data[2 * T - 2:2 * T + 2].isdigit() and data[4 * T - 3:4 * T + 3] == b" " * 6 and not data.endswith(b"\n")
    for cut in (T, 2 * T, 3 * T, 3 * T + 1, 5 * T, 6 * T):                    # blocks that end inside each of them
        check_lines(hip, data[:cut])
    check_lines(hip, data[5:])
    blk = dev_bytes(b"xxx" + data)[3:]
    start, fields = hip.vectors_lines(blk)                                   # a block that does not start on a 16-B boundary
    np.testing.assert_array_equal(start.cpu().numpy(), ref.lines(data)[0])
    np.testing.assert_array_equal(fields.cpu().numpy(), ref.lines(data)[1])


def test_lines_capacity_reports_the_true_count_and_writes_nothing_behind_it(hip):
    data = random_text(3 * T + 7, 5)
    want_start, want_fields = ref.lines(data)
    cap = len(want_start) // 2
    start = torch.full((cap + 16,), -7, dtype=torch.int32, device="cuda:0")
    fields = torch.full((cap + 16,), -7, dtype=torch.int32, device="cuda:0")
    sizes = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    hip.vectors_lines_enqueue(dev_bytes(data), start[:cap], fields[:cap], sizes)
    assert int(sizes[0]) == len(want_start) > cap
    np.testing.assert_array_equal(start[:cap].cpu().numpy(), want_start[:cap])
    np.testing.assert_array_equal(fields[:cap].cpu().numpy(), want_fields[:cap])
    assert (start[cap:] == -7).all() and (fields[cap:] == -7).all()


# ---- parse
def number_file(d, seed):
    """Records of d numbers (tokens of every family, fallbacks among them), some with fewer and some with more fields, words
    of 1 and of 1000 bytes; no trailing newline."""
    rng = np.random.default_rng(seed)
    tokens = number_tokens(seed, 300) + FALLBACKS * 3
    rng.shuffle(tokens)
    words = [b"a", b"w" * 1000, "café".encode(), b"na\xc2\xa0me\t1.5", b"1.5", b"word"]
    lines, k, r = [], 0, 0
    while k < len(tokens):
        n = d if r % 9 else (max(d - 2, 0) if r % 2 else d + 3)              # every ninth record is short or long
        sep = [b" ", b"  ", b"   "][r % 3]
        lines.append(words[r % len(words)] + sep + sep.join(tokens[k:k + n]) + [b"\n", b"\r\n", b" \n"][r % 3])
        k += max(n, 1)
        r += 1
    return b"\n".join([b"".join(lines[:5]), b"", b"".join(lines[5:])]).rstrip(b"\r\n ")


@pytest.fixture(scope="module")
def parsed_reference():
    out = {}
    for d in (1, 3, 4, 5, 50, 300):
        data = number_file(d, d)
        start, fields = ref.lines(data)
        out[d] = (data, start, fields, ref.parse(data, start, d))
    return out


@pytest.mark.parametrize("d", [1, 3, 4, 5, 50, 300])
def test_parse_bits_and_fallback_set(hip, parsed_reference, d):
    data, start, fields, (want, want_len, want_index, want_span) = parsed_reference[d]
    assert (fields < d + 1).any() and (fields > d + 1).any() and len(want_index) > 50 and want_len.max() == 1000 and want_len.min() == 1
    blk = dev_bytes(data)
    line_start, line_fields = hip.vectors_lines(blk)
    np.testing.assert_array_equal(line_fields.cpu().numpy(), fields)
    vec, word_len, fb_index, fb_span = hip.vectors_parse(blk, line_start, d)
    ld = (d + 3) // 4 * 4
    assert vec.shape == (len(start), ld) and vec.dtype == torch.float32
    np.testing.assert_array_equal(word_len.cpu().numpy(), want_len)
    np.testing.assert_array_equal(fb_index.cpu().numpy(), want_index)
    np.testing.assert_array_equal(fb_span.cpu().numpy(), want_span)
    got = vec.cpu().numpy().copy()
    got.reshape(-1)[want_index] = 0                     # (the device writes nothing for a fallback token)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert not len(bad), [(int(i) // ld, int(i) % ld, got.reshape(-1)[i], want.reshape(-1)[i]) for i in bad[:5]]
    assert not got[:, d:].any()


def test_parse_fallback_capacity(hip, parsed_reference):
    data, start, fields, (want, want_len, want_index, want_span) = parsed_reference[5]
    blk, m, cap_fb = dev_bytes(data), len(start), 3
    vec = torch.empty((m, 8), dtype=torch.float32, device="cuda:0")
    word_len = torch.empty(m, dtype=torch.int32, device="cuda:0")
    fb_index = torch.full((cap_fb + 8,), -7, dtype=torch.int64, device="cuda:0")
    fb_span = torch.full((cap_fb + 8,), -7, dtype=torch.int64, device="cuda:0")
    sizes = torch.tensor([m, 0, 0], dtype=torch.int64).to("cuda:0")
    hip.vectors_parse_enqueue(blk, dev(start), sizes[0:1], 5, vec, word_len, fb_index[:cap_fb], fb_span[:cap_fb], sizes[1:3])
    assert int(sizes[1]) == len(want_index) > cap_fb
    assert (fb_index[cap_fb:] == -7).all() and (fb_span[cap_fb:] == -7).all()
    listed = dict(zip(want_index.tolist(), want_span.tolist()))
    for i, s in zip(fb_index[:cap_fb].tolist(), fb_span[:cap_fb].tolist()):
        assert listed[i] == s
    # fewer lines than the arrays hold: the rest is not touched
    vec.fill_(7.0)
    sizes = torch.tensor([2, 0, 0], dtype=torch.int64).to("cuda:0")
    hip.vectors_parse_enqueue(blk, dev(start), sizes[0:1], 5, vec, word_len, fb_index[:cap_fb], fb_span[:cap_fb], sizes[1:3])
    assert (vec[2:] == 7.0).all() and not (vec[:2, 5:] != 0).any()


# ---- format
FORMAT_ROWS, FORMAT_D = 1000, 300
HOST_ROWS = {5: np.nan, 20: np.inf, 40: -np.inf, 62: 2.0 ** 31, 64: -2.0 ** 31, 999: np.nan}


@pytest.fixture(scope="module")
def format_table():
    pool = format_values()
    with np.errstate(invalid="ignore"):
        pool = pool[np.isfinite(pool) & (np.abs(pool) < np.float32(2.0 ** 31))]
    rng = np.random.default_rng(11)
    W = pool[rng.integers(len(pool), size=(FORMAT_ROWS, FORMAT_D))]
    W[:len(pool) // FORMAT_D].reshape(-1)[:len(pool) // FORMAT_D * FORMAT_D] = pool[:len(pool) // FORMAT_D * FORMAT_D]      # each once
    for r, x in HOST_ROWS.items():
        W[r, 0] = x                                     # column 0: inside every d
    words = [("w%d" % r if r % 7 else "café日" * (r % 5 + 1)) for r in range(FORMAT_ROWS)]
    words[3] = "x" * 1000
    return np.ascontiguousarray(W, np.float32), words, {}


def expected_rows(format_table, p, d):
    """The rows' texts by Python's % (tests/test_vectors.py holds the integer rule against it), b"" for a host row."""
    W, words, cache = format_table
    if (p, d) not in cache:
        cache[(p, d)] = [b"" if r in HOST_ROWS else (words[r] + "".join(" %.*f" % (p, x) for x in W[r, :d].tolist()) + "\n").encode()
                         for r in range(FORMAT_ROWS)]
    return cache[(p, d)]


@pytest.mark.parametrize("d", [1, 4, 5, 300])
@pytest.mark.parametrize("p", [0, 1, 6, 9])
def test_format_bytes_offsets_and_host_rows(hip, format_table, p, d):
    W, words, _ = format_table
    rows = expected_rows(format_table, p, d)
    Wd = dev(W)
    for n in (0, 1, 63, 64, 65, 1000):
        encoded = [w.encode() for w in words[:n]]
        word_off = np.concatenate([[0], np.cumsum([len(e) for e in encoded])]).astype(np.int64)
        word_bytes = dev_bytes(b"".join(encoded) or b"\0")
        want = b"".join(rows[:n])
        cap = int(word_off[-1]) + n * (d * (p + 13) + 1)
        assert len(want) <= cap
        out, row_off, host_row = hip.vectors_format(Wd[:n], d, p, word_bytes, dev(word_off), cap)
        assert out.cpu().numpy().tobytes() == want, (n, d, p)
        np.testing.assert_array_equal(row_off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(r) for r in rows[:n]])]))
        np.testing.assert_array_equal(host_row.cpu().numpy(), [int(r in HOST_ROWS) for r in range(n)])


def test_format_rule_on_the_device_equals_the_integer_rule(hip, format_table):
    """The reference's own integers (not %) on the first rows, so that the two restatements and the kernel are tied together."""
    W, words, _ = format_table
    n, d, p = 12, 300, 6
    encoded = [w.encode() for w in words[:n]]
    word_off = np.concatenate([[0], np.cumsum([len(e) for e in encoded])]).astype(np.int64)
    want, want_off, want_host = ref.format_rows(W[:n], d, p, b"".join(encoded), word_off)
    out, row_off, host_row = hip.vectors_format(dev(W[:n]), d, p, dev_bytes(b"".join(encoded)), dev(word_off), len(want))
    assert out.cpu().numpy().tobytes() == want and row_off.cpu().tolist() == want_off.tolist() and host_row.cpu().tolist() == want_host.tolist()


def test_format_capacity_one_byte_short(hip, format_table):
    W, words, _ = format_table
    n, d, p = 65, 5, 6
    want = b"".join(expected_rows(format_table, p, d)[:n])
    encoded = [w.encode() for w in words[:n]]
    word_off = dev(np.concatenate([[0], np.cumsum([len(e) for e in encoded])]).astype(np.int64))
    out = torch.full((len(want) + 16,), CANARY, dtype=torch.uint8, device="cuda:0")
    row_off = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    host_row = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    sizes = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    hip.vectors_format_enqueue(dev(W[:n]), d, p, dev_bytes(b"".join(encoded)), word_off, out[:len(want) - 1], row_off, host_row, sizes)
    assert int(row_off[n]) == len(want) and int(sizes[0]) == sum(r < n for r in HOST_ROWS)
    assert out[:len(want) - 1].cpu().numpy().tobytes() == want[:-1] and (out[len(want) - 1:] == CANARY).all()
    from trainer.hip_api import GloveHipError
    with pytest.raises(GloveHipError, match="capacity"):
        hip.vectors_format(dev(W[:n]), d, p, dev_bytes(b"".join(encoded)), word_off, len(want) - 1)


# ---- end to end on the device backend
def test_export_import_and_analogy_end_to_end(hip, tmp_path):
    from trainer import analogy, vectors
    V, d, G = 300, 50, 4
    rng = np.random.default_rng(21)
    vocab = ["<UNK>"] + ["g%d%d" % (i, j) for i in range(G) for j in range(G)] + WORDS[2:8] + ["v%d" % i for i in range(V - 23)]
    R = (0.05 * rng.standard_normal((V, d))).astype(np.float32)
    R[0] = 0
    for i in range(G):
        for j in range(G):
            R[1 + i * G + j, i] += 1.0
            R[1 + i * G + j, G + j] += 1.0
    make_job(tmp_path / "job", vocab, R, C=(0.05 * rng.standard_normal((V, d))).astype(np.float32))
    lines = [": grid"] + ["g%d%d g%d%d g%d%d g%d%d" % (i, j, i, k, l, j, l, k) for i in range(G) for j in range(2) for k in (2, 3) for l in ((i + 1) % G,)]
    lines += [": gram-random"] + ["v%d v%d v%d v%d" % tuple(rng.integers(V - 23, size=4)) for _ in range(8)]
    questions = tmp_path / "questions.txt"
    questions.write_text("\n".join(lines) + "\n")
    for fmt, header in (("glove", False), ("word2vec", True), ("word2vec-bin", True)):
        out = tmp_path / ("vectors." + fmt)
        vectors.main(["export", "--job-dir", str(tmp_path / "job"), "--output", str(out), "--format", fmt, "--block-rows", "128"], backend=hip)
        data = out.read_bytes()
        assert data == ref.write_vectors(vocab[1:], R[1:], fmt, 6)
        back = tmp_path / ("back_" + fmt)
        got = vectors.main(["import", "--vectors", str(out), "--job-dir", str(back), "--block-bytes", "20000", "--optimizer", "Adagrad"],
                           backend=hip)
        words, W = ref.read_word2vec_bin(data) if fmt == "word2vec-bin" else ref.read_text(data, header)
        assert got["words"] == vocab and got["records"] == V - 1 and got["duplicates"] == 0 and got["fallback_tokens"] == 0
        tables = job_tables(back)
        assert same_bits(tables["R"].numpy()[1:], W) and not tables["R"][0].any() and not tables["C"].any()
        if fmt == "word2vec-bin":
            assert same_bits(W, R[1:])
    results = []
    for job in (tmp_path / "job", tmp_path / "back_word2vec-bin"):
        analogy.main(job_dir=str(job), questions=str(questions), embeddings="row")
        results.append(json.loads((job / "eval" / "analogy.json").read_text()))
    a, b = results
    assert a["sections"] == b["sections"] and a["total"] == b["total"] and a["total"]["total"] == len(lines) - 2
    assert a["sections"][0]["accuracy"] == 1.0 and a["total"]["accuracy"] < 1.0
