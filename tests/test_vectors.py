"""Reading and writing word-vector files, without a GPU: the two exact rules of tests/vectors_ref.py against float() and %,
the field splitting, trainer.vectors (export, import, errors) on the NumPy backend against the reference reader and writer,
and the surface and host-side argument checks of the vector entry points of libglove_prep_hip.so
(include/glove_vectors_hip.h).  The kernels themselves: tests/test_gpu_vectors.py."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import vectors_ref as ref
from test_analogy import BADARG, FAKE, declared_functions

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
HEADER = REPO / "include" / "glove_vectors_hip.h"
FALLBACKS = [b"1234567890123456", b"0.1234567890123456", b"1e23", b"1e-23", b"1e-45", b"123e23", b"nan", b"inf", b"-inf",
             b"Infinity", b"0x10", b"1_0", b"--1", b"1.2.3", b"1e", b"e5", b".", b"+", b"-", b"1e+", b"1,5", b"\xc2\xa01"]


def f32(token):
    with np.errstate(over="ignore"):
        return np.float32(float(token))


def same_bits(a, b):
    return np.asarray(a, np.float32).view(np.uint32).tolist() == np.asarray(b, np.float32).view(np.uint32).tolist()


def number_tokens(seed=0, n=4000):
    """Tokens of every family the parser meets: %f, %e, %g and repr of random floats, and the edges of the fast path."""
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        values = np.concatenate([rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n), rng.integers(-2 ** 26, 2 ** 26, n).astype(np.float64),
                                 rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)])
    values = values[np.isfinite(values)]
    tokens = []
    for k, x in enumerate(values.tolist()):
        tokens.append([b"%.6f", b"%.5f", b"%e", b"%.9e", b"%g", b"%.6g", b"%.14e", b"%.15e", b"%.17g"][k % 9] % x)
        if k % 7 == 0:
            tokens.append(repr(x).encode())
        if k % 11 == 0:
            tokens.append(repr(float(np.float32(x))).encode())
    tokens += [b"0", b"-0", b"+0", b"-0.0", b".5", b"5.", b"+.5", b"-5.", b"1E+05", b"1e-05", b"0e999", b"-0e-999", b"00012.500",
               b"123456789012345", b"1234567890123456", b"0.123456789012345", b"0.0123456789012345", b"0.1234567890123456",
               b"000000000000000000001", b"1e22", b"1e23", b"1e-22", b"1e-23", b"123e20", b"123e21", b"1.5e23", b"1.5e24",
               b"1.25e-20", b"1.25e-21", b"999999999999999e22", b"999999999999999e-22", b"0.000000000000000000001",
               b"16777217", b"16777219", b"33554434", b"33554438", b"-16777217", b"3.4028235e38", b"3.4028236e38", b"1e39"]
    return tokens


# ---- the two rules
def test_parse_rule_equals_float_on_every_family():
    tokens = number_tokens()
    fallbacks = 0
    for t in tokens:
        got = ref.parse_token(t)
        if got is None:
            fallbacks += 1
            continue
        assert same_bits(got, f32(t)), t
    assert len(tokens) > 12000 and fallbacks < len(tokens) // 2         # (coverage: most tokens take the fast path)
    rng = np.random.default_rng(1)
    for x in rng.standard_normal(3000).astype(np.float32).tolist():            # what %f and %.6g write never falls back
        for t in (b"%f" % x, b"%.6g" % x, b"%.5f" % (1000 * x)):
            assert ref.parse_token(t) is not None and same_bits(ref.parse_token(t), f32(t)), t


def test_parse_rule_falls_back_exactly_on_the_listed_families():
    for t in FALLBACKS:
        assert ref.parse_token(t) is None, t
    for t in (b"123456789012345", b"0.00000123456789012345", b"1e22", b"1e-22", b"100000000000000e8", b"0e999", b"5.", b".5", b"-0"):
        assert ref.parse_token(t) is not None and same_bits(ref.parse_token(t), f32(t)), t
    for t in (b"16777217", b"16777219", b"33554434", b"33554438"):             # double -> float ties
        assert same_bits(ref.parse_token(t), f32(t))
    assert ref.parse_token(b"16777217") == 16777216 and ref.parse_token(b"16777219") == 16777220
    assert np.signbit(ref.parse_token(b"-0")) and not np.signbit(ref.parse_token(b"0"))


def format_values():
    rng = np.random.default_rng(2)
    bits = rng.integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32)
    small = bits[:1000] & np.uint32(0x807FFFFF) | (rng.integers(100, 158, 1000).astype(np.uint32) << np.uint32(23))
    edges = np.asarray([0.5, 1.5, 2.5, -0.5, 0.125, 0.375, 0.625, -0.0, 0.0, 0.9999995, 9.9999995, 0.99999994, 99.5, 1e-7, -1e-7,
                        5e-7, 0.0000005, 1.4e-45, -1.4e-45, 1e-40, 1.1754942e-38, 2147483520.0, -2147483520.0, 16777216.0,
                        0.05, 0.25, 0.35, 1e9, 123456.789], np.float32)
    return np.concatenate([bits.view(np.float32), small.view(np.float32), rng.standard_normal(1000).astype(np.float32), edges])


@pytest.mark.parametrize("p", range(10))
def test_format_rule_equals_percent(p):
    hosts = 0
    for x in format_values():
        got = ref.format_value(x, p)
        if not np.isfinite(x) or abs(float(x)) >= 2.0 ** 31:
            assert got is None
            hosts += 1
        else:
            assert got == ("%.*f" % (p, float(x))).encode(), (float(x), p)
    assert hosts > 100
    if p == 0:
        assert [ref.format_value(np.float32(x), 0) for x in (0.5, 1.5, 2.5, -0.0)] == [b"0", b"2", b"2", b"-0"]
    if p == 2:
        assert [ref.format_value(np.float32(x), 2) for x in (0.125, 0.375)] == [b"0.12", b"0.38"]
    if p == 6:
        assert [ref.format_value(np.float32(x), 6) for x in (0.9999995, 9.9999995, -0.0)] == [b"1.000000", b"9.999999", b"-0.000000"]


def test_field_splitting():
    data = ("na\u00a0me\t1.5 1 2\r\n" "  a   3  4 \n" "\n" " \r \n" "\u3000b\u2003  5 6\n" "last 7 8").encode()
    recs = ref.records(data)
    assert [[data[o:o + n] for o, n in r] for r in recs] == [
        ["na\u00a0me\t1.5".encode(), b"1", b"2"], [b"a", b"3", b"4"], ["\u3000b\u2003".encode(), b"5", b"6"], [b"last", b"7", b"8"]]
    start, fields = ref.lines(data)
    assert fields.tolist() == [3, 3, 3, 3] and [data[s:s + 1] for s in start.tolist()] == [b"n", b"a", b"\xe3", b"l"]
    vec, word_len, fb_index, fb_span = ref.parse(data, start, 2)
    assert vec[:, :2].tolist() == [[1, 2], [3, 4], [5, 6], [7, 8]] and not vec[:, 2:].any() and vec.shape == (4, 4)
    assert word_len.tolist() == [10, 1, 7, 4] and len(fb_index) == 0
    assert ref.records(b"") == [] and ref.records(b"\n\r\n  ") == [] and ref.records(b"x") == [[(0, 1)]]


# ---- the command line on the NumPy backend
def make_job(job, vocab, R, C=None, optimizer="Adagrad"):
    """A job directory with one checkpoint holding the given tables, the way trainer.svd writes one."""
    from trainer.config_utils import build_parser, init_params
    from trainer.hip_api import DeviceTables
    from trainer.train_utils import CheckpointManager
    job.mkdir(parents=True, exist_ok=True)
    (job / "vocab.txt").write_bytes("\n".join(vocab).encode())
    params = init_params(vars(build_parser().parse_args([
        "--vocab-txt", str(job / "vocab.txt"), "--job-dir", str(job), "--disable-datetime-path", "--embedding-size",
        str(R.shape[1]), "--optimizer", optimizer])).copy())
    tables = DeviceTables(len(vocab), R.shape[1], optimizer, device="cpu", seed=0)
    tables.embeddings("R").copy_(torch.from_numpy(R))
    tables.embeddings("C").copy_(torch.from_numpy(R[::-1].copy() if C is None else C))
    CheckpointManager(params["job_dir"]).save(tables)
    return params


def job_tables(job):
    from trainer.train_utils import CheckpointManager
    return torch.load(CheckpointManager(str(job)).latest(), map_location="cpu", weights_only=False)["tables"]


def random_table(V, d, seed=5):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((V, d)) * 10.0 ** rng.integers(-4, 3, (V, d))).astype(np.float32)
    W.reshape(-1)[:8] = [0.5, -0.0, 0.9999995, 2.5, 1e-7, -1e-7, 123456.79, 1.4e-45]
    return W


WORDS = ["<UNK>", "the", ",", "na\u00a0me\t1.5", "café", "日本", "x.y1", "a" * 70] + ["w%d" % i for i in range(30)]


def run(argv):
    from trainer import vectors
    return vectors.main(argv, backend=ref.NumpyVectorsBackend())


@pytest.mark.parametrize("fmt, precision", [("glove", 6), ("word2vec", 6), ("glove", 0), ("word2vec", 9), ("word2vec-bin", 6)])
def test_export_equals_the_reference_writer(tmp_path, fmt, precision):
    R = random_table(len(WORDS), 5)
    make_job(tmp_path / "job", WORDS, R)
    for embeddings, W in (("row", R), ("col", R[::-1]), ("sum", R + R[::-1])):
        out = tmp_path / ("%s.%s" % (embeddings, fmt))
        run(["export", "--job-dir", str(tmp_path / "job"), "--output", str(out), "--embeddings", embeddings, "--format", fmt,
             "--precision", str(precision), "--block-rows", "7"])
        assert out.read_bytes() == ref.write_vectors(WORDS[1:], W[1:], fmt, precision), embeddings      # <UNK> left out


def test_export_splices_the_rows_the_backend_leaves_to_the_host(tmp_path):
    R = random_table(len(WORDS), 4)
    R[3, 1], R[4, 0], R[9, 3], R[10, 2] = np.nan, np.inf, -2.0 ** 31, 2.0 ** 31
    make_job(tmp_path / "job", WORDS, R)
    run(["export", "--job-dir", str(tmp_path / "job"), "--output", str(tmp_path / "v.txt"), "--block-rows", "6"])
    assert (tmp_path / "v.txt").read_bytes() == ref.write_vectors(WORDS[1:], R[1:], "glove", 6)
    assert b" nan " in (tmp_path / "v.txt").read_bytes() and b" -2147483648.000000\n" in (tmp_path / "v.txt").read_bytes()


def check_import(job, words, W, records, duplicates, fallbacks, fmt):
    from trainer.data_utils import read_vocab
    vocab, R, dup = ref.imported_tables(words, W)
    tables = job_tables(job)
    assert read_vocab(job / "vocab.txt") == vocab and dup == duplicates
    assert (tables["V"], tables["d"], int(tables["global_step"])) == (len(vocab), W.shape[1], 0)
    assert same_bits(tables["R"].numpy(), R) and tables["R"].shape == R.shape
    assert not tables["C"].any() and not tables["br"].any() and not tables["bc"].any()
    rec = json.loads((job / "vectors.json").read_text())
    assert (rec["format"], rec["d"], rec["records"], rec["duplicates_dropped"], rec["fallback_tokens"]) == (
        fmt, W.shape[1], records, duplicates, fallbacks)
    assert rec["seconds"] and rec["vocab_size"] == len(vocab)
    params = json.loads((job / "params.json").read_text())
    assert params["embedding_size"] == W.shape[1] and Path(params["vocab_txt"]) == job / "vocab.txt"


@pytest.mark.parametrize("block_bytes", ["64Mi", "30", "1"])
def test_import_equals_the_reference_reader(tmp_path, block_bytes):
    for name, header, fmt, fallbacks in (("vectors_glove.txt", False, "text", 2), ("vectors_word2vec.txt", True, "word2vec", 0)):
        data = (GOLDEN / name).read_bytes()
        words, W = ref.read_text(data, header)
        job = tmp_path / name
        out = run(["import", "--vectors", str(GOLDEN / name), "--job-dir", str(job), "--block-bytes", block_bytes, "--optimizer", "Adagrad"])
        check_import(job, words, W, len(words), 1 if not header else 0, fallbacks, fmt)
        assert out["unk_in_file"] == (not header)
    # the glove fixture: its own <UNK> record is row 0, the second `the` is dropped, the word with a no-break space and a tab is one word
    tables = job_tables(tmp_path / "vectors_glove.txt")
    assert tables["R"][0].tolist() == [f32("0.001"), f32("0.002"), f32("0.003")]
    from trainer.data_utils import read_vocab
    assert read_vocab(tmp_path / "vectors_glove.txt" / "vocab.txt") == ["<UNK>", "the", ",", "na\u00a0me\t1.5", "end"]
    R = tables["R"].numpy()
    assert np.isnan(R[4, 2]) and R[4, 1] == f32("1e23") and R[1, 0] == f32("0.418")
    assert not job_tables(tmp_path / "vectors_word2vec.txt")["R"][0].any()                 # no <UNK> in the file: zeros


def test_binary_round_trip_keeps_every_bit(tmp_path):
    rng = np.random.default_rng(8)
    R = rng.integers(0, 2 ** 32, (len(WORDS), 6), dtype=np.uint64).astype(np.uint32).view(np.float32)     # NaNs and all
    make_job(tmp_path / "job", WORDS, R)
    run(["export", "--job-dir", str(tmp_path / "job"), "--output", str(tmp_path / "v.bin"), "--format", "word2vec-bin"])
    words, W = ref.read_word2vec_bin((tmp_path / "v.bin").read_bytes())
    assert words == WORDS[1:] and same_bits(W, R[1:])
    run(["import", "--vectors", str(tmp_path / "v.bin"), "--job-dir", str(tmp_path / "back")])         # auto: not text behind the header
    check_import(tmp_path / "back", words, W, len(words), 0, 0, "word2vec-bin")
    assert same_bits(job_tables(tmp_path / "back")["R"].numpy()[1:], R[1:])


@pytest.mark.parametrize("fmt, p", [("glove", 6), ("word2vec", 2), ("glove", 9), ("word2vec", 0)])
def test_text_round_trip_is_the_rounded_decimal(tmp_path, fmt, p):
    R = random_table(len(WORDS), 7)
    make_job(tmp_path / "job", WORDS, R)
    run(["export", "--job-dir", str(tmp_path / "job"), "--output", str(tmp_path / "v.txt"), "--format", fmt, "--precision", str(p)])
    run(["import", "--vectors", str(tmp_path / "v.txt"), "--job-dir", str(tmp_path / "back"), "--block-bytes", "1Ki"])
    want = np.asarray([[np.float32(float("%.*f" % (p, float(x)))) for x in row] for row in R[1:]], np.float32)
    got = job_tables(tmp_path / "back")["R"].numpy()
    assert same_bits(got[1:], want) and not got[0].any()
    assert json.loads((tmp_path / "back" / "vectors.json").read_text())["fallback_tokens"] == 0


def test_import_errors_name_the_line(tmp_path):
    def refused(data, match, **kw):
        path = tmp_path / "bad.txt"
        path.write_bytes(data)
        with pytest.raises(ValueError, match=match):
            run(["import", "--vectors", str(path), "--job-dir", str(tmp_path / "bad"), "--block-bytes", kw.get("block", "64Mi")])
    refused(b"a 1 2\n\nb 1 2 3\n", "line 3: expected 3 fields .a word and 2 numbers., got 4")
    refused(b"a 1 2\nb 1\n", "line 2: expected 3 fields", block="1")
    refused(b"a 1 2\nb\xff 1 2\n", "line 2: the word .* is not UTF-8")
    refused(b"a 1 2\r\nb 1 0x10\n", "line 2: b'0x10' is no number")
    refused(b"a\n", "line 1: a word and no numbers")
    refused(b"\n \n", "holds no record")
    refused(b"3 2\na 1 2\nb 3 4\n", "the header names 3 x 2, the file holds 2 records of 2 numbers")
    from trainer import vectors
    with pytest.raises(ValueError, match="starts with a line of two integers"):
        vectors.sniff(GOLDEN / "vectors_glove.txt", "word2vec-bin")
    with pytest.raises(ValueError, match="holds a space or a line break"):
        vectors.export_vectors(["a b"], np.zeros((1, 2), np.float32), tmp_path / "x.txt", backend=ref.NumpyVectorsBackend())


def test_an_imported_directory_opens_like_a_trained_one(tmp_path):
    from test_analogy import RefBackend
    from trainer.estimator import Estimator
    run(["import", "--vectors", str(GOLDEN / "vectors_word2vec.txt"), "--job-dir", str(tmp_path / "job"), "--optimizer", "Adam"])
    params = json.loads((tmp_path / "job" / "params.json").read_text())
    e = Estimator(params, backend=RefBackend(), device="cpu")
    words, W = ref.read_text((GOLDEN / "vectors_word2vec.txt").read_bytes(), header=True)
    assert e.vocab_size == 5 and e.model.tables.global_step == 0
    assert same_bits(e._evaluation_table("row", None).numpy()[1:, :2], W)          # (rows are stored padded)
    assert np.array_equal(e._evaluation_table("sum", None).numpy()[1:, :2], W)     # C = 0: the same values (-0.0 + 0.0 is 0.0)
    assert not e._evaluation_table("col", None).any()


# ---- the library: surface, workspace queries, argument checks (all before any launch)
@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.PREP_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_prep_library()


def test_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADER)
    assert set(names) == set(hip_api.VECTORS_EXPORTED_SYMBOLS) and len(names) == len(hip_api.VECTORS_EXPORTED_SYMBOLS) == 6
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_vectors_abi_version() == hip_api.GLOVE_VECTORS_ABI_VERSION == 1
    text = HEADER.read_text()
    assert "GLOVE_VECTORS_ABI_VERSION 1" in text and "GLOVE_VECTORS_TILE_BYTES %d" % hip_api.VECTORS_TILE_BYTES in text
    assert "GLOVE_VECTORS_MAX_SPAN %d" % hip_api.VECTORS_MAX_SPAN in text and "GLOVE_VECTORS_MAX_D %d" % hip_api.VECTORS_MAX_D in text
    assert hip_api.VECTORS_MAX_SPAN == ref.MAX_SPAN
    others = set(hip_api.EXPORTED_SYMBOLS) | set(hip_api.EVAL_EXPORTED_SYMBOLS) | set(hip_api.EVAL_SIM_EXPORTED_SYMBOLS) \
        | set(hip_api.EVAL_CLUSTER_EXPORTED_SYMBOLS) | set(hip_api.PREP_EXPORTED_SYMBOLS) | set(hip_api.TEXT_EXPORTED_SYMBOLS) \
        | set(hip_api.FACTOR_EXPORTED_SYMBOLS)
    assert not set(names) & others
    train = hip_api.load_library()
    assert not any(hasattr(train, n) for n in names)            # the prep library's, not the training library's
    assert len(hip_api.PREP_EXPORTED_SYMBOLS) == 7 and len(hip_api.TEXT_EXPORTED_SYMBOLS) == 8
    assert hip_api.GLOVE_ABI_VERSION == 15 and len(hip_api.EXPORTED_SYMBOLS) == 42
    assert hip_api.GLOVE_TEXT_ABI_VERSION == 1 and hip_api.GLOVE_COOC_STREAM_ABI_VERSION == 1


def test_workspace_queries_are_pure_host_functions(lib):
    from trainer import hip_api
    lines, fmt = lib.glove_vectors_lines_workspace_bytes, lib.glove_vectors_format_workspace_bytes
    assert lines(-1, 5) == 0 and lines(2 ** 31, 5) == 0 and lines(5, -1) == 0 and lines(0, 0) > 0 and lines(2 ** 31 - 1, 2 ** 30) > 0
    for bad in ((-1, 4), (2 ** 31, 4), (5, 0), (5, -4), (5, hip_api.VECTORS_MAX_D + 1)):
        assert fmt(*bad) == 0, bad
    assert fmt(0, 1) > 0 and fmt(2 ** 31 - 1, hip_api.VECTORS_MAX_D) > 0
    T = hip_api.VECTORS_TILE_BYTES
    sizes = [0, 1, T - 1, T, T + 1, 10 ** 6, 10 ** 8, 2 ** 31 - 1]
    for a, b in zip(sizes, sizes[1:]):
        assert lines(a, 1000) <= lines(b, 1000) and lines(10 ** 6, a) <= lines(10 ** 6, b) and fmt(a, 300) <= fmt(b, 300)
    assert lines(10 ** 6, 1000) < lines(10 ** 8, 1000) and lines(10 ** 8, 1000) < lines(10 ** 8, 10 ** 7) and fmt(10 ** 3, 300) < fmt(10 ** 6, 300)
    # the layouts, as the header states them
    up = lambda x: (x + 255) // 256 * 256
    tiles = (10 ** 6 + T - 1) // T
    assert lines(10 ** 6, 1000) == 2 * up(16 * tiles) + up(4 * 1000) + up((64 << 10) + 16 * tiles)
    assert lines(10 ** 6, 10 ** 9) == 2 * up(16 * tiles) + up(4 * 500000) + up((64 << 10) + 16 * tiles)
    assert fmt(1000, 300) == up(8 * 1001) + up((64 << 10) + 8 * 1001)


def test_argument_errors_are_reported_before_any_launch(lib):
    big = 1 << 30
    call = lambda fn, order, defaults, kw: fn(*[{**defaults, **kw}[k] for k in order])
    A, O = 0x100000, 0x700000
    # lines
    order = ("bytes", "n_bytes", "line_start", "line_fields", "n_lines", "cap", "ws", "ws_bytes", "stream")
    base = dict(bytes=FAKE, n_bytes=100, line_start=O, line_fields=O + 0x10000, n_lines=O + 0x20000, cap=50, ws=A, ws_bytes=big, stream=None)
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap=-1), dict(bytes=None), dict(line_start=None), dict(line_fields=None),
               dict(n_lines=None), dict(ws=None)):
        assert call(lib.glove_vectors_lines_u8, order, base, kw) == BADARG, kw
    assert call(lib.glove_vectors_lines_u8, order, base, dict(ws_bytes=16)) == -2                # GLOVE_E_WORKSPACE
    # parse
    order = ("bytes", "n_bytes", "line_start", "n_lines", "cap_lines", "d", "ld", "vec", "word_len", "fb_index", "fb_span", "n_fallback",
             "cap_fb", "stream")
    base = dict(bytes=FAKE, n_bytes=100, line_start=A, n_lines=A + 0x10000, cap_lines=50, d=5, ld=8, vec=O, word_len=O + 0x10000,
                fb_index=O + 0x20000, fb_span=O + 0x30000, n_fallback=O + 0x40000, cap_fb=10, stream=None)
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap_lines=-1), dict(cap_fb=-1), dict(d=0), dict(d=-3), dict(d=65537, ld=65540),
               dict(ld=4), dict(ld=6), dict(ld=10), dict(d=6, ld=6), dict(bytes=None), dict(line_start=None), dict(n_lines=None),
               dict(vec=None), dict(word_len=None), dict(fb_index=None), dict(fb_span=None), dict(n_fallback=None)):
        assert call(lib.glove_vectors_parse_f32, order, base, kw) == BADARG, kw
    # format
    order = ("W", "n_rows", "d", "ld", "precision", "word_bytes", "word_off", "out", "row_off", "host_row", "n_host_rows", "cap_out",
             "ws", "ws_bytes", "stream")
    base = dict(W=FAKE, n_rows=10, d=5, ld=8, precision=6, word_bytes=A, word_off=A + 0x10000, out=O, row_off=O + 0x10000,
                host_row=O + 0x20000, n_host_rows=O + 0x30000, cap_out=1000, ws=A + 0x20000, ws_bytes=big, stream=None)
    for kw in (dict(n_rows=-1), dict(n_rows=2 ** 31), dict(d=0), dict(d=65537, ld=65540), dict(ld=4), dict(precision=-1), dict(precision=10),
               dict(cap_out=-1), dict(W=None), dict(word_off=None), dict(out=None), dict(row_off=None), dict(host_row=None),
               dict(n_host_rows=None), dict(ws=None)):
        assert call(lib.glove_vectors_format_f32, order, base, kw) == BADARG, kw
    assert call(lib.glove_vectors_format_f32, order, base, dict(ws_bytes=16)) == -2
