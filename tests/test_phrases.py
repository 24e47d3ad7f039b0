"""Phrase detection without a GPU: trainer.phrases on the NumPy backend of tests/phrases_ref.py against the sequential
restatement word2phrase_plain, and the surface and host-side argument checks of the fifth header of libglove_prep_hip.so
(include/glove_phrases_hip.h)."""
import collections
import json
import re
from pathlib import Path

import pytest

import cooc_stream_ref
import phrases_cases as cases
import phrases_ref as pref
import text_ref
from test_analogy import BADARG, FAKE, WORKSPACE, declared_functions

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "glove_phrases_hip.h"
SEEDS = (1, 3)
BLOCKS = (64, 257, 4096, 1 << 30)
EDGES = cases.edge_cases()


class Backends(pref.NumpyPhrasesBackend, text_ref.NumpyTextBackend, cooc_stream_ref.NumpyBackend):
    """Tokenizing, merging and the three phrase operations in NumPy: what trainer.phrases and trainer.cooccur drive."""


@pytest.fixture(scope="module")
def lib():
    from trainer import hip_api
    if not hip_api.PREP_LIB_PATH.exists():
        import __graft_entry__
        __graft_entry__.build()
    return hip_api.load_prep_library()


def header_define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, HEADER.read_text()).group(1))


# ---- surface
def test_header_declares_exactly_the_bound_symbols(lib):
    from trainer import hip_api
    names = declared_functions(HEADER)
    assert set(names) == set(hip_api.PHRASES_EXPORTED_SYMBOLS)
    assert len(names) == len(hip_api.PHRASES_EXPORTED_SYMBOLS) == 7
    for n in names:
        assert hasattr(lib, n), n
    assert lib.glove_phrases_abi_version() == hip_api.GLOVE_PHRASES_ABI_VERSION == header_define("GLOVE_PHRASES_ABI_VERSION") == 1
    assert header_define("GLOVE_PHRASE_TILE") == hip_api.PHRASE_TILE
    assert header_define("GLOVE_PHRASE_SELECT_TILE") == hip_api.PHRASE_SELECT_TILE
    every = {k: v for k, v in vars(hip_api).items() if k.endswith("EXPORTED_SYMBOLS")}
    assert len(every) >= 11
    for k, v in every.items():
        if k != "PHRASES_EXPORTED_SYMBOLS":
            assert not set(names) & set(v), k
    train = hip_api.load_library()
    assert not any(hasattr(train, n) for n in names)            # the prep library's, not the training library's
    # the other prep headers still say 1, and their symbol lists are what they were
    for header, macro in (("glove_cooc_stream_hip.h", "GLOVE_COOC_STREAM_ABI_VERSION"), ("glove_text_hip.h", "GLOVE_TEXT_ABI_VERSION"),
                          ("glove_vectors_hip.h", "GLOVE_VECTORS_ABI_VERSION"), ("glove_cooc_options_hip.h", "GLOVE_COOC_OPTIONS_ABI_VERSION")):
        assert "%s 1" % macro in (REPO / "include" / header).read_text() and getattr(hip_api, macro) == 1
    assert lib.glove_cooc_stream_abi_version() == lib.glove_text_abi_version() == lib.glove_vectors_abi_version() \
        == lib.glove_cooc_options_abi_version() == 1
    assert (len(hip_api.PREP_EXPORTED_SYMBOLS), len(hip_api.TEXT_EXPORTED_SYMBOLS), len(hip_api.VECTORS_EXPORTED_SYMBOLS),
            len(hip_api.COOC_OPTIONS_EXPORTED_SYMBOLS)) == (7, 8, 6, 5)


# ---- workspace
def test_workspace_queries_equal_the_stated_layouts(lib):
    from trainer import hip_api
    big, sel, join = lib.glove_phrase_bigram_workspace_bytes, lib.glove_phrase_select_workspace_bytes, lib.glove_phrase_join_workspace_bytes
    T, S = hip_api.PHRASE_TILE, hip_api.PHRASE_SELECT_TILE
    up = lambda x: (x + 255) // 256 * 256
    for cap in (0, 1, T - 1, T, T + 1, 3 * T + 5, 10 ** 6, 2 ** 31 - 1):
        n, tiles = max(1, cap), max(1, -(-cap // T))
        assert big(cap) == 2 * up(8 * n) + up(4 * n) + up(8 * 32) + up((16 << 20) + 16 * n), cap
        assert join(cap) == up(4 * n) + up(4 * 64) + 2 * up(8 * tiles) + up((64 << 10) + 8 * tiles), cap
    for cap in (0, 1, S - 1, S, S + 1, 3 * S + 5, 10 ** 6, 1 << 40):
        tiles = max(1, -(-cap // S))
        assert sel(cap) == 2 * up(8 * tiles) + up((64 << 10) + 8 * tiles), cap
    assert big(-1) == big(2 ** 31) == join(-1) == join(2 ** 31) == sel(-1) == sel((1 << 40) + 1) == 0


# ---- refusals, all before any launch
def test_argument_errors_are_reported_before_any_launch(lib):
    big = 1 << 30
    BY, ST, LN, ID, NT, KO, CO, NO, SO = (0x100000 * i for i in range(1, 10))      # distinct "device" ranges, 1 MiB apart
    order = ("bytes", "n_bytes", "start", "len", "ids", "n_tokens", "cap_tokens", "keys_out", "counts_out", "n_out", "cap", "ws",
             "ws_bytes", "stream")
    base = dict(bytes=BY, n_bytes=4000, start=ST, len=LN, ids=ID, n_tokens=NT, cap_tokens=1000, keys_out=KO, counts_out=CO,
                n_out=NO, cap=1000, ws=FAKE, ws_bytes=big, stream=None)
    keys = lambda **kw: lib.glove_phrase_bigram_keys_i32(*[{**base, **kw}[k] for k in order])
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap_tokens=-1), dict(cap_tokens=2 ** 31), dict(cap=-1), dict(bytes=None),
               dict(start=None), dict(len=None), dict(ids=None), dict(n_tokens=None), dict(keys_out=None), dict(counts_out=None),
               dict(n_out=None), dict(ws=None),
               dict(keys_out=ID), dict(keys_out=ID + 3996), dict(keys_out=ID - 7996), dict(counts_out=BY + 100), dict(n_out=ST + 8),
               dict(n_out=NT), dict(counts_out=KO + 8), dict(n_out=KO + 7992)):
        assert keys(**kw) == BADARG, kw
    assert keys(ws_bytes=16) == WORKSPACE
    assert keys(ws_bytes=lib.glove_phrase_bigram_workspace_bytes(1000) - 1) == WORKSPACE

    K, C, N, U = BY, ST, LN, ID
    order = ("keys", "counts", "n", "cap_keys", "unigram", "V", "total", "min_count", "threshold", "keys_out", "counts_out",
             "score_out", "n_out", "cap_out", "ws", "ws_bytes", "stream")
    base = dict(keys=K, counts=C, n=N, cap_keys=5000, unigram=U, V=200, total=10 ** 6, min_count=5, threshold=100.0, keys_out=KO,
                counts_out=CO, score_out=SO, n_out=NO, cap_out=5000, ws=FAKE, ws_bytes=big, stream=None)
    sel = lambda **kw: lib.glove_phrase_select(*[{**base, **kw}[k] for k in order])
    for kw in (dict(cap_keys=-1), dict(cap_keys=(1 << 40) + 1), dict(V=0), dict(V=-1), dict(total=-1), dict(min_count=0),
               dict(min_count=-3), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")),
               dict(threshold=float("inf")), dict(cap_out=-1), dict(keys=None), dict(counts=None), dict(n=None), dict(unigram=None),
               dict(keys_out=None), dict(counts_out=None), dict(score_out=None), dict(n_out=None), dict(ws=None),
               dict(keys_out=K), dict(keys_out=K + 39992), dict(score_out=U + 8), dict(n_out=C), dict(n_out=N), dict(counts_out=KO),
               dict(score_out=CO + 39992), dict(n_out=SO)):
        assert sel(**kw) == BADARG, kw
    assert sel(ws_bytes=16) == WORKSPACE
    assert sel(ws_bytes=lib.glove_phrase_select_workspace_bytes(5000) - 1) == WORKSPACE

    PK, NP, CA, JO, NJ = KO, CO, NO, SO, 0xA00000
    order = ("bytes", "n_bytes", "start", "len", "ids", "n_tokens", "cap_tokens", "phrase_keys", "n_phrases", "cap_phrases",
             "delimiter", "carry", "joined", "n_joined", "ws", "ws_bytes", "stream")
    base = dict(bytes=BY, n_bytes=4000, start=ST, len=LN, ids=ID, n_tokens=NT, cap_tokens=1000, phrase_keys=PK, n_phrases=NP,
                cap_phrases=100, delimiter=ord("_"), carry=CA, joined=JO, n_joined=NJ, ws=FAKE, ws_bytes=big, stream=None)
    join = lambda **kw: lib.glove_phrase_join_u8(*[{**base, **kw}[k] for k in order])
    for kw in (dict(n_bytes=-1), dict(n_bytes=2 ** 31), dict(cap_tokens=-1), dict(cap_tokens=2 ** 31), dict(cap_phrases=-1),
               dict(cap_phrases=2 ** 31), dict(delimiter=-1), dict(delimiter=128), dict(delimiter=255), dict(delimiter=0x20),
               dict(delimiter=0x0A), dict(delimiter=0x09), dict(delimiter=0x0D), dict(delimiter=0x1C), dict(delimiter=0x1F),
               dict(bytes=None), dict(start=None), dict(len=None), dict(ids=None), dict(n_tokens=None), dict(phrase_keys=None),
               dict(n_phrases=None), dict(carry=None), dict(joined=None), dict(n_joined=None), dict(ws=None),
               dict(joined=PK), dict(joined=PK + 792), dict(bytes=ST - 100), dict(bytes=ID + 3999), dict(carry=ID + 4),
               dict(carry=NT + 4), dict(n_joined=NP), dict(joined=BY + 3999), dict(n_joined=JO + 8), dict(carry=BY)):
        assert join(**kw) == BADARG, kw
    for ok in (0, 1, ord("+"), ord("_"), 0x0E, 0x1B, 0x21, 127):         # every other byte below 0x80 may delimit
        assert join(delimiter=ok, ws_bytes=16) == WORKSPACE, ok
    assert join(ws_bytes=lib.glove_phrase_join_workspace_bytes(1000) - 1) == WORKSPACE


# ---- the generated corpora
@pytest.fixture(scope="module")
def plain():
    """{(seed, threshold): (corpus, the rewritten corpus, the accepted table, tokens)} by the sequential restatement, once."""
    out = {}
    for seed in SEEDS:
        data = cases.generated(seed)
        for threshold in cases.THRESHOLDS:
            out[seed, threshold] = (data,) + pref.word2phrase_plain(data, 5, threshold)
    return out


def test_the_generated_corpora_exercise_the_rule(plain):
    for (seed, threshold), (data, out, accepted, tokens) in plain.items():
        runs = collections.Counter(pref.candidate_runs(data, 5, threshold))
        assert runs[1] and runs[2] and runs[3] and sum(v for k, v in runs.items() if k >= 4), (seed, threshold, runs)
        joins = sum(row[1] for row in accepted.values())
        assert joins >= 100 and joins == sum(a != b for a, b in zip(data, out)) and len(out) == len(data)
        assert tokens >= 6000 and len(data) > 20000
        for sep in cases.NON_PLAIN:                 # an accepted pair stands across every separator that breaks a phrase
            assert any(a + sep + b in out for a, b in accepted), (seed, threshold, sep)
        assert (b"hong", b"kong") in accepted and b"hong_kong" in out


def phrases_txt(accepted, delimiter=b"_"):
    """The lines of OUT.phrases.txt from the sequential restatement's table, as a set (the order is checked apart)."""
    return {a + delimiter + b + b"\t%d\t%d\t%.6f" % row for (a, b), row in accepted.items()}


def run(tmp_path, data, name, **kw):
    from trainer import phrases
    src, out = tmp_path / "corpus.txt", tmp_path / name
    src.write_bytes(data)
    report = phrases.process_corpus(src, out, backend=Backends(), **kw)
    files = [Path(str(out) + ext).read_bytes() for ext in ("", ".phrases.txt", ".phrases.json")]
    assert json.loads(files[2]) == report
    return files, report


@pytest.mark.parametrize("threshold", cases.THRESHOLDS)
@pytest.mark.parametrize("seed", SEEDS)
def test_numpy_backend_equals_the_sequential_restatement(tmp_path, plain, seed, threshold):
    data, want, accepted, tokens = plain[seed, threshold]
    results = [run(tmp_path, data, "out%d" % b, min_count=5, threshold=threshold, block_bytes=b) for b in BLOCKS]
    files, report = results[0]
    for other, _ in results[1:]:
        assert other == files                       # the corpus, the table and the counts do not depend on the blocks
    assert files[0] == want
    lines = files[1].splitlines()
    assert set(lines) == phrases_txt(accepted) and len(lines) == len(accepted)
    scores = [float(l.split(b"\t")[3]) for l in lines]
    assert scores == sorted(scores, reverse=True)
    joins = sum(row[1] for row in accepted.values())
    only = report["passes"][0]
    assert (only["tokens"], only["phrases"], only["joins"], only["tokens_out"]) == (tokens, len(accepted), joins, tokens - joins)
    words = collections.Counter(data[s:s + n] for s, n in text_ref.token_spans(data))
    assert only["types"] == len(words) and only["kept_types"] == sum(v >= 5 for v in words.values())
    assert report["options"] == {"min_count": 5, "threshold": threshold, "delimiter": "_", "passes": 1}
    assert len(text_ref.token_spans(files[0])) == only["tokens_out"]


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_cases(tmp_path, name):
    data, options, want = EDGES[name]
    kw = {"min_count": 5, "threshold": 100.0, "delimiter": "_", **options}
    ref, accepted, tokens = pref.word2phrase_plain(data, kw["min_count"], kw["threshold"], kw["delimiter"].encode())
    assert want is None or ref == want              # the restatement gives what was written down by hand
    for b in BLOCKS:
        files, report = run(tmp_path, data, "out%d" % b, block_bytes=b, **kw)
        assert files[0] == ref, b
        assert set(files[1].splitlines()) == phrases_txt(accepted, kw["delimiter"].encode())
        assert report["passes"][0]["tokens"] == tokens and report["passes"][0]["joins"] == sum(r[1] for r in accepted.values())


def test_edge_cases_say_what_they_claim():
    assert EDGES["alternating_40"][2].startswith(b"x_y x_y x_y") and EDGES["alternating_40"][2].endswith(b" x_y")
    assert EDGES["alternating_41"][2].endswith(b" x_y x")
    data, options, _ = EDGES["score_equals_threshold"]
    _, accepted, tokens = pref.word2phrase_plain(data, options["min_count"], 1.0)
    assert tokens == 64 and accepted[b"a", b"b"] == (8, 8, 4.0)            # the score IS the threshold of the case, bit for bit
    data, options, _ = EDGES["count_at_and_above_min_count"]
    words = collections.Counter(data.split())
    pairs = collections.Counter(re.findall(rb"(\w+) (\w+)", data))
    assert pairs[b"p", b"q"] == 5 and pairs[b"r", b"s"] == 6 and words[b"p"] == 5
    data, _, _ = EDGES["rare_word_in_strong_pair"]
    assert collections.Counter(data.split())[b"m"] == 4
    assert max(len(w) for w in EDGES["token_longer_than_the_block"][0].split()) > 257
    assert not EDGES["no_separator_at_the_end"][0][-1:].isspace()


# ---- passes
def test_two_passes_equal_running_the_tool_twice(tmp_path, plain):
    data = plain[SEEDS[0], 10.0][0]
    (twice, table, _), report = run(tmp_path, data, "twice", min_count=5, threshold=10.0, passes=2, block_bytes=257)
    (first, first_table, _), first_report = run(tmp_path, data, "first", min_count=5, threshold=10.0)
    (second, second_table, _), second_report = run(tmp_path, first, "second", min_count=5, threshold=10.0)
    assert twice == second and table == second_table
    assert any(tok.count(b"_") >= 2 for tok in twice.split())              # new_york_city, a1_a2_a3_a4, ...
    assert b"a1_a2_a3_a4 a5" in twice and b"san_francisco_bay_area" in twice
    assert not (tmp_path / "twice.pass1").exists()
    stripped = [{k: v for k, v in p.items() if k != "table"} for p in report["passes"]]
    assert stripped == first_report["passes"] + second_report["passes"]
    want = [l.split(b"\t") for l in first_table.splitlines()]
    assert report["passes"][0]["table"] == [[w[0].decode(), int(w[1]), int(w[2]), pytest.approx(float(w[3]), abs=1e-6)] for w in want]
    assert "table" not in report["passes"][1]
    # the sequential restatement, twice
    once = pref.word2phrase_plain(data, 5, 10.0)[0]
    assert twice == pref.word2phrase_plain(once, 5, 10.0)[0]


# ---- the command line and its refusals
def test_the_command_line_writes_its_three_files(tmp_path, plain):
    from trainer import phrases
    data, want, _, _ = plain[SEEDS[0], 100.0]
    (tmp_path / "in.txt").write_bytes(data)
    phrases.main(["--corpus", str(tmp_path / "in.txt"), "--output", str(tmp_path / "out.txt"), "--block-bytes", "4096"], backend=Backends())
    assert sorted(p.name for p in tmp_path.iterdir()) == ["in.txt", "out.txt", "out.txt.phrases.json", "out.txt.phrases.txt"]
    assert (tmp_path / "out.txt").read_bytes() == want                     # the defaults are word2phrase's: 5, 100, "_"
    phrases.main(["--corpus", str(tmp_path / "in.txt"), "--output", str(tmp_path / "plus.txt"), "--min-count", "5", "--threshold", "10",
                  "--delimiter", "+", "--passes", "2"], backend=Backends())
    assert b"san+francisco+bay+area" in (tmp_path / "plus.txt").read_bytes()


def test_bad_options_are_refused_before_the_corpus_is_opened(tmp_path):
    from trainer import phrases
    missing = tmp_path / "no_such_corpus.txt"
    for kw in (dict(min_count=0), dict(min_count=-1), dict(threshold=0.0), dict(threshold=-5.0), dict(threshold=float("nan")),
               dict(threshold=float("inf")), dict(delimiter=""), dict(delimiter="__"), dict(delimiter="é"), dict(delimiter=" "),
               dict(delimiter="\n"), dict(delimiter="\t"), dict(delimiter="\x1f"), dict(passes=0), dict(passes=-2)):
        with pytest.raises(ValueError):
            phrases.process_corpus(missing, tmp_path / "out.txt", backend=Backends(), **kw)
    with pytest.raises(ValueError, match="corpus itself"):
        phrases.process_corpus(missing, tmp_path / "sub" / ".." / "no_such_corpus.txt", backend=Backends())
    with pytest.raises(ValueError, match="corpus itself"):
        phrases.process_corpus(str(missing) + ".pass1", missing, passes=2, backend=Backends())
    with pytest.raises(FileNotFoundError):                                  # good options get as far as the file
        phrases.process_corpus(missing, tmp_path / "out.txt", backend=Backends())
    assert not (tmp_path / "out.txt").exists()


def test_errors_of_the_tokenizer_are_errors_here(tmp_path):
    from trainer import phrases
    (tmp_path / "long.txt").write_bytes(b"a " + b"z" * 65536 + b" b\n")
    with pytest.raises(ValueError, match="longer than 65535"):
        phrases.process_corpus(tmp_path / "long.txt", tmp_path / "out.txt", backend=Backends())

    class Colliding(Backends):                      # every token of the second read looks like a hash collision
        def text_token_ids(self, block, start, length, hashes, kept):
            ids, _ = super().text_token_ids(block, start, length, hashes, kept)
            return ids, 3
    (tmp_path / "ok.txt").write_bytes(b"a b\n" * 9)
    with pytest.raises(ValueError, match="hash collision"):
        phrases.process_corpus(tmp_path / "ok.txt", tmp_path / "out.txt", backend=Colliding())


# ---- the next stage
def test_cooccur_on_the_output_numbers_the_phrases(tmp_path, plain):
    from trainer import cooccur
    data, want, _, _ = plain[SEEDS[0], 10.0]
    (files, _) = run(tmp_path, data, "phrased.txt", min_count=5, threshold=10.0)
    assert files[0] == want
    cooccur.main(str(tmp_path / "phrased.txt"), tmp_path / "prep", vocab_size=None, coverage=0.9, context_size=5, chunk_tokens=1000,
                 count_minimum=10, seed=3, backend=Backends(), tokenizer="device", block_bytes=4096)
    vocab = (tmp_path / "prep" / "vocab.txt").read_text().split()
    assert "new_york" in vocab and "los_angeles" in vocab and "new york" not in " ".join(vocab)
