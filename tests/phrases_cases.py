"""Corpora for the phrase-detection tests: a seeded generator with planted collocations and every separator kind, and
the edge cases of the rule (include/glove_phrases_hip.h), each with the options it is run under.  Shared by
tests/test_phrases.py (NumPy backend) and tests/test_gpu_phrases.py (GloveHip)."""
import numpy as np

CHAINS = [b"new york", b"new york city", b"san francisco bay area", b"a1 a2 a3 a4 a5", b"los angeles"]
SEPARATORS = [b" ", b"\n", b"  ", b"\t", b"\xc2\xa0", b" \n"]
SEPARATOR_WEIGHTS = [0.90, 0.04, 0.02, 0.02, 0.01, 0.01]
NON_PLAIN = SEPARATORS[1:]
THRESHOLDS = (10.0, 100.0)
FILLERS = 150


def generated(seed: int, n_tokens: int = 6000) -> bytes:
    """About 30 KB: FILLERS filler words drawn Zipf(1); 3 % of the draws insert one of CHAINS, whose inner separators are a
    single space with probability 0.95; every other separator is drawn from SEPARATORS.  Every 375 tokens "hong kong" is
    planted, seen nowhere else: ten times on a single space and once across each of the NON_PLAIN separators, so it is
    accepted at both THRESHOLDS (5 / 15 / 15 * 6000 = 133), stands alone as a candidate run of length one, and every
    separator kind breaks an accepted pair somewhere."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, FILLERS + 1)
    p /= p.sum()
    draw_sep = lambda: SEPARATORS[rng.choice(len(SEPARATORS), p=SEPARATOR_WEIGHTS)]
    out, n, planted = [], 0, 0
    while n < n_tokens:
        if n >= 375 * (planted + 1):
            out += [b"hong", NON_PLAIN[planted // 3 % len(NON_PLAIN)] if planted % 3 == 2 else b" ", b"kong", draw_sep()]
            planted += 1
            n += 2
        elif rng.random() < 0.03:
            chain = CHAINS[rng.integers(len(CHAINS))].split()
            for i, word in enumerate(chain):
                inner = i + 1 < len(chain) and rng.random() < 0.95
                out += [word, b" " if inner else draw_sep()]
            n += len(chain)
        else:
            out += [b"w%d" % rng.choice(FILLERS, p=p), draw_sep()]
            n += 1
    return b"".join(out)


def alternating(n_tokens: int) -> bytes:
    """x y x y ... on single spaces: one candidate run of n_tokens - 1 pairs at min_count 5, threshold 1."""
    return b" ".join([b"x", b"y"][i & 1] for i in range(n_tokens))


def alternating_joined(n_tokens: int, delimiter=b"_", flipped=False) -> bytes:
    """What the rule makes of it: x_y x_y ... (a last x stays alone); flipped (the pair in front of the block was joined):
    x y_x y_x ..."""
    out = bytearray(alternating(n_tokens))
    for t in range(n_tokens - 1):
        if (t & 1) == (1 if flipped else 0):
            out[2 * t + 1] = delimiter[0]
    return bytes(out)


def _lines(*groups) -> bytes:
    """Every (line, times) on lines of its own: the newline keeps a line's last word from pairing with the next line's first."""
    return b"".join((line + b"\n") * times for line, times in groups)


def _fillers(n: int, prefix=b"f") -> bytes:
    return b"".join(prefix + b"%d\n" % i for i in range(n))


# name -> (corpus, options, the expected output where it is written down by hand, else None)
def edge_cases() -> dict:
    cases = {}
    for n in (40, 41):
        cases["alternating_%d" % n] = (alternating(n), dict(min_count=5, threshold=1.0), alternating_joined(n))
    # score == threshold exactly, in powers of two: n_ab - min_count = 4, n_a = n_b = 8, N = 64: 4 / 8 / 8 * 64 = 4.0
    exact = _lines((b"a b", 8)) + _fillers(48)
    cases["score_equals_threshold"] = (exact, dict(min_count=4, threshold=4.0), exact)
    cases["score_above_threshold"] = (exact, dict(min_count=4, threshold=3.999), exact.replace(b"a b", b"a_b"))
    # n_ab == min_count scores 0; min_count + 1 scores 1 / 6 / 6 * 200 = 5.55...
    counts = _lines((b"p q", 5), (b"r s", 6)) + _fillers(178)
    cases["count_at_and_above_min_count"] = (counts, dict(min_count=5, threshold=1.0), counts.replace(b"r s", b"r_s"))
    # m is seen min_count - 1 times: it is no kept word, whatever "k m" would score
    rare = _lines((b"k m", 4), (b"k z", 10)) + _fillers(100)
    cases["rare_word_in_strong_pair"] = (rare, dict(min_count=5, threshold=1.0), rare.replace(b"k z", b"k_z"))
    high = _lines((b"caf\xc3\xa9 cr\xc3\xa8me", 8), (b"na\xefve \xff\xfe", 7)) + _fillers(60)
    cases["bytes_above_0x7f"] = (high, dict(min_count=5, threshold=1.0),
                                 high.replace(b"caf\xc3\xa9 cr", b"caf\xc3\xa9_cr").replace(b"na\xefve \xff", b"na\xefve_\xff"))
    ends = _fillers(30) + _lines((b"g h", 7))[:-1]
    cases["no_separator_at_the_end"] = (ends, dict(min_count=5, threshold=1.0), ends.replace(b"g h", b"g_h"))
    cases["empty"] = (b"", dict(), b"")
    cases["one_token"] = (b"alone", dict(), b"alone")
    cases["separators_only"] = (b" \n\t \xc2\xa0 \n", dict(), b" \n\t \xc2\xa0 \n")
    long_token = b"L" * 300
    longer = _lines((long_token + b" tail", 9)) + _fillers(20)
    cases["token_longer_than_the_block"] = (longer, dict(min_count=5, threshold=1.0), longer.replace(b"L tail", b"L_tail"))
    other = _lines((b"c d", 9)) + _fillers(40)
    cases["other_delimiter"] = (other, dict(min_count=5, threshold=1.0, delimiter="+"), other.replace(b"c d", b"c+d"))
    return cases
