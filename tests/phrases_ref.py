"""Two independent restatements of include/glove_phrases_hip.h.

word2phrase_plain reads a corpus the way word2phrase.c does: sequentially, with dicts and a left-to-right `prev_joined`
flag, on the header's tokens (text_ref.token_spans).  NumpyPhrasesBackend states the three device operations as array
operations (np.unique, searchsorted, a running maximum), carry word included; with text_ref.NumpyTextBackend and
cooc_stream_ref.NumpyBackend it is a backend trainer.phrases runs on (the product backend is GloveHip).  Keys travel as
int64: an id is below 2^31, so (a << 32 | b) is the same number as the header's uint64."""
import numpy as np

import text_ref


def word2phrase_plain(data: bytes, min_count=5, threshold=100.0, delimiter=b"_"):
    """(the rewritten bytes, {(word a, word b): (bigram count, joins, score)} of the accepted bigrams, the token count)."""
    spans = text_ref.token_spans(data)
    words = [data[s:s + n] for s, n in spans]
    total = len(words)
    unigram = {}
    for w in words:
        unigram[w] = unigram.get(w, 0) + 1

    def plain(t):
        s, n = spans[t]
        return spans[t + 1][0] == s + n + 1 and data[s + n:s + n + 1] == b" "

    bigram = {}
    for t in range(total - 1):
        a, b = words[t], words[t + 1]
        if plain(t) and unigram[a] >= min_count and unigram[b] >= min_count:
            bigram[(a, b)] = bigram.get((a, b), 0) + 1
    accepted = {}
    for (a, b), n_ab in bigram.items():
        if n_ab < min_count:
            continue
        score = float(n_ab - min_count) / float(unigram[a]) / float(unigram[b]) * float(total)
        if score > threshold:
            accepted[(a, b)] = [n_ab, 0, score]
    out = bytearray(data)
    prev_joined = False
    for t in range(total - 1):
        pair = (words[t], words[t + 1])
        if not prev_joined and plain(t) and pair in accepted:
            s, n = spans[t]
            out[s + n] = delimiter[0]
            accepted[pair][1] += 1
            prev_joined = True
        else:
            prev_joined = False
    return bytes(out), {k: tuple(v) for k, v in accepted.items()}, total


def candidate_runs(data: bytes, min_count=5, threshold=100.0):
    """The lengths of the maximal runs of consecutive candidate pairs (plain and accepted), in corpus order."""
    _, accepted, _ = word2phrase_plain(data, min_count, threshold)
    spans = text_ref.token_spans(data)
    words = [data[s:s + n] for s, n in spans]
    runs, run = [], 0
    for t in range(len(words) - 1):
        s, n = spans[t]
        if spans[t + 1][0] == s + n + 1 and data[s + n:s + n + 1] == b" " and (words[t], words[t + 1]) in accepted:
            run += 1
        else:
            if run:
                runs.append(run)
            run = 0
    if run:
        runs.append(run)
    return runs


# ---- the three device operations on arrays ------------------------------------------------------------------------------
def pair_keys(block, start, length, ids):
    """int64 [n - 1]: the key of every adjacent pair, -1 where the pair is not plain or an id is not a kept word's."""
    block = np.asarray(block, np.uint8)
    start, length, ids = (np.asarray(a, np.int64) for a in (start, length, ids))
    if len(ids) < 2:
        return np.zeros(0, np.int64)
    sep = start[:-1] + length[:-1]
    inside = (sep >= 0) & (sep < len(block))
    space = np.zeros(len(sep), bool)
    space[inside] = block[sep[inside]] == 0x20
    ok = space & (start[1:] == sep + 1) & (ids[:-1] > 0) & (ids[1:] > 0)
    return np.where(ok, (ids[:-1] << 32) | ids[1:], -1)


def bigram_keys(block, start, length, ids):
    keys = pair_keys(block, start, length, ids)
    uk, cnt = np.unique(keys[keys >= 0], return_counts=True)
    return uk.astype(np.int64), cnt.astype(np.int64)


def select(keys, counts, unigram, total_tokens, min_count, threshold):
    keys, counts, unigram = (np.asarray(a, np.int64) for a in (keys, counts, unigram))
    a, b = keys >> 32, keys & 0xFFFFFFFF
    V = len(unigram)
    known = (a >= 1) & (a < V) & (b >= 1) & (b < V)
    n_a, n_b = unigram[np.where(known, a, 0)], unigram[np.where(known, b, 0)]
    known &= (n_a >= 1) & (n_b >= 1) & (counts >= min_count)
    score = np.zeros(len(keys), np.float64)
    # one rounding per operation, in the header's order
    score[known] = (counts[known] - np.int64(min_count)).astype(np.float64) / n_a[known].astype(np.float64) \
        / n_b[known].astype(np.float64) * np.float64(total_tokens)
    take = known & (score > np.float64(threshold))
    return keys[take], counts[take], score[take]


def join(block, start, length, ids, phrase_keys, delimiter, carry, joined):
    """In place on block, carry and joined; -> the block's joins."""
    keys = pair_keys(block, start, length, ids)
    if len(keys) == 0:
        return 0
    phrase_keys = np.asarray(phrase_keys, np.int64)
    at = np.searchsorted(phrase_keys, keys)
    cand = np.zeros(len(keys), bool)
    if len(phrase_keys):
        inside = at < len(phrase_keys)
        cand[inside] = (phrase_keys[at[inside]] == keys[inside]) & (keys[inside] >= 0)
    t = np.arange(len(keys), dtype=np.int64)
    # b(t): the last non-candidate index < t; in front of the block stands -1, or a chosen candidate -1 behind -2
    front = np.int64(-2 if int(carry[0]) else -1)
    last = np.maximum.accumulate(np.where(cand, front, t))
    b = np.concatenate([[front], last[:-1]])
    chosen = cand & (((t - b) & 1) == 1)
    where = np.asarray(start, np.int64)[:-1][chosen] + np.asarray(length, np.int64)[:-1][chosen]
    block[where] = delimiter
    np.add.at(joined, at[chosen], 1)
    carry[0] = 1 if chosen[-1] else 0
    return int(chosen.sum())


class NumpyPhrasesBackend:
    """The phrase operations of a trainer.phrases backend on numpy arrays (no `device`)."""

    def phrase_bigram_keys(self, block, start, length, ids):
        return bigram_keys(block, start, length, ids)

    def phrase_select(self, keys, counts, unigram, total_tokens, min_count, threshold):
        return select(keys, counts, unigram, total_tokens, min_count, threshold)

    def phrase_join(self, block, start, length, ids, phrase_keys, delimiter, carry, joined):
        return join(block, start, length, ids, phrase_keys, delimiter, carry, joined)
