"""`python -m trainer.wordsim --job-dir J --pairs FILE [--embeddings row|col|sum] [--restrict-vocab N] [--no-lowercase]
[--delimiter D] [--score-column 3]`

Scores a word-similarity dataset (WordSim-353's combined.tab, MEN, RW; SimLex-999 with --score-column 4) against the newest
checkpoint of J: the cosine of every word pair on the GPU (include/glove_eval_sim_hip.h) against the file's human scores,
by Spearman's rank correlation (what the GloVe paper reports; gensim's evaluate_word_pairs) and Pearson's.  The reference
does not have this.  Writes J/eval/wordsim.json.  One process, like trainer.analogy.

This module holds the file format and the statistics; `Estimator.evaluate_word_pairs` does the work.
"""
from __future__ import annotations

import argparse
import json
import logging
from pathlib import Path

import numpy as np

from trainer import config
from trainer.analogy import EMBEDDINGS, SKIPPED_TOKEN

logger = logging.getLogger(__name__)


def _number(text):
    """The finite number `text` spells, or None."""
    try:
        x = float(text)
    except ValueError:
        return None
    return x if np.isfinite(x) else None


def parse_pairs(path, lowercase=True, delimiter=None, score_column=3) -> list:
    """[(line number, word1, word2, score), ...] in file order.  One pair per line, `word1 word2 ... score` split on
    whitespace or on `delimiter`, the score in column `score_column` (counted from 1, at least 3).  Blank lines and lines
    starting with `#` are skipped; the first remaining line is a header, and skipped, if its score column is no number.
    Any later line with fewer columns or a score that is no number is an error that names it."""
    if score_column < 3:
        raise ValueError("--score-column must be at least 3 (two words come first), got %r" % (score_column,))
    rows, first = [], True
    with open(path, encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            fields = [x.strip() for x in line.rstrip("\r\n").split(delimiter)] if delimiter else line.split()
            score = _number(fields[score_column - 1]) if len(fields) >= score_column else None
            header, first = first, False
            if score is None:
                if header:
                    continue
                raise ValueError("%s line %d: expected at least %d columns with a number in column %d"
                                 % (path, lineno, score_column, score_column))
            words = (fields[0], fields[1])
            rows.append((lineno,) + (tuple(w.lower() for w in words) if lowercase else words) + (score,))
    return rows


def lookup_pairs(rows, vocab, limit=None):
    """Pair words -> ids, under the rules of analogy.lookup_questions.  `vocab`: tokens in id order, used as they are;
    `limit`: ids from it on do not exist (--restrict-vocab).  Returns (ids [(i, j), ...] of the pairs kept, in order,
    their scores, the number of pairs skipped).  A pair is skipped when one of its words is missing, is "<UNK>", or lies
    at or beyond the limit."""
    ids_of = {}
    for i, token in enumerate(vocab):
        if token != SKIPPED_TOKEN and (limit is None or i < limit):
            ids_of.setdefault(token, i)
    ids, scores = [], []
    for _, w1, w2, score in rows:
        i, j = ids_of.get(w1), ids_of.get(w2)
        if i is None or j is None:
            continue
        ids.append((i, j))
        scores.append(score)
    return ids, scores, len(rows) - len(ids)


def average_ranks(x) -> np.ndarray:
    """Ranks from 1 in float64; ties share the mean of the ranks they cover."""
    x = np.asarray(x, np.float64)
    order = np.argsort(x, kind="stable")
    s = x[order]
    start = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])            # where a run of equal values begins
    end = np.r_[start[1:], len(s)]
    ranks = np.empty(len(s), np.float64)
    ranks[order] = np.repeat((start + 1 + end) / 2.0, end - start)  # mean of start + 1 .. end
    return ranks


def pearson(x, y):
    """Pearson's r in float64, or None with fewer than two values or a constant side."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if len(x) != len(y):
        raise ValueError("pearson: %d and %d values" % (len(x), len(y)))
    if len(x) < 2:
        return None
    dx, dy = x - x.mean(), y - y.mean()
    sx, sy = np.sqrt((dx * dx).sum()), np.sqrt((dy * dy).sum())
    if sx == 0.0 or sy == 0.0:
        return None
    return float(np.clip((dx / sx) @ (dy / sy), -1.0, 1.0))


def spearman(x, y):
    """Spearman's rho: Pearson's r of the average ranks; None where pearson is."""
    if len(x) != len(y):
        raise ValueError("spearman: %d and %d values" % (len(x), len(y)))
    return pearson(average_ranks(x), average_ranks(y))


def main(job_dir=config.JOB_DIR, pairs=None, embeddings="row", restrict_vocab=None, no_lowercase=False, delimiter=None,
         score_column=3, **_):
    from trainer.estimator import Estimator
    params = json.loads(Path(job_dir, "params.json").read_text())
    return Estimator(params).evaluate_word_pairs(pairs, embeddings=embeddings, restrict_vocab=restrict_vocab,
                                                 lowercase=not no_lowercase, delimiter=delimiter, score_column=score_column)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0], formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    cli.add_argument("--job-dir", default=config.JOB_DIR, help="job directory of a finished or running training")
    cli.add_argument("--pairs", required=True, help="pairs file: lines of `word1 word2 score`; # lines and one header line are skipped")
    cli.add_argument("--embeddings", choices=EMBEDDINGS, default="row", help="row table, col table, or their sum (the GloVe paper's W + W~)")
    cli.add_argument("--restrict-vocab", type=int, default=None, help="use the first N vocabulary rows only")
    cli.add_argument("--no-lowercase", action="store_true", help="take the words as written instead of lowercasing them")
    cli.add_argument("--delimiter", default=None, help="column separator (default: any whitespace)")
    cli.add_argument("--score-column", type=int, default=3, help="column of the human score, counted from 1 (SimLex-999: 4)")
    try:
        main(**vars(cli.parse_args()))
    except KeyboardInterrupt:
        pass
